"""Rendered overlay frames on the device: ops.render_overlay against the numpy restatement of its rule (tests/_overlay_ref.py), and the
surfaces above it (model.overlay_output / overlay_style, online_video(emit="overlay")).  The rule is integers only, so every comparison is
torch.equal: there is no tolerance anywhere.

Kernel shapes: the smallest at which it can go wrong -- nothing divides by 4 (a thread's group of 4 pixels straddles rows and frames, the
output starts at an odd byte with f_off = 1), up- and down-sampling, a row shorter than one group, every alignment of the output address.
The model cases use the set-up of test_label_map_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5 frames."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _overlay_ref as REF  # noqa: E402

SIZES = [(61, 97, 61, 97), (60, 90, 120, 180), (96, 160, 61, 97), (5, 7, 1, 3)]      # (h0, w0, Ho, Wo)
F = 3
A256 = (0, 1, 128, 255, 256)


def _rects(rng, Ho, Wo):
    """Random rectangles of labels (1 and 255 among them), regions on all four borders, single-pixel regions."""
    lab = np.zeros((Ho, Wo), dtype=np.uint8)
    for l in [1, 255] + rng.integers(1, 256, size=8).tolist():
        y0, x0 = int(rng.integers(0, Ho)), int(rng.integers(0, Wo))
        lab[y0:y0 + int(rng.integers(1, Ho // 2 + 2)), x0:x0 + int(rng.integers(1, Wo // 2 + 2))] = l
    lab[0, :max(1, Wo // 3)] = 1                                      # top
    lab[-1, Wo // 2:] = 255                                           # bottom
    lab[:max(1, Ho // 2), 0] = 17                                     # left
    lab[Ho // 3:, -1] = 99                                            # right
    for _ in range(6):
        lab[int(rng.integers(0, Ho)), int(rng.integers(0, Wo))] = int(rng.integers(1, 256))
    return lab


def _label_sets(Ho, Wo, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:Ho, :Wo]
    checker = np.where((yy + xx) % 2 == 0, 7, 200).astype(np.uint8)  # every pixel with a neighbour inside is an edge
    a = np.stack([_rects(rng, Ho, Wo), checker, np.zeros((Ho, Wo), dtype=np.uint8)])
    b = np.stack([np.full((Ho, Wo), 1, dtype=np.uint8), _rects(rng, Ho, Wo), _rects(rng, Ho, Wo)])
    return [a, b]


def _frames(kind, n, h0, w0, seed):
    """-> (tensor handed to the wrapper, the same frames as numpy [n, 3, h0, w0] for the painter); kind: u8 | f32 | none | strided."""
    g = torch.Generator().manual_seed(seed)
    if kind == "none":
        return None, None
    if kind == "f32":
        # exact integers, k + 0.5 (half to even), values below 0 and above 255, NaN
        fr = torch.randint(-40, 600, (n, 3, h0, w0), generator=g).float() * 0.5
        fr[torch.rand(fr.shape, generator=g) < 0.02] = float("nan")
        fr.view(-1)[:6] = torch.tensor([0.5, 1.5, 2.5, 254.5, 255.5, -0.5])
        return fr.cuda(), fr.numpy()
    if kind == "strided":                                             # every second frame of a twice-as-long buffer
        buf = torch.randint(0, 256, (2 * n, 3, h0, w0), generator=g, dtype=torch.uint8)
        view = buf.cuda()[::2]
        assert not view.is_contiguous() or n == 1
        return view, buf[::2].numpy()
    fr = torch.randint(0, 256, (n, 3, h0, w0), generator=g, dtype=torch.uint8)
    return fr.cuda(), fr.numpy()


def _palettes():
    from mdqe_cvpr2023_amd.render import default_palette
    rnd = torch.randint(0, 256, (256, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    return [default_palette(), rnd]


def _check(lab, fr_dev, fr_np, pal, f_off, a256, contour):
    """One launch against the painter, with guard frames in front and behind."""
    from mdqe_cvpr2023_amd import ops
    n, Ho, Wo = lab.shape
    out = torch.full((f_off + n + 1, Ho, Wo, 3), 0xAB, dtype=torch.uint8, device="cuda")
    got = ops.render_overlay(torch.from_numpy(lab).cuda(), fr_dev, pal.cuda(), out, f_off, a256, contour)
    assert got is out
    o = out.cpu()
    want = torch.from_numpy(REF.paint(lab, fr_np, pal.numpy(), a256, contour))
    assert torch.equal(o[f_off:f_off + n], want), (lab.shape, f_off, a256, contour)
    assert bool((o[:f_off] == 0xAB).all()) and bool((o[f_off + n:] == 0xAB).all())
    return o[f_off:f_off + n]


@pytest.mark.parametrize("kind", ["u8", "f32", "none", "strided"])
@pytest.mark.parametrize("size", SIZES)
def test_render_overlay_against_the_painter(size, kind):
    h0, w0, Ho, Wo = size
    sets = _label_sets(Ho, Wo, seed=Ho * 1000 + Wo)
    fr_dev, fr_np = _frames(kind, F, h0, w0, seed=h0 + w0)
    pals = _palettes()
    # every contour reach x every blend weight on one set of labels ...
    for contour in range(4):
        for a256 in A256:
            _check(sets[0], fr_dev, fr_np, pals[0], 1, a256, contour)       # (61 x 97: f_off = 1 starts at an odd byte)
    # ... and the other labels, palette and offset with the parameters rotating
    k = 0
    for lab in sets:
        for pal in pals:
            for f_off in (0, 1):
                _check(lab, fr_dev, fr_np, pal, f_off, A256[k % 5], k % 4)
                k += 1
    if kind == "u8":                                                  # a256 = 0 without contours is the (nearest-sampled) source itself
        got = _check(sets[1], fr_dev, fr_np, pals[1], 0, 0, 0)
        sy, sx = (np.arange(Ho) * h0) // Ho, (np.arange(Wo) * w0) // Wo
        assert np.array_equal(got.numpy(), np.moveaxis(fr_np[:, :, sy][:, :, :, sx], 1, -1))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_alignment_of_the_output_and_runs_are_identical(shift):
    """The output begins `shift` bytes behind an aligned address: 0..3 single pixels in front of the first 12-byte group, and as many as
    are left behind the last; a single frame and one of two pixels (fewer than one group) as well."""
    from mdqe_cvpr2023_amd import ops
    pal = _palettes()[1]
    for n, Ho, Wo in ((2, 13, 9), (1, 1, 2), (1, 2, 3), (1, 1, 1)):
        rng = np.random.default_rng(n * Ho + Wo)
        lab = rng.integers(0, 4, size=(n, Ho, Wo)).astype(np.uint8) * 85
        fr = torch.randint(0, 256, (n, 3, Ho, Wo), generator=torch.Generator().manual_seed(Ho), dtype=torch.uint8)
        nb = n * Ho * Wo * 3
        raw = torch.full((nb + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        out = raw[shift:shift + nb].view(n, Ho, Wo, 3)
        assert out.is_contiguous() and out.data_ptr() % 4 == shift
        args = (torch.from_numpy(lab).cuda(), fr.cuda(), pal.cuda())
        ops.render_overlay(*args, out, 0, 77, 2)
        want = torch.from_numpy(REF.paint(lab, fr.numpy(), pal.numpy(), 77, 2))
        r = raw.cpu()
        assert torch.equal(r[shift:shift + nb].view(n, Ho, Wo, 3), want), (shift, n, Ho, Wo)
        assert bool((r[:shift] == 0xAB).all()) and bool((r[shift + nb:] == 0xAB).all())
        again = torch.empty_like(out)
        ops.render_overlay(*args, again, 0, 77, 2)
        assert torch.equal(again, out)                                # identical from run to run


def test_no_frames_to_paint_is_no_launch():
    from mdqe_cvpr2023_amd import ops
    pal = _palettes()[0].cuda()
    out = torch.full((2, 4, 5, 3), 0xAB, dtype=torch.uint8, device="cuda")
    ops.render_overlay(torch.zeros(0, 4, 5, dtype=torch.uint8, device="cuda"), None, pal, out, 1)
    ops.render_overlay(torch.zeros(0, 4, 5, dtype=torch.uint8, device="cuda"), torch.zeros(0, 3, 4, 5, device="cuda"), pal, out, 2)
    assert bool((out == 0xAB).all())


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)
    return cfg, MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()


L, OUT = 17, (90, 150)
SETTINGS = {"off": {}, "lab": {"label_output": True}, "geo": {"label_output": True, "geometry_output": True}, "rle": {"rle_output": True},
            "late": {"early_masks": False}, "late_lab": {"early_masks": False, "label_output": True},
            # every plane, label, overlay and geometry form together, through the early path and through the late one
            "rle_lab_geo": {"rle_output": True, "label_output": True, "geometry_output": True},
            "late_rle_lab_geo": {"rle_output": True, "label_output": True, "geometry_output": True, "early_masks": False}}


def _forward(model, frames, **attrs):
    """forward() with the given attributes set, everything restored behind it."""
    names = ("label_output", "geometry_output", "rle_output", "early_masks", "overlay_output", "overlay_style")
    saved = {k: getattr(model, k) for k in names}
    try:
        for k, v in attrs.items():
            setattr(model, k, v)
        return model([{"image": frames, "height": OUT[0], "width": OUT[1]}])
    finally:
        for k, v in saved.items():
            setattr(model, k, v)


@pytest.fixture(scope="module", params=[None, 1e-6], ids=["thr_default", "thr_1e-6"])
def model_video(request):
    """One 17-frame video (three tracker windows of 6, 6, 5 frames) through forward() in every setting with the overlay off and on,
    once.  With the preset's class threshold the random weights leave the tracker one track; lowered to 1e-6 many tracks compete."""
    from bench import synth_video
    _, model = _model(n_frames_window_test=6) if request.param is None else _model(n_frames_window_test=6, apply_cls_thres=request.param)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    assert model.overlay_output is False
    runs = {}
    for name, attrs in SETTINGS.items():
        runs[name] = _forward(model, frames, **attrs)
        runs[name + "+ov"] = _forward(model, frames, overlay_output=True, **attrs)
    assert model.overlay_output is False
    return model, frames, runs


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    return a == b


def _paint(labels, frames, style=None):
    from mdqe_cvpr2023_amd.render import Style
    st = style if style is not None else Style()
    pal = st.palette_on("cpu")
    return torch.from_numpy(REF.paint(labels.numpy(), frames.cpu().numpy(), pal.numpy(), st.a256, st.contour))


def test_model_overlay_output_every_path_and_nothing_else_changes(model_video):
    model, frames, runs = model_video
    lm = runs["lab"]["pred_label_map"]
    want = _paint(lm, frames)
    assert int(lm.max()) > 0 and not torch.equal(want, _paint(torch.zeros_like(lm), frames))     # (something is painted)
    for name in SETTINGS:
        off, on = runs[name], runs[name + "+ov"]
        pic = on["pred_overlay"]
        assert pic.dtype == torch.uint8 and tuple(pic.shape) == (L,) + OUT + (3,) and not pic.is_cuda and pic.is_pinned()
        assert torch.equal(pic, want), name                           # early and late path, with and without the other outputs
        assert set(on) == set(off) | {"pred_overlay", "pred_track_ids"}, name
        assert ("pred_label_map" in on) == ("lab" in name or name == "geo")       # without label_output the map is a device scratch
        for k in off:                                                 # every other key: the bits of the run with the overlay off
            assert _same(on[k], off[k]), (name, k)
        assert on["pred_track_ids"] == runs["lab"]["pred_track_ids"] and len(on["pred_track_ids"]) == len(on["pred_scores"])
    assert "pred_label_boxes" in runs["geo+ov"] and "pred_rles" in runs["rle+ov"]


def _online(model, frames, sizes, **kw):
    ov = model.online_video(height=OUT[0], width=OUT[1], **kw)
    wins, a, held = [], 0, []
    for n in sizes:
        wins += ov.push(frames[a:a + n])
        a += n
        emitted = wins[-1].frames[1] if wins else 0
        held.append((ov.frames_held, ov.received - emitted))
    wins += ov.close()
    return ov, wins, held


PLANS = ([L], [1] * L, [min(5, L - a) for a in range(0, L, 5)])


def test_online_overlay_windows(model_video):
    model, frames, runs = model_video
    want = runs["off+ov"]["pred_overlay"]
    _, ref_wins, _ = _online(model, frames, [L], emit="labels", geometry=True)
    assert [w.frames for w in ref_wins] == [(0, 6), (6, 12), (12, 17)]
    print("tracks per window:", [len(w.track_ids) for w in ref_wins])
    for sizes in PLANS:
        ov, wins, held = _online(model, frames, sizes, emit="overlay", keep=True, geometry=True)
        assert [w.frames for w in wins] == [w.frames for w in ref_wins]
        for w, r in zip(wins, ref_wins):
            f0, f1 = w.frames
            assert w.masks is None and w.rles is None and w.track_ids == r.track_ids
            assert torch.equal(w.labels, r.labels)                    # what emit="labels" gives
            assert w.overlay.dtype == torch.uint8 and tuple(w.overlay.shape) == (f1 - f0,) + OUT + (3,)
            assert torch.equal(w.overlay, _paint(w.labels, frames[f0:f1]))
            assert torch.equal(w.boxes, r.boxes) and torch.equal(w.areas, r.areas)      # geometry=True: the "labels" mode's
        res = ov.result()
        assert torch.equal(torch.cat([w.overlay for w in wins]), res["pred_overlay"]) and torch.equal(res["pred_overlay"], want)
        assert torch.equal(res["pred_label_map"], runs["lab"]["pred_label_map"]) and res["pred_track_ids"] == runs["lab"]["pred_track_ids"]
        assert _same(res["pred_label_boxes"], runs["geo"]["pred_label_boxes"]) and _same(res["pred_label_areas"], runs["geo"]["pred_label_areas"])
        assert "pred_masks" not in res and "pred_boxes" not in res
        # the store is bounded by the schedule: frames no window has emitted yet, plus less than one push; empty at the end
        for h, waiting in held:
            assert waiting <= h <= waiting + max(sizes) - 1, (sizes, held)
        assert ov.frames_held == 0
    if len(PLANS[2]) > 1:                                            # pushes of five: the window (6, 12) spans the pushes 5..9 and 10..14
        assert any(h > w for h, w in _online(model, frames, PLANS[2], emit="overlay")[2])
    ov, wins, _ = _online(model, frames, [L], emit="overlay")        # keep=False: the windows only
    assert torch.equal(torch.cat([w.overlay for w in wins]), want) and all(w.boxes is None for w in wins)
    assert "pred_overlay" not in ov.result() and "pred_label_map" not in ov.result()


def test_uint8_frames_host_frames_and_a_refilled_device_buffer(model_video):
    """The frames rounded to uint8: another input, so another result than the float run's -- each run against its OWN labels.  Frames
    pushed from the host (uploaded on the copy stream) give the same bits, and so does a caller that refills ONE device buffer for
    every push (the session copies what it still has to paint)."""
    model, frames, runs = model_video
    u8 = frames.round().clamp(0, 255).to(torch.uint8)
    off = _forward(model, u8, label_output=True, overlay_output=True)
    assert torch.equal(off["pred_overlay"], _paint(off["pred_label_map"], u8))
    host = _forward(model, u8.cpu().pin_memory(), label_output=True, overlay_output=True)
    assert torch.equal(host["pred_overlay"], off["pred_overlay"]) and torch.equal(host["pred_label_map"], off["pred_label_map"])
    for sizes in PLANS[1:]:
        ov, wins, _ = _online(model, u8, sizes, emit="overlay", keep=True)
        for w in wins:
            assert torch.equal(w.overlay, _paint(w.labels, u8[w.frames[0]:w.frames[1]]))
        assert torch.equal(ov.result()["pred_overlay"], off["pred_overlay"])
        ov, wins, _ = _online(model, u8.cpu(), sizes, emit="overlay", keep=True)
        assert torch.equal(ov.result()["pred_overlay"], off["pred_overlay"])
    ov = model.online_video(height=OUT[0], width=OUT[1], emit="overlay", keep=True)
    buf = torch.empty(5, 3, 96, 160, dtype=torch.uint8, device="cuda")
    for a in range(0, L, 5):
        n = min(5, L - a)
        buf[:n].copy_(u8[a:a + n])
        ov.push(buf[:n])
        buf.fill_(0)
    ov.close()
    assert torch.equal(ov.result()["pred_overlay"], off["pred_overlay"])


def test_a_style_of_ones_own_reaches_the_kernel(model_video):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, runs = model_video
    pal = torch.randint(0, 256, (256, 3), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    st = Style(alpha=0.25, contour=2, palette=pal)
    want = _paint(runs["lab"]["pred_label_map"], frames, st)
    assert not torch.equal(want, runs["off+ov"]["pred_overlay"])
    assert torch.equal(_forward(model, frames, overlay_output=True, overlay_style=st)["pred_overlay"], want)
    assert torch.equal(_forward(model, frames, overlay_output=True, overlay_style=st, early_masks=False)["pred_overlay"], want)
    ov, wins, _ = _online(model, frames, PLANS[2], emit="overlay", style=st)
    assert torch.equal(torch.cat([w.overlay for w in wins]), want)
    assert torch.equal(runs["off+ov"]["pred_overlay"], _forward(model, frames, overlay_output=True)["pred_overlay"])    # the model's own style is back


def test_a_window_without_tracks_returns_the_frames(model_video):
    """A hand-made first window without tracks (as `_hand_windows` of the label-map tests makes it), online and on the early path: all
    background, so the overlay is the source frames -- at the frames' own size literally, at another size their nearest sample."""
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.meta_arch import ClipMerger
    from mdqe_cvpr2023_amd.render import Style
    model, frames, runs = model_video
    cfg = model.cfg
    frame_hw = (96, 160)
    geo = model.engine.geometry(*frame_hw)
    mask_hw = (geo.Hp // cfg.match_stride, geo.Wp // cfg.match_stride)
    u8 = frames[:3].round().clamp(0, 255).to(torch.uint8)
    for out_size in (frame_hw, OUT):
        with model._on_device(), torch.no_grad():
            store = merge.FrameStore()
            store.add(0, u8)
            on = ClipMerger(model, frame_hw, out_size, mask_hw, n_frames=None, online="overlay", frame_source=store, style=Style())
            m = torch.zeros(0, 3, *mask_hw, device="cuda")
            on.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(on.side):
                rec = on._online_window(torch.zeros(0, cfg.num_classes), m)
            m.record_stream(on.side)
            model.overlay_output = True
            try:
                mg = ClipMerger(model, frame_hw, out_size, mask_hw, n_frames=3, frame_source=store)
                mg.side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(mg.side):
                    mg._early_masks(m)
                mg.cls_clips.append(torch.zeros(0, cfg.num_classes))
                mg.f_off += 3
                early = mg.finish()
            finally:
                model.overlay_output = False
        rec["ready"].synchronize()
        assert not bool(rec["labels"].any())
        want = _paint(torch.zeros(3, *out_size, dtype=torch.uint8), u8)
        if out_size == frame_hw:
            assert torch.equal(want, u8.cpu().permute(0, 2, 3, 1))
        assert torch.equal(rec["overlay"], want) and torch.equal(early["pred_overlay"], want)
        assert "pred_label_map" not in early
