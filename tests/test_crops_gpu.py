"""Per-track crops on the device: ops.track_crops / ops.track_crops_yuv against the numpy restatement of their rule (tests/_crops_ref.py),
and the surfaces above them (model.crop_output, online_video(crops=...)).  The rule is integers only, so every comparison is exact.

Kernel shapes: the overlay tests' (nothing divides by anything, up- and down-sampling, a picture of three pixels) and one wide enough
for footprints of thousands of pixels; chips from one pixel (a whole-rect footprint: the wave form) to larger than the picture
(replication).  The model cases use the set-up of test_overlay_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5."""
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

import _crops_ref as REF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402

SIZES = [(61, 97, 61, 97), (60, 90, 120, 180), (96, 160, 61, 97), (5, 7, 1, 3), (70, 300, 70, 300)]      # (h0, w0, Ho, Wo)
CHIPS = [(1, 1), (8, 8), (7, 5), (24, 40), (64, 128)]
PADS = (0, 32, 256)
STEPS = ((0, 1), (1, 2), (2, 5))
F, N = 3, 4
FILL = (17, 200, 3)
SENTINEL = 0xAB


def _frames(kind, n, h0, w0, seed):
    """-> (tensor handed to the wrapper, the same frames as numpy [n, 3, h0, w0]); kind: u8 | f32 | strided."""
    g = torch.Generator().manual_seed(seed)
    if kind == "f32":                                                 # exact integers, k + 0.5 (half to even), below 0, above 255, NaN
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


def _table(Ho, Wo):
    """int32 [N * F, 5], row k * F + f: a full-picture box, a one-pixel box, a box that touches two borders, a row that is not live."""
    rows = np.zeros((N, F, 5), dtype=np.int32)
    for f in range(F):
        rows[0, f] = (Ho * Wo, 0, 0, Wo - 1, Ho - 1)
        x, y = (Wo // 2 + f) % Wo, (Ho // 3 + f) % Ho
        rows[1, f] = (1, x, y, x, y)
        if f == 1:                                                    # left and top
            rows[2, f] = (5, 0, 0, min(Wo - 1, 4), min(Ho - 1, 2))
        else:                                                         # right and bottom
            rows[2, f] = (5, Wo - 1 - min(Wo - 1, 3 + f), Ho - 1 - min(Ho - 1, 2), Wo - 1, Ho - 1)
    rows[3] = [(0, Wo, Ho, -1, -1), (7, 3, 2, 1, 5), (9, 0, 0, Wo, 0)]    # empty; xmin > xmax; xmax outside the picture
    return rows.reshape(N * F, 5)


def _labels(Ho, Wo, seed):
    return np.random.default_rng(seed).integers(0, N + 1, size=(F, Ho, Wo)).astype(np.uint8)


def _launch(fn, lab_dev, src_dev, geom_dev, size, c_off, **kw):
    """One launch into a row-strided view of a sentinel buffer, with guard chips before and after -> (chips, rects) of the call on the
    host, after checking that nothing else was written."""
    first, step = kw.get("first", 0), kw.get("step", 1)
    fc = len(range(first, F, step))
    big = torch.full((N, c_off + fc + 3) + tuple(size) + (3,), SENTINEL, dtype=torch.uint8, device="cuda")
    rbig = torch.full((N, c_off + fc + 2, 4), -7, dtype=torch.int32, device="cuda")
    out, rects = big[:, :c_off + fc + 1], rbig[:, :c_off + fc + 1]
    assert N == 1 or not out.is_contiguous()
    got = fn(lab_dev, src_dev, geom_dev, N, tuple(size), out, c_off, rects, **kw)
    assert got[0] is out and got[1] is rects
    b, r = big.cpu(), rbig.cpu()
    assert bool((b[:, :c_off] == SENTINEL).all()) and bool((b[:, c_off + fc:] == SENTINEL).all())
    assert bool((r[:, :c_off] == -7).all()) and bool((r[:, c_off + fc:] == -7).all())
    return b[:, c_off:c_off + fc], r[:, c_off:c_off + fc]


def _combos(salt):
    """(chip size, cutout, pad256, (first, step), min_area): every chip size with and without cutout; the rest rotates."""
    k = salt
    for size in CHIPS:
        for cutout in (False, True):
            yield size, cutout, PADS[k % 3], STEPS[(k // 3 + k) % 3], (0, 2)[k % 2]
            k += 1


@pytest.mark.parametrize("kind", ["u8", "f32", "strided"])
@pytest.mark.parametrize("size", SIZES)
def test_track_crops_against_the_reference(size, kind):
    from mdqe_cvpr2023_amd import ops
    h0, w0, Ho, Wo = size
    fr_dev, fr_np = _frames(kind, F, h0, w0, seed=h0 + w0)
    lab, geom = _labels(Ho, Wo, Ho * 1000 + Wo), _table(Ho, Wo)
    src = REF.expand_rgb(fr_np, Ho, Wo)
    lab_dev, geom_dev = torch.from_numpy(lab).cuda(), torch.from_numpy(geom).cuda()
    seen = set()
    for chip, cutout, pad256, (first, step), min_area in _combos(SIZES.index(size) + 2 * ["u8", "f32", "strided"].index(kind)):
        kw = dict(first=first, step=step, pad256=pad256, min_area=min_area, cutout=cutout, fill=FILL)
        want = REF.crops_fast(src, lab, geom, N, chip, **kw)
        got = _launch(ops.track_crops, lab_dev, fr_dev, geom_dev, chip, 1, **kw)
        assert np.array_equal(got[1].numpy(), want[1]), (chip, kw)
        assert np.array_equal(got[0].numpy(), want[0]), (chip, kw)
        seen.add((pad256, first))
        if chip == (7, 5):                                            # a second run into a fresh buffer: identical bytes
            again = _launch(ops.track_crops, lab_dev, fr_dev, geom_dev, chip, 1, **kw)
            assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])
    assert len(seen) >= 5
    # the buffers the wrapper allocates itself; the table as [n, F, 5]; no row; no frame taken
    out, rects = ops.track_crops(lab_dev, fr_dev, geom_dev.view(N, F, 5), N, (7, 5), pad256=32, fill=FILL)
    want = REF.crops_fast(src, lab, geom, N, (7, 5), pad256=32, fill=FILL)
    assert tuple(out.shape) == (N, F, 7, 5, 3) and np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(rects.cpu().numpy(), want[1])
    assert tuple(ops.track_crops(lab_dev, fr_dev, geom_dev[:0], 0, (7, 5))[0].shape) == (0, F, 7, 5, 3)
    keep = torch.full((N, 2, 7, 5, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    ops.track_crops(lab_dev, fr_dev, geom_dev, N, (7, 5), out=keep, c_off=2, first=F)
    assert bool((keep == SENTINEL).all())


def test_the_slow_reference_agrees_on_a_small_case():
    """The per-sample loops of the reference itself, once, against the kernel: the fast form is not the only oracle."""
    from mdqe_cvpr2023_amd import ops
    h0, w0, Ho, Wo = 9, 14, 12, 10
    fr_dev, fr_np = _frames("f32", F, h0, w0, seed=3)
    lab, geom = _labels(Ho, Wo, 5), _table(Ho, Wo)
    for chip, cutout in (((1, 1), False), ((5, 7), True), ((16, 13), True)):
        kw = dict(first=0, step=2, pad256=64, min_area=0, cutout=cutout, fill=FILL)
        want = REF.crops(REF.rgb_source(fr_np), h0, w0, lab, geom, N, chip, **kw)
        got = _launch(ops.track_crops, torch.from_numpy(lab).cuda(), fr_dev, torch.from_numpy(geom).cuda(), chip, 0, **kw)
        assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]), chip


def test_both_splits_at_their_threshold_and_a_wave_form_of_two_tiles():
    """The kernel sums a chip's footprints per thread while their bound (ceil(ch / Sh) + 1) * (ceil(cw / Sw) + 1) is at most 256 and per
    wave above: boxes of 30 x 30 and 30 x 31 into 2 x 2 chips sit on either side (16 * 16 and 16 * 17), and a 17 x 16 chip of a 300 x 400
    box is a wave form of two blocks (272 chip pixels)."""
    from mdqe_cvpr2023_amd import ops
    for (Ho, Wo), chip, boxes in (((40, 40), (2, 2), [(900, 3, 5, 32, 34), (930, 3, 5, 33, 34), (930, 3, 5, 32, 35), (0, 40, 40, -1, -1)]),
                                  ((300, 400), (17, 16), [(120000, 0, 0, 399, 299), (9, 7, 7, 9, 9), (50000, 10, 0, 399, 290), (1, 0, 0, 0, 0)])):
        g = torch.Generator().manual_seed(Ho)
        fr = torch.randint(0, 256, (F, 3, Ho, Wo), generator=g, dtype=torch.uint8)
        lab = np.random.default_rng(Wo).integers(0, N + 1, size=(F, Ho, Wo)).astype(np.uint8)
        geom = np.array([b for b in boxes for _ in range(F)], dtype=np.int32)
        for cutout in (False, True):
            kw = dict(first=0, step=2, pad256=0, min_area=0, cutout=cutout, fill=FILL)
            want = REF.crops_fast(REF.expand_rgb(fr.numpy(), Ho, Wo), lab, geom, N, chip, **kw)
            got = _launch(ops.track_crops, torch.from_numpy(lab).cuda(), fr.cuda(), torch.from_numpy(geom).cuda(), chip, 1, **kw)
            assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]), (Ho, Wo, cutout)


# ---- surfaces --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (5, 37), (16, 64), (70, 300)])
def test_track_crops_yuv_equals_the_converted_frames_and_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames, yuv_to_rgb
    ys, cs = YREF.make_content(H * 1000 + W, F, H, W, fmt)
    tight = YREF.tight_pitch(W, fmt)
    pitch, crow, lead = (tight // 16 + 1) * 16, H + 1, 2              # padded rows, a spare row, an allocation that starts 2 bytes in
    flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, 2, lead)
    host = torch.from_numpy(flat)
    dev = host.cuda()
    k = 0
    for Ho, Wo in ((H, W), (max(1, H // 2 + 1), W + 3)):              # labels at the surfaces' size, and at another
        lab, geom = _labels(Ho, Wo, H * 31 + W + Ho), _table(Ho, Wo)
        lab_dev, geom_dev = torch.from_numpy(lab).cuda(), torch.from_numpy(geom).cuda()
        for chip in ((1, 1), (7, 5), (24, 40)):
            matrix, full, order = ("bt601", "bt709")[k % 2], bool(k // 2 % 2), ("rgb", "bgr")[k % 3 % 2]
            s = YuvFrames(*YREF.plane_views(dev, F, H, W, fmt, pitch, crow, rows, lead), H, W, fmt=fmt, matrix=matrix, full_range=full, order=order)
            kw = dict(first=STEPS[k % 3][0], step=STEPS[k % 3][1], pad256=PADS[(k + 1) % 3], min_area=0, cutout=bool(k % 2), fill=FILL)
            want = REF.crops_fast(REF.expand_yuv(ys, cs, H, W, fmt, matrix, full, order, Ho, Wo), lab, geom, N, chip, **kw)
            got = _launch(ops.track_crops_yuv, lab_dev, s, geom_dev, chip, 1, **kw)
            rgb = _launch(ops.track_crops, lab_dev, yuv_to_rgb(s), geom_dev, chip, 1, **kw)
            assert torch.equal(got[0], rgb[0]) and torch.equal(got[1], rgb[1]), (Ho, Wo, chip, kw)
            assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1]), (Ho, Wo, chip, kw)
            k += 1
    assert torch.equal(dev.cpu(), host)                               # the allocation, padding included, is unchanged


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)
    return cfg, MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()


L, OUT = 17, (90, 150)
SETTINGS = {"lab": {"label_output": True}, "rle": {"rle_output": True}, "only": {"label_output": "only"}, "ov": {"overlay_output": True},
            "late": {"early_masks": False}, "geo": {"label_output": True, "geometry_output": True}}


def _specs():
    from mdqe_cvpr2023_amd.render import Crops
    return {"plain": Crops(size=(12, 10), pad=0.125), "cut3": Crops(size=(9, 16), pad=0.5, cutout=True, fill=FILL, min_area=3, every=3)}


def _forward(model, frames, size=OUT, **attrs):
    """forward() with the given attributes set, everything restored behind it."""
    names = ("label_output", "geometry_output", "rle_output", "early_masks", "overlay_output", "crop_output")
    saved = {k: getattr(model, k) for k in names}
    try:
        for k, v in attrs.items():
            setattr(model, k, v)
        return model([dict({"image": frames}, **({"height": size[0], "width": size[1]} if size else {}))])
    finally:
        for k, v in saved.items():
            setattr(model, k, v)


@pytest.fixture(scope="module")
def model_video():
    """One 17-frame video (three tracker windows of 6, 6, 5 frames) through forward() in every setting without and with crops, once.
    The class threshold is lowered so that many tracks compete for the pixels."""
    from bench import synth_video
    _, model = _model(n_frames_window_test=6, apply_cls_thres=1e-6)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    assert model.crop_output is None
    runs = {}
    for name, attrs in SETTINGS.items():
        runs[name] = _forward(model, frames, **attrs)
        runs[name + "+plain"] = _forward(model, frames, crop_output=_specs()["plain"], **attrs)
    runs["lab+cut3"] = _forward(model, frames, crop_output=_specs()["cut3"], label_output=True)
    assert model.crop_output is None
    return model, frames, runs


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    return a == b


def _want(res, frames_np, spec, size=OUT):
    """The reference's chips and rects of every output of `res`, from its label map and the input frames."""
    lm, ids = res["pred_label_map"].numpy(), res["pred_track_ids"]
    n = max(ids) + 1
    geom = np.array([REF.box_of(lm[f] == k + 1) for k in range(n) for f in range(lm.shape[0])], dtype=np.int32)
    chips, rects = REF.crops_fast(REF.expand_rgb(frames_np, *size), lm, geom, n, spec.size, first=0, step=spec.every, pad256=spec.pad256,
                                  min_area=spec.min_area, cutout=spec.cutout, fill=spec.fill)
    return chips[ids], rects[ids]


def test_model_crop_output_every_path_and_nothing_else_changes(model_video):
    model, frames, runs = model_video
    for spec_name in ("plain", "cut3"):
        spec = _specs()[spec_name]
        on = runs["lab+" + spec_name]
        chips, rects = _want(on, frames.cpu().numpy(), spec)
        lc = -(-L // spec.every)
        assert on["pred_crop_frames"] == list(range(0, L, spec.every)) and len(on["pred_crop_frames"]) == lc
        pc, pr = on["pred_crops"], on["pred_crop_rects"]
        assert pc.dtype == torch.uint8 and tuple(pc.shape) == (len(on["pred_track_ids"]), lc) + spec.size + (3,) and pc.is_pinned() and not pc.is_cuda
        assert pr.dtype == torch.int32 and tuple(pr.shape) == (len(on["pred_track_ids"]), lc, 4)
        assert np.array_equal(pr.numpy(), rects) and np.array_equal(pc.numpy(), chips)
        live = (pr[:, :, 2] >= 0)
        assert bool(live.any())                                         # (something is cut)
        assert bool((pc[~live] == torch.tensor(spec.fill, dtype=torch.uint8)).all())
    assert len(set(runs["lab+plain"]["pred_track_ids"])) > 1
    for name in SETTINGS:
        off, on = runs[name], runs[name + "+plain"]
        assert set(on) == set(off) | {"pred_crops", "pred_crop_rects", "pred_crop_frames", "pred_track_ids"}, name
        for k in off:                                                 # every other key: the bits of the run without crops
            assert _same(on[k], off[k]), (name, k)
        assert not any(k.startswith("pred_crop") for k in off)
        assert on["pred_track_ids"] == runs["lab"]["pred_track_ids"]
        for k in ("pred_crops", "pred_crop_rects", "pred_crop_frames"):       # early and late path, with and without the other outputs
            assert _same(on[k], runs["lab+plain"][k]), (name, k)
        assert ("pred_label_map" in on) == (name in ("lab", "only", "geo"))     # elsewhere the map is a device scratch


def _online(model, feed, sizes, size=OUT, **kw):
    ov = model.online_video(**dict({"height": size[0], "width": size[1]} if size else {}, **kw))
    wins, a, held = [], 0, []
    for n in sizes:
        wins += ov.push(feed[a:a + n])
        a += n
        emitted = wins[-1].frames[1] if wins else 0
        held.append((ov.frames_held, ov.received - emitted))
    wins += ov.close()
    return ov, wins, held


def _stitched(wins, ids, spec):
    """Per output the track's chips over the video, from the windows: `fill` and the dead rect before its first window."""
    fill = torch.tensor(spec.fill, dtype=torch.uint8).expand(spec.size + (3,))
    none = torch.tensor([0, 0, -1, -1], dtype=torch.int32)
    chips, rects = [], []
    for t in ids:
        chips.append(torch.cat([w.crops[t] if t < len(w.track_ids) else fill.expand((len(w.crop_frames),) + tuple(fill.shape)) for w in wins]))
        rects.append(torch.cat([w.crop_rects[t] if t < len(w.track_ids) else none.expand(len(w.crop_frames), 4) for w in wins]))
    return torch.stack(chips), torch.stack(rects)


PUSHES = [min(5, L - a) for a in range(0, L, 5)]                       # the window (6, 12) spans the pushes 5..9 and 10..14


@pytest.mark.parametrize("emit", ["masks", "rle", "labels", "overlay"])
def test_online_crops_beside_every_emit_equal_the_offline_rows(model_video, emit):
    model, frames, runs = model_video
    for spec_name in ("plain", "cut3"):
        spec, off = _specs()[spec_name], runs["lab+" + spec_name]
        ov, wins, held = _online(model, frames, PUSHES, emit=emit, keep=True, crops=spec)
        assert [w.frames for w in wins] == [(0, 6), (6, 12), (12, 17)]
        for w in wins:
            n, fc = len(w.track_ids), len(w.crop_frames)
            assert w.crop_frames == [f for f in range(*w.frames) if f % spec.every == 0]
            assert w.crops.dtype == torch.uint8 and tuple(w.crops.shape) == (n, fc) + spec.size + (3,) and (w.crops.is_pinned() or not w.crops.numel())
            assert w.crop_rects.dtype == torch.int32 and tuple(w.crop_rects.shape) == (n, fc, 4)
        chips, rects = _stitched(wins, off["pred_track_ids"], spec)
        assert torch.equal(chips, off["pred_crops"]) and torch.equal(rects, off["pred_crop_rects"])
        res = ov.result()
        assert res["pred_track_ids"] == off["pred_track_ids"] and res["pred_crop_frames"] == off["pred_crop_frames"]
        assert torch.equal(res["pred_crops"], off["pred_crops"]) and torch.equal(res["pred_crop_rects"], off["pred_crop_rects"])
        for h, waiting in held:                                       # the documented bound, whatever the emit
            assert waiting <= h <= waiting + max(PUSHES) - 1, held
        assert any(h > w for h, w in held) and ov.frames_held == 0
        # the emit's own outputs are what they are without crops
        plain_ov, plain_wins, plain_held = _online(model, frames, PUSHES, emit=emit, keep=True)
        for w, p in zip(wins, plain_wins):
            assert p.crops is None and p.crop_rects is None and p.crop_frames is None
            for k in ("masks", "labels", "overlay"):
                assert _same(getattr(w, k), getattr(p, k)), (emit, k)
            assert _same(w.rles, p.rles)
        assert _same({k: v for k, v in res.items() if not k.startswith("pred_crop")}, plain_ov.result())
        if emit != "overlay":                                         # without crops= such a session holds no frames, as ever
            assert all(h == 0 for h, _ in plain_held)


def test_online_surface_session_with_crops_equals_forward_on_surfaces_and_on_the_converted_frames(model_video):
    from bench import synth_video
    from mdqe_cvpr2023_amd.preprocess import YuvFrames, yuv_to_rgb
    model, _, _ = model_video
    h, w, crow = 96, 160, 98
    v = synth_video(0, L, seed=1, h=h, w=w, n_obj=4).numpy().astype(np.int64)
    ys, cs = v[:, 1].astype(np.uint8), np.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(L, h // 2, -1).astype(np.uint8)
    flat, rows = YREF.pack(ys, cs, "nv12", 176, crow, extra_rows=2)
    s = YuvFrames.from_surface(torch.from_numpy(flat).view(L, rows, -1).cuda(), h, w, crow, fmt="nv12")
    spec = _specs()["cut3"]
    off = _forward(model, s, size=None, crop_output=spec, overlay_output="surface", label_output=True)
    rgb = _forward(model, yuv_to_rgb(s), size=None, crop_output=spec, label_output=True)
    assert torch.equal(off["pred_label_map"], rgb["pred_label_map"]) and int(off["pred_label_map"].max()) > 0
    for k in ("pred_crops", "pred_crop_rects", "pred_crop_frames", "pred_track_ids"):
        assert _same(off[k], rgb[k]), k
    chips, rects = _want(off, yuv_to_rgb(s).cpu().numpy(), spec, size=(h, w))
    assert np.array_equal(off["pred_crops"].numpy(), chips) and np.array_equal(off["pred_crop_rects"].numpy(), rects)
    ov, wins, held = _online(model, s, PUSHES, size=None, emit="overlay", surface=True, keep=True, crops=spec)
    got = _stitched(wins, off["pred_track_ids"], spec)
    assert torch.equal(got[0], off["pred_crops"]) and torch.equal(got[1], off["pred_crop_rects"])
    assert torch.equal(ov.result()["pred_crops"], off["pred_crops"])
    for hd, waiting in held:
        assert waiting <= hd <= waiting + max(PUSHES) - 1, held
