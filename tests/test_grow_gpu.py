"""The redaction margin on the device: mdqe_grow_labels_u8 (ops.grow_labels, csrc/grow.hip) against the numpy rule (tests/_grow_ref.py) --
every shape, radius and table, sparse maps whose tiles are skipped or flagged through their halo alone, ties across a tile boundary,
every output alignment -- the painters fed the grown map, and the styles above them: forward() with model.overlay_style and
online_video(style=...) with Style(grow=...), RGB pictures and NV12 surfaces, under trails, boxes and captions.  Integers only: every
comparison is exact.

Kernel shapes: (1, 3) and (3, 200) are shorter than the radius one way, (3, 200), (61, 97), (70, 300) and (120, 180) several 16 x 64
tiles; at (70, 300) a halo of 32 reaches past a neighbouring tile."""
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

import _blur_ref as BREF  # noqa: E402
import _grow_ref as REF  # noqa: E402
import _mosaic_ref as MREF  # noqa: E402
import _overlay_ref as OREF  # noqa: E402
import _overlay_yuv_ref as OYREF  # noqa: E402
import _paths_ref as PREF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402
from test_annotate_gpu import _annotated, _Spy  # noqa: E402
from test_overlay_gpu import L, OUT, PLANS, _forward, _label_sets, _model, _online, _palettes, _same  # noqa: E402
from test_overlay_yuv_gpu import _layouts, _raw, _session, _surfaces  # noqa: E402
from test_overlay_yuv_gpu import _frames as _yuv_frames  # noqa: E402
from test_overlay_yuv_gpu import _palette as _yuv_palette  # noqa: E402

SHAPES = [(1, 3), (3, 200), (61, 97), (70, 300), (120, 180)]
RADII = (0, 1, 2, 5, 17, 32)
TABLES = REF.tables()
F = 3
SENTINEL = 0xCD


def _run(lab, table, radius, shift=1):
    """One launch into a sentinel-filled buffer, `out` sliced out of it at byte `shift`; the guard bytes are checked.  -> out on the host."""
    from mdqe_cvpr2023_amd import ops
    n = lab.size
    raw = torch.full((n + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = raw[shift:shift + n].view(lab.shape)
    assert out.is_contiguous() and out.data_ptr() % 4 == shift % 4
    assert ops.grow_labels(torch.from_numpy(lab).cuda(), torch.from_numpy(table).cuda(), radius, out) is out
    r = raw.cpu()
    assert bool((r[:shift] == SENTINEL).all()) and bool((r[shift + n:] == SENTINEL).all())
    return r[shift:shift + n].view(lab.shape).numpy()


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_grow_labels_against_the_reference(shape, radius):
    Ho, Wo = shape
    sets = _label_sets(Ho, Wo, seed=Ho * 1000 + Wo)
    for k, lab in enumerate(sets):
        for name, table in TABLES.items():
            got = _run(lab, table, radius, shift=1 + 2 * k)            # (an odd byte offset: 1 and 3)
            want = REF.grow(lab, table, radius)
            assert np.array_equal(got, want), (shape, radius, k, name, int((got != want).sum()))
            if radius == 0 or name == "none":
                assert np.array_equal(got, lab)                       # a copy
    assert np.array_equal(REF.grow(sets[0], TABLES["all"], radius), REF.grow(sets[0], TABLES["all+0"], radius))      # entry 0 is ignored


def _sparse(case):
    """Maps of 70 x 300 (tiles of 16 x 64: corners at rows 16, 32, ... and columns 64, 128, ...); label 9 grows, label 4 does not."""
    lab = np.zeros((2, 70, 300), dtype=np.uint8)
    if case == "four tiles":                                          # a 5 x 5 blob straddles the corner of four tiles
        lab[0, 30:35, 126:131] = 9
        lab[1, 16:21, 64:69] = 9                                      # ... or starts exactly at one
    elif case == "picture corners":
        for f in range(2):
            lab[f, :5, :5] = 9; lab[f, :5, -5:] = 9; lab[f, -5:, :5] = 9; lab[f, -5:, -5:] = 9
    else:                                                             # "empty neighbour": the blob's tile neighbours empty tiles at distance <= radius
        lab[0, 20:28, 120:127] = 9                                    # (columns 128.. and rows 32.. belong to tiles without a label of their own)
        lab[1, 47, 191] = 9                                           # one pixel in a tile's last corner: it grows into three empty tiles
    lab[:, 40:50, 200:230] = 4                                        # a region that does not grow, in tiles that are skipped: copied through
    return lab


@pytest.mark.parametrize("case", ["four tiles", "picture corners", "empty neighbour"])
def test_sparse_maps_flag_a_tile_through_its_halo_and_copy_the_skipped_ones(case):
    lab = _sparse(case)
    table = np.zeros(256, dtype=np.uint8)
    table[9] = 1
    for radius in (1, 5, 17, 32):
        got = _run(lab, table, radius)
        want = REF.grow(lab, table, radius)
        assert np.array_equal(got, want), (case, radius)
        assert int((want == 9).sum()) > int((lab == 9).sum())         # it grew ...
        assert np.array_equal(want[want != 9], lab[want != 9]) and (want == 4).any()      # ... and where 9 did not reach, the map is copied
    if case == "empty neighbour":                                     # (radius 32) the pixel at (47, 191) reaches rows 48.. and columns 192..: other tiles
        assert got[1, 48, 191] == 9 and got[1, 47, 192] == 9 and got[1, 60, 200] == 9
        assert (got[1, 48:, 192:] == 9).any() and (got[0, 32:, 128:] == 9).any()
    both = np.ones(256, dtype=np.uint8)                               # with label 4 growing too: the two regions meet
    assert np.array_equal(_run(lab, both, 32), REF.grow(lab, both, 32))


def test_ties_across_a_tile_boundary_take_the_smaller_label():
    table = np.zeros(256, dtype=np.uint8)
    table[[3, 7]] = 1
    # (position of 7, position of 3, the pixel at equal distance), around the tile corner (16, 64): a horizontal, a vertical, a mixed tie
    cases = (((16, 61), (16, 67), (16, 64)), ((13, 64), (19, 64), (16, 64)), ((15, 68), (18, 67), (15, 63)), ((18, 67), (15, 68), (15, 63)))
    for p7, p3, at in cases:
        for a, b in ((7, 3), (3, 7)):
            lab = np.zeros((1, 40, 140), dtype=np.uint8)
            lab[0][p7], lab[0][p3] = a, b
            got = _run(lab, table, 5)
            assert np.array_equal(got, REF.grow(lab, table, 5)) and np.array_equal(got, REF.grow_pixelwise(lab, table, 5))
            assert got[0][at] == 3, (p7, p3, a, b)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_alignment_of_the_output_and_runs_are_identical(shift):
    from mdqe_cvpr2023_amd import ops
    for n, Ho, Wo, radius in ((2, 13, 9, 2), (2, 13, 70, 5), (1, 1, 2, 17), (1, 2, 3, 1), (1, 1, 1, 32), (1, 20, 132, 8), (2, 17, 64, 3)):
        rng = np.random.default_rng(n * Ho + Wo)
        lab = np.where(rng.random((n, Ho, Wo)) < 0.1, rng.integers(1, 256, size=(n, Ho, Wo)), 0).astype(np.uint8)
        table = TABLES["subset"]
        got = _run(lab, table, radius, shift)
        assert np.array_equal(got, REF.grow(lab, table, radius)), (shift, n, Ho, Wo)
        lab_dev, tab_dev = torch.from_numpy(lab).cuda(), torch.from_numpy(table).cuda()
        a, b = ops.grow_labels(lab_dev, tab_dev, radius), ops.grow_labels(lab_dev, tab_dev, radius)
        assert a is not b and torch.equal(a, b) and np.array_equal(a.cpu().numpy(), got)     # identical from run to run


def test_copies_empty_maps_and_refusals():
    from mdqe_cvpr2023_amd import ops
    lab = torch.from_numpy(_label_sets(61, 97, seed=4)[0]).cuda()
    every = torch.from_numpy(TABLES["all"]).cuda()
    assert torch.equal(ops.grow_labels(lab, every, 0), lab)
    assert torch.equal(ops.grow_labels(lab, torch.zeros(256, dtype=torch.uint8, device="cuda"), 32), lab)
    empty = torch.zeros(0, 61, 97, dtype=torch.uint8, device="cuda")
    assert tuple(ops.grow_labels(empty, every, 8).shape) == (0, 61, 97)
    assert tuple(ops.grow_labels(torch.zeros(2, 0, 5, dtype=torch.uint8, device="cuda"), every, 8).shape) == (2, 0, 5)
    # not in place: out may not meet labels in any byte
    before = lab.clone()
    flat = torch.zeros(2 * lab.numel(), dtype=torch.uint8, device="cuda")
    src = flat[:lab.numel()].view(lab.shape).copy_(lab)
    for out in (src, flat[lab.numel() - 1:2 * lab.numel() - 1].view(lab.shape)):
        with pytest.raises(RuntimeError, match="grow_labels"):
            ops.grow_labels(src, every, 4, out)
    assert torch.equal(src, before)
    with pytest.raises(RuntimeError, match="grow_labels: grow must be a CUDA tensor"):
        ops.grow_labels(lab, every.cpu(), 4)


# ---- the painters take the grown map ---------------------------------------------------------------------------------------------------
def _taps(radius):
    from mdqe_cvpr2023_amd.render import blur_taps
    t = blur_taps(radius)
    return t.cuda(), t.view(torch.int16).numpy().view(np.uint16)


def test_the_painters_fed_the_grown_map_equal_their_references_fed_the_references_map():
    from mdqe_cvpr2023_amd import ops
    Ho, Wo, radius = 37, 150, 6
    lab = np.zeros((2, Ho, Wo), dtype=np.uint8)
    lab[0, 10:18, 60:70], lab[0, 20:30, 100:140], lab[1, 0:6, 0:9], lab[1, 30:37, 64:80] = 9, 4, 9, 200
    table = np.zeros(256, dtype=np.uint8)
    table[[9, 200]] = 1
    want_map = REF.grow(lab, table, radius)
    grown = ops.grow_labels(torch.from_numpy(lab).cuda(), torch.from_numpy(table).cuda(), radius)
    assert np.array_equal(grown.cpu().numpy(), want_map) and not np.array_equal(want_map, lab)
    act = {"mosaic": np.ones(256, dtype=np.uint8), "blur": np.ones(256, dtype=np.uint8)}
    act["mosaic"][[0, 9, 200]] = 0, 2, 2
    act["blur"][[0, 9, 200]] = 0, 3, 3
    taps_dev, taps_np = _taps(5)
    taps_c_dev, taps_c_np = _taps(3)
    # RGB
    fr = torch.randint(0, 256, (2, 3, Ho, Wo), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    pal = _palettes()[0]
    args = (grown, fr.cuda(), pal.cuda())

    def blank():
        return torch.full((2, Ho, Wo, 3), 0xAB, dtype=torch.uint8, device="cuda")
    got = ops.render_overlay(*args, blank(), 0, 128, 1)
    assert np.array_equal(got.cpu().numpy(), OREF.paint(want_map, fr.numpy(), pal.numpy(), 128, 1))
    got = ops.render_mosaic(*args, torch.from_numpy(act["mosaic"]).cuda(), blank(), 0, 128, 1, 8)
    assert np.array_equal(got.cpu().numpy(), MREF.paint(want_map, fr.numpy(), pal.numpy(), act["mosaic"], 128, 1, 8))
    got = ops.render_blur(*args, torch.from_numpy(act["blur"]).cuda(), taps_dev, blank(), 0, 128, 1)
    want = BREF.paint(want_map, fr.numpy(), pal.numpy(), act["blur"], 128, 1, taps_np)
    assert np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want, BREF.paint(lab, fr.numpy(), pal.numpy(), act["blur"], 128, 1, taps_np))      # (the margin shows)
    # NV12
    fmt = "nv12"
    ys, cs = YREF.make_content(Ho * 1000 + Wo, 2, Ho, Wo, fmt)
    pal_np, pal_t = _yuv_palette(Ho + Wo, fmt)
    pitch, crow, extra, lead = _layouts(Ho, Wo, fmt)[0]
    flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
    src = _yuv_frames(torch.from_numpy(flat).cuda(), 2, Ho, Wo, fmt, pitch, crow, rows, lead)
    yargs = (grown, src, pal_t.cuda())
    for got, (wy, wc) in (
            (ops.render_overlay_yuv(*yargs, None, 0, 128, 1), OYREF.paint(ys, cs, want_map, pal_np, fmt, 128, 1)),
            (ops.render_mosaic_yuv(*yargs, torch.from_numpy(act["mosaic"]).cuda(), None, 0, 128, 1, 8),
             MREF.paint_yuv(ys, cs, want_map, pal_np, act["mosaic"], fmt, 128, 1, 8)),
            (ops.render_blur_yuv(*yargs, torch.from_numpy(act["blur"]).cuda(), taps_dev, taps_c_dev, None, 0, 128, 1),
             BREF.paint_yuv(ys, cs, want_map, pal_np, act["blur"], fmt, 128, 1, taps_np, taps_c_np))):
        assert np.array_equal(_raw(got.y, fmt), wy) and np.array_equal(_raw(got.uv, fmt), wc)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class _GrowSpy:
    """Counts the ops.grow_labels calls."""

    def __init__(self, monkeypatch):
        from mdqe_cvpr2023_amd import ops
        self.calls = 0
        real = ops.grow_labels

        def fn(*a, **kw):
            self.calls += 1
            return real(*a, **kw)
        monkeypatch.setattr(ops, "grow_labels", fn)

    def take(self):
        c, self.calls = self.calls, 0
        return c


@pytest.fixture(scope="module")
def video():
    """The fixture of test_mosaic_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5 frames, many tracks; the runs with
    the default style, and the windows' class rows from an online session."""
    from bench import synth_video
    _, model = _model(n_frames_window_test=6, apply_cls_thres=1e-6)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    base = {early: _forward(model, frames, overlay_output=True, label_output=True, early_masks=early) for early in (True, False)}
    _, wins, _ = _online(model, frames, [L], emit="labels")
    rows = [(w.frames, w.cls_probs) for w in wins]
    assert [f for f, _ in rows] == [(0, 6), (6, 12), (12, 17)]
    return model, frames, base, rows


def _styles(rows):
    from mdqe_cvpr2023_amd.render import Style
    last = rows[-1][1]
    picked = sorted(set(last.argmax(1)[::2].tolist()))                # classes of this run's own rows: every second track of the last window
    return {"blur": Style(blur="tracks", grow=4), "classes": Style(mosaic="tracks", classes=picked, grow=3), "plain": Style(grow=2)}


def _painted(lm, frames, style, rows):
    """Label map -> ops.grow_labels with style.grows(the window's class rows) -> the style's painter, window by window, on the device.
    -> (the picture, the grown map), on the host."""
    from mdqe_cvpr2023_amd import ops
    pics, maps = [], []
    pal = style.palette_on("cuda")
    for (f0, f1), c in rows:
        lab = lm[f0:f1].cuda().contiguous()
        grown = ops.grow_labels(lab, style.grows(c).cuda(), style.grow) if style.grow > 0 else lab
        out = torch.empty((f1 - f0,) + OUT + (3,), dtype=torch.uint8, device="cuda")
        fr = frames[f0:f1]
        if style.blur is not None:
            ops.render_blur(grown, fr, pal, style.actions(c).cuda(), style.taps_on("cuda"), out, 0, style.a256, style.contour)
        elif style.mosaic is not None:
            ops.render_mosaic(grown, fr, pal, style.actions(c).cuda(), out, 0, style.a256, style.contour, style.cell)
        else:
            ops.render_overlay(grown, fr, pal, out, 0, style.a256, style.contour)
        pics.append(out.cpu())
        maps.append(grown.cpu())
    return torch.cat(pics), torch.cat(maps)


def test_forward_with_a_margin_on_both_paths_and_nothing_else_changes(video, monkeypatch):
    model, frames, base, rows = video
    spy = _GrowSpy(monkeypatch)
    lm = base[True]["pred_label_map"]
    assert int(lm.max()) > 0
    for name, st in _styles(rows).items():
        flat = dataclasses.replace(st, grow=0)
        spy.take()
        want, grown = _painted(lm, frames, st, rows)
        assert spy.take() == 3
        assert np.array_equal(grown.numpy(), np.concatenate([REF.grow(lm[f0:f1].numpy(), st.grows(c).numpy(), st.grow) for (f0, f1), c in rows]))
        print(name, "grown pixels:", int((grown != lm).sum()))
        assert int((grown != lm).sum()) > 100 and not torch.equal(want, _painted(lm, frames, flat, rows)[0])
        for early in (True, False):
            ref = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=flat)
            assert spy.take() == 0                                    # grow == 0: no launch
            got = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=st)
            assert spy.take() == 3                                    # one per window with tracks
            assert set(got) == set(ref) == set(base[early]), (name, early)
            pic = got["pred_overlay"]
            assert pic.dtype == torch.uint8 and tuple(pic.shape) == (L,) + OUT + (3,) and not pic.is_cuda
            assert torch.equal(got["pred_label_map"], lm) and torch.equal(pic, want), (name, early)
            for k in ref:                                             # every other key: the bits of the grow = 0 run
                if k != "pred_overlay":
                    assert _same(got[k], ref[k]) and _same(got[k], base[early][k]), (name, early, k)
    again = _forward(model, frames, overlay_output=True, label_output=True)      # the model's own style is back
    assert torch.equal(again["pred_overlay"], base[True]["pred_overlay"])


def test_online_windows_concatenate_to_the_offline_picture(video, monkeypatch):
    model, frames, base, rows = video
    spy = _GrowSpy(monkeypatch)
    lm = base[True]["pred_label_map"]
    for name, st in _styles(rows).items():
        want = _painted(lm, frames, st, rows)[0]
        for sizes in PLANS:
            spy.take()
            ov, wins, _ = _online(model, frames, sizes, emit="overlay", style=st)
            assert spy.take() == 3, (name, sizes)                     # one per window, however many pieces it is painted in
            assert [w.frames for w in wins] == [f for f, _ in rows]
            for w, (_, c) in zip(wins, rows):
                assert torch.equal(w.labels, lm[w.frames[0]:w.frames[1]]) and torch.equal(w.cls_probs, c)      # the un-grown map
            assert torch.equal(torch.cat([w.overlay for w in wins]), want), (name, sizes)
            assert "pred_overlay" not in ov.result()


def test_trails_boxes_and_captions_are_those_of_the_map_as_made(video, monkeypatch):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    n = int(lm.max())
    st = Style(blur="tracks", blur_radius=6, grow=4, trail=5, trail_width=2, box=2, caption="id+class+score")
    pts = PREF.centroids(lm.numpy(), n, 0)[1]                         # (of the un-grown map)
    painted = _painted(lm, frames, st, rows)[0]
    trailed = torch.from_numpy(PREF.trails_rgb(painted.numpy(), pts, n, st.palette_on("cpu").numpy(), L, 0, 0, st.trail, st.trail_width))
    spy = _Spy(monkeypatch)
    got = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=st)
    geoms, calls = spy.take()
    assert calls == 3
    want = _annotated(trailed, geoms, rows, st)                       # (the geometry tables are ops.final_label_map's: un-grown)
    assert torch.equal(got["pred_overlay"], want) and torch.equal(got["pred_label_map"], lm)
    assert not torch.equal(trailed, painted) and not torch.equal(want, trailed)
    plain = _forward(model, frames, overlay_output=True, label_output=True, geometry_output=True,
                     overlay_style=Style(blur="tracks", blur_radius=6, trail=5, trail_width=2, box=2, caption="id+class+score"))
    geo = _forward(model, frames, overlay_output=True, label_output=True, geometry_output=True, overlay_style=st)
    assert set(geo) == set(plain) and torch.equal(geo["pred_overlay"], want) and not torch.equal(plain["pred_overlay"], want)
    for k in plain:                                                   # boxes, areas and the rest: the bits of the grow = 0 run
        if k != "pred_overlay":
            assert _same(geo[k], plain[k]), k


def test_online_nv12_surfaces_with_a_margin(video, monkeypatch):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style
    model = video[0]
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda", matrix="bt601", full_range=True, order="bgr")
    before = s.y.clone(), s.uv.clone()
    pushes = (5, 3, 7, 2)
    spy = _GrowSpy(monkeypatch)
    for flat in (Style(blur="tracks"), Style(mosaic="background", alpha=0.25, contour=2, cell=6), Style()):
        st = dataclasses.replace(flat, grow=5)
        ref, _, _ = _session(model, s, pushes, surface=True, style=flat)
        assert spy.take() == 0
        wins, res, _ = _session(model, s, pushes, surface=True, style=st)
        assert spy.take() == 3 and [w.frames for w in wins] == [(0, 6), (6, 12), (12, 17)]
        pal = st.palette_yuv_on("cuda", s.fmt, s.matrix, s.full_range, s.order)
        differs = False
        for win, r in zip(wins, ref):
            f0, f1 = win.frames
            assert torch.equal(win.labels, r.labels)                  # the label map is the un-grown one
            pic = win.overlay
            assert isinstance(pic, YuvFrames) and not pic.is_cuda and len(pic) == f1 - f0 and pic.meta() == s.meta()
            grown = ops.grow_labels(win.labels.cuda(), st.grows(win.cls_probs).cuda(), st.grow)
            assert np.array_equal(grown.cpu().numpy(), REF.grow(win.labels.numpy(), st.grows(win.cls_probs).numpy(), st.grow))
            if st.blur is not None:
                want = ops.render_blur_yuv(grown, s[f0:f1], pal, st.actions().cuda(), st.taps_on("cuda"), st.taps_c_on("cuda"), None, 0,
                                           st.a256, st.contour)
            elif st.mosaic is not None:
                want = ops.render_mosaic_yuv(grown, s[f0:f1], pal, st.actions().cuda(), None, 0, st.a256, st.contour, st.cell)
            else:
                want = ops.render_overlay_yuv(grown, s[f0:f1], pal, None, 0, st.a256, st.contour)
            assert torch.equal(pic.y[:, :, :160], want.y.cpu()) and torch.equal(pic.uv[:, :, :160], want.uv.cpu()), (flat, win.frames)
            differs |= not torch.equal(pic.y, r.overlay.y)
        assert differs
        assert torch.equal(torch.cat([w.overlay.y for w in wins]), res["pred_overlay"].y)
        spy.take()
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])           # the caller's surfaces are not painted on


def test_a_window_without_tracks_returns_the_frames(video, monkeypatch):
    """A hand-made first window without tracks (as test_overlay_gpu.py makes it), online and on the early path, in a style with a margin:
    nothing grows, no grow launch is made, and the overlay is the source frames."""
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.meta_arch import ClipMerger
    from mdqe_cvpr2023_amd.render import Style
    model, frames = video[0], video[1]
    spy = _GrowSpy(monkeypatch)
    cfg = model.cfg
    frame_hw = (96, 160)
    geo = model.engine.geometry(*frame_hw)
    mask_hw = (geo.Hp // cfg.match_stride, geo.Wp // cfg.match_stride)
    u8 = frames[:3].round().clamp(0, 255).to(torch.uint8)
    st = Style(blur="tracks", grow=4)
    saved = model.overlay_output, model.overlay_style
    with model._on_device(), torch.no_grad():
        store = merge.FrameStore()
        store.add(0, u8)
        on = ClipMerger(model, frame_hw, frame_hw, mask_hw, n_frames=None, online="overlay", frame_source=store, style=st)
        m = torch.zeros(0, 3, *mask_hw, device="cuda")
        on.side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(on.side):
            rec = on._online_window(torch.zeros(0, cfg.num_classes), m)
        m.record_stream(on.side)
        model.overlay_output, model.overlay_style = True, st
        try:
            mg = ClipMerger(model, frame_hw, frame_hw, mask_hw, n_frames=3, frame_source=store)
            mg.side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(mg.side):
                mg._early_masks(m)
            mg.cls_clips.append(torch.zeros(0, cfg.num_classes))
            mg.f_off += 3
            early = mg.finish()
        finally:
            model.overlay_output, model.overlay_style = saved
    rec["ready"].synchronize()
    assert spy.take() == 0 and not bool(rec["labels"].any())
    want = u8.cpu().permute(0, 2, 3, 1)
    assert torch.equal(rec["overlay"], want) and torch.equal(early["pred_overlay"], want)
