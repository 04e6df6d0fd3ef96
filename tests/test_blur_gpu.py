"""The blur overlay on the device: mdqe_render_blur_u8 and mdqe_render_blur_yuv420sp (ops.render_blur, ops.render_blur_yuv) against the
numpy oracle (tests/_blur_ref.py), their equality with the plain painters under the table [0, 1, 1, ...], sparse label maps (most tiles
skip the filter, a flagged tile's halo reads pixels of unflagged ones), every output alignment, and the styles above them: forward()
with model.overlay_style and online_video(style=...) with blur "tracks", "background" and a blur of classes, RGB pictures and NV12
surfaces, and a blur under trails, boxes and captions.  Integers only: every comparison is exact.

Kernel shapes are those of test_mosaic_gpu.py plus (3, 200): shorter than the radius one way, several 16 x 64 tiles the other; at
(70, 300) a halo of 32 reaches past a neighbouring tile.  Per case the radii (0, 1, 2, 5, 17, 32) meet the four action tables (all
blur, background only, a random mix of 0 / 1 / 3, the plain overlay's) with contour 0..3 and a256 in {0, 128, 256} rotating through
them."""
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

import _blur_ref as REF  # noqa: E402
import _overlay_yuv_ref as OYREF  # noqa: E402
import _paths_ref as PREF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402
from test_annotate_gpu import _annotated, _Spy  # noqa: E402
from test_mosaic_gpu import YUV_SHAPES as MOSAIC_YUV_SHAPES  # noqa: E402
from test_overlay_gpu import L, OUT, PLANS, _forward, _frames, _label_sets, _model, _online, _palettes, _same  # noqa: E402
from test_overlay_yuv_gpu import _check_windows, _layouts, _raw, _session, _surfaces, _typed  # noqa: E402
from test_overlay_yuv_gpu import _frames as _yuv_frames  # noqa: E402
from test_overlay_yuv_gpu import _palette as _yuv_palette  # noqa: E402

SIZES = [(61, 97, 61, 97), (60, 90, 120, 180), (96, 160, 61, 97), (5, 7, 1, 3), (70, 300, 70, 300), (3, 200, 3, 200)]   # (h0, w0, Ho, Wo)
YUV_SHAPES = MOSAIC_YUV_SHAPES + [(3, 200)]
RADII = (0, 1, 2, 5, 17, 32)
YUV_RADII = (0, 1, 5, 32)
TABLES = REF.action_tables()
A256 = (0, 128, 256)
F = 3
SENTINEL = 0xCD


def _taps(radius):
    """(the device table, the same as numpy)."""
    from mdqe_cvpr2023_amd.render import blur_taps
    t = blur_taps(radius)
    return t.cuda(), t.view(torch.int16).numpy().view(np.uint16)


def _combos(radii):
    """(radius, table name, contour, a256): every radius with every table; contour and a256 rotate with coprime periods."""
    k = 0
    for radius in radii:
        for name in TABLES:
            yield radius, name, k % 4, A256[k % 3]
            k += 5


# ---- the RGB kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32", "none", "strided"])
@pytest.mark.parametrize("size", SIZES)
def test_render_blur_against_the_reference(size, kind):
    from mdqe_cvpr2023_amd import ops
    h0, w0, Ho, Wo = size
    sets = _label_sets(Ho, Wo, seed=Ho * 1000 + Wo)
    fr_dev, fr_np = _frames(kind, F, h0, w0, seed=h0 + w0)
    pals = _palettes()
    acts = {k: torch.from_numpy(v).cuda() for k, v in TABLES.items()}
    n = 0
    for i, (radius, name, contour, a256) in enumerate(_combos(RADII)):
        lab, pal, f_off = sets[i % 2], pals[(i // 2) % 2], 1 - i % 2          # (f_off = 1: the output starts at an odd byte for odd Ho * Wo)
        taps_dev, taps_np = _taps(radius)
        out = torch.full((f_off + F + 1, Ho, Wo, 3), 0xAB, dtype=torch.uint8, device="cuda")
        lab_dev, pal_dev = torch.from_numpy(lab).cuda(), pal.cuda()
        assert ops.render_blur(lab_dev, fr_dev, pal_dev, acts[name], taps_dev, out, f_off, a256, contour) is out
        o = out.cpu()
        want = torch.from_numpy(REF.paint(lab, fr_np, pal.numpy(), TABLES[name], a256, contour, taps_np))
        assert torch.equal(o[f_off:f_off + F], want), (size, kind, radius, name, contour, a256)
        assert bool((o[:f_off] == 0xAB).all()) and bool((o[f_off + F:] == 0xAB).all())           # the guard frames
        if name == "plain":                                                                      # the plain painter, bit for bit
            plain = torch.full_like(out, 0xAB)
            ops.render_overlay(lab_dev, fr_dev, pal_dev, plain, f_off, a256, contour)
            assert torch.equal(plain, out), (size, kind, radius)
        n += 1
    assert n == 24


@pytest.mark.parametrize("where", ["tile corner", "picture corners"])
def test_sparse_label_maps_blur_a_few_tiles_from_their_neighbours_pixels(where):
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 70, 300
    lab = np.zeros((2, Ho, Wo), dtype=np.uint8)
    if where == "tile corner":                                        # the 5 x 5 blob straddles the corner of four 16 x 64 tiles
        lab[0, 30:35, 126:131] = 9
        lab[1, 16:21, 64:69] = 9                                      # ... or starts exactly at one
    else:
        for f in range(2):
            lab[f, :5, :5] = 9; lab[f, :5, -5:] = 9; lab[f, -5:, :5] = 9; lab[f, -5:, -5:] = 9
    lab[:, 40:50, 200:230] = 4                                        # a tinted region in tiles that skip the filter
    act = np.zeros(256, dtype=np.uint8)
    act[9], act[4] = 3, 1
    fr = torch.randint(0, 256, (2, 3, Ho, Wo), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    pal = _palettes()[0]
    for radius in (1, 17, 32):
        taps_dev, taps_np = _taps(radius)
        out = torch.full((2, Ho, Wo, 3), 0xAB, dtype=torch.uint8, device="cuda")
        ops.render_blur(torch.from_numpy(lab).cuda(), fr.cuda(), pal.cuda(), torch.from_numpy(act).cuda(), taps_dev, out, 0, 128, 1)
        want = REF.paint(lab, fr.numpy(), pal.numpy(), act, 128, 1, taps_np)
        assert np.array_equal(out.cpu().numpy(), want), (where, radius)
        kept = np.moveaxis(fr.numpy(), 1, -1)
        assert np.array_equal(want[lab == 0], kept[lab == 0]) and not np.array_equal(want[lab == 9], kept[lab == 9])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_alignment_of_the_output_and_runs_are_identical(shift):
    from mdqe_cvpr2023_amd import ops
    pal = _palettes()[1]
    act = torch.from_numpy(TABLES["mix"]).cuda()
    for n, Ho, Wo, radius in ((2, 13, 9, 2), (2, 13, 70, 5), (1, 1, 2, 17), (1, 2, 3, 1), (1, 1, 1, 32), (1, 20, 132, 8)):
        rng = np.random.default_rng(n * Ho + Wo)
        lab = rng.integers(0, 256, size=(n, Ho, Wo)).astype(np.uint8)
        fr = torch.randint(0, 256, (n, 3, Ho, Wo), generator=torch.Generator().manual_seed(Ho), dtype=torch.uint8)
        taps_dev, taps_np = _taps(radius)
        nb = n * Ho * Wo * 3
        raw = torch.full((nb + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        out = raw[shift:shift + nb].view(n, Ho, Wo, 3)
        assert out.is_contiguous() and out.data_ptr() % 4 == shift
        args = (torch.from_numpy(lab).cuda(), fr.cuda(), pal.cuda(), act, taps_dev)
        ops.render_blur(*args, out, 0, 77, 2)
        want = torch.from_numpy(REF.paint(lab, fr.numpy(), pal.numpy(), TABLES["mix"], 77, 2, taps_np))
        r = raw.cpu()
        assert torch.equal(r[shift:shift + nb].view(n, Ho, Wo, 3), want), (shift, n, Ho, Wo)
        assert bool((r[:shift] == 0xAB).all()) and bool((r[shift + nb:] == 0xAB).all())
        again = torch.empty_like(out)
        ops.render_blur(*args, again, 0, 77, 2)
        assert torch.equal(again, out)                                # identical from run to run


def test_no_frames_to_paint_is_no_launch():
    from mdqe_cvpr2023_amd import ops
    pal, act = _palettes()[0].cuda(), torch.from_numpy(TABLES["all"]).cuda()
    out = torch.full((2, 4, 5, 3), 0xAB, dtype=torch.uint8, device="cuda")
    ops.render_blur(torch.zeros(0, 4, 5, dtype=torch.uint8, device="cuda"), None, pal, act, _taps(8)[0], out, 1)
    assert bool((out == 0xAB).all())


# ---- the surface kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", YUV_SHAPES)
def test_render_blur_yuv_against_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops
    ys, cs = YREF.make_content(H * 1000 + W, F, H, W, fmt)
    lab = OYREF.make_labels(H * 7 + W, F, H, W)
    pal_np, pal = _yuv_palette(H + W, fmt)
    combos = list(_combos(YUV_RADII))
    tables = {r: (_taps(r), _taps((r + 1) // 2)) for r in YUV_RADII}
    want = [REF.paint_yuv(ys, cs, lab, pal_np, TABLES[name], fmt, a256, contour, tables[r][0][1], tables[r][1][1]) for r, name, contour, a256 in combos]
    lab_dev, pal_dev = torch.from_numpy(lab).cuda(), pal.cuda()
    acts = {k: torch.from_numpy(v).cuda() for k, v in TABLES.items()}
    low = 0
    for pitch, crow, extra, lead in _layouts(H, W, fmt):              # tight; padded; entered one sample late
        flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
        host = torch.from_numpy(flat)
        dev = host.cuda()
        src = _yuv_frames(dev, F, H, W, fmt, pitch, crow, rows, lead)
        blank = torch.full((lead + (F + 2) * rows * pitch,), SENTINEL, dtype=torch.uint8)
        for (r, name, contour, a256), (wy, wc) in zip(combos, want):
            (taps, _), (taps_c, _) = tables[r]
            expect = blank.clone()
            e = _yuv_frames(expect, F + 2, H, W, fmt, pitch, crow, rows, lead)
            e.y[1:1 + F, :, :W] = _typed(wy, fmt)
            e.uv[1:1 + F, :, :wc.shape[2]] = _typed(wc, fmt)
            out_flat = blank.cuda()
            out = _yuv_frames(out_flat, F + 2, H, W, fmt, pitch, crow, rows, lead)
            assert ops.render_blur_yuv(lab_dev, src, pal_dev, acts[name], taps, taps_c, out, 1, a256, contour) is out   # f_off = 1, sentinels around
            assert torch.equal(out_flat.cpu(), expect), (pitch, crow, extra, lead, r, name, contour, a256)
            if name == "plain":                                       # the plain surface painter, bit for bit
                other = blank.cuda()
                ops.render_overlay_yuv(lab_dev, src, pal_dev, _yuv_frames(other, F + 2, H, W, fmt, pitch, crow, rows, lead), 1, a256, contour)
                assert torch.equal(other, out_flat), (pitch, r)
            if fmt == "p010" and name == "mix":                       # kept words keep all 16 bits (make_content sets low bits)
                keep = ~np.isin(TABLES[name][lab], (1, 3))
                assert np.array_equal(wy[keep], ys[keep])
                low += int((wy[keep] & 0x3F != 0).sum())
        assert torch.equal(dev.cpu(), host), (pitch, crow, extra, lead)   # the input allocation, padding included, is unchanged
        (taps, _), (taps_c, _) = tables[5]
        with pytest.raises(RuntimeError, match="render_blur_yuv"):    # in place is refused (MDQE_EINVAL), and nothing is written
            ops.render_blur_yuv(lab_dev, src, pal_dev, acts["all"], taps, taps_c, src, 0, 128, 1)
        if F > 1:
            with pytest.raises(RuntimeError, match="render_blur_yuv"):    # ... and so is an output that meets the input one surface on
                ops.render_blur_yuv(lab_dev[:F - 1], src[:F - 1], pal_dev, acts["all"], taps, taps_c, src, 1, 128, 1)
        assert torch.equal(dev.cpu(), host)
    if fmt == "p010" and H * W > 30:
        assert low > 0
    # the output the wrapper allocates itself (tight), twice: identical from run to run
    r, name, contour, a256 = combos[6]
    (taps, _), (taps_c, _) = tables[r]
    wy, wc = want[6]
    got = ops.render_blur_yuv(lab_dev, src, pal_dev, acts[name], taps, taps_c, None, 0, a256, contour)
    assert got.is_cuda and len(got) == F and got.meta() == src.meta() and np.array_equal(_raw(got.y, fmt), wy) and np.array_equal(_raw(got.uv, fmt), wc)
    again = ops.render_blur_yuv(lab_dev, src, pal_dev, acts[name], taps, taps_c, None, 0, a256, contour)
    assert torch.equal(again.y, got.y) and torch.equal(again.uv, got.uv)
    assert len(ops.render_blur_yuv(lab_dev[3:], src[3:], pal_dev, acts[name], taps, taps_c)) == 0


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _paint(labels, frames, style, cls_rows=None):
    """The oracle's picture of a label map in `style`; cls_rows: [((f0, f1), class rows)] per window for a style with classes."""
    pal = style.palette_on("cpu").numpy()
    fr = frames.cpu().numpy()
    taps = _taps(style.blur_radius)[1]
    if style.classes is None:
        return torch.from_numpy(REF.paint(labels.numpy(), fr, pal, style.actions().numpy(), style.a256, style.contour, taps))
    return torch.cat([torch.from_numpy(REF.paint(labels[f0:f1].numpy(), fr[f0:f1], pal, style.actions(c).numpy(), style.a256, style.contour,
                                                 taps)) for (f0, f1), c in cls_rows])


@pytest.fixture(scope="module")
def video():
    """The fixture of test_mosaic_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5 frames, many tracks; the run with
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
    # classes of this run's own rows: the first maximum of every second track of the last window
    last = rows[-1][1]
    picked = sorted(set(last.argmax(1)[::2].tolist()))
    return {"tracks": Style(blur="tracks"), "background": Style(blur="background", alpha=0, contour=0),
            "classes": Style(blur="tracks", classes=picked, blur_radius=3)}


def test_forward_with_a_blur_style_on_both_paths_and_nothing_else_changes(video):
    model, frames, base, rows = video
    styles = _styles(rows)
    lm = base[True]["pred_label_map"]
    assert int(lm.max()) > 0
    tables = [styles["classes"].actions(c)[1:int(c.shape[0]) + 1].tolist() for _, c in rows]
    print("tracks per window:", [int(c.shape[0]) for _, c in rows], "classes:", styles["classes"].classes, "tables:", tables)
    assert any(3 in t for t in tables) and any(1 in t for t in tables)           # some tracks are selected and some are not
    for name, st in styles.items():
        want = _paint(lm, frames, st, rows)
        assert not torch.equal(want, base[True]["pred_overlay"]), name            # another picture than the default style's
        for early in (True, False):
            got = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=st)
            assert set(got) == set(base[early]), (name, early)
            pic = got["pred_overlay"]
            assert pic.dtype == torch.uint8 and tuple(pic.shape) == (L,) + OUT + (3,) and not pic.is_cuda
            assert torch.equal(got["pred_label_map"], lm) and torch.equal(pic, want), (name, early)
            for k in base[early]:                                                 # every other key: the bits of the default style's run
                if k != "pred_overlay":
                    assert _same(got[k], base[early][k]), (name, early, k)
    again = _forward(model, frames, overlay_output=True, label_output=True)      # the model's own style is back
    assert torch.equal(again["pred_overlay"], base[True]["pred_overlay"])


def test_online_windows_concatenate_to_the_offline_picture(video):
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    for name, st in _styles(rows).items():
        want = _paint(lm, frames, st, rows)
        for sizes in PLANS:
            ov, wins, _ = _online(model, frames, sizes, emit="overlay", style=st)
            assert [w.frames for w in wins] == [f for f, _ in rows]
            for w, (_, c) in zip(wins, rows):
                assert torch.equal(w.labels, lm[w.frames[0]:w.frames[1]]) and torch.equal(w.cls_probs, c)
            assert torch.equal(torch.cat([w.overlay for w in wins]), want), (name, sizes)
            assert "pred_overlay" not in ov.result()                              # (keep=False: no new keys anywhere)


def test_a_blur_lies_under_trails_boxes_and_captions(video, monkeypatch):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    n = int(lm.max())
    st = Style(blur="tracks", blur_radius=6, trail=5, trail_width=2, box=2, caption="id+class+score")
    pts = PREF.centroids(lm.numpy(), n, 0)[1]
    blurred = _paint(lm, frames, st, rows)
    trailed = torch.from_numpy(PREF.trails_rgb(blurred.numpy(), pts, n, st.palette_on("cpu").numpy(), L, 0, 0, st.trail, st.trail_width))
    spy = _Spy(monkeypatch)
    got = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=st)
    geoms, calls = spy.take()
    assert calls == 3
    want = _annotated(trailed, geoms, rows, st)                       # (the annotation reference after the trail reference, window by window)
    assert torch.equal(got["pred_overlay"], want) and torch.equal(got["pred_label_map"], lm)
    assert not torch.equal(trailed, blurred) and not torch.equal(want, trailed)
    for k in base[True]:
        if k != "pred_overlay":
            assert _same(got[k], base[True][k]), k


def test_online_nv12_surfaces_with_a_blur_and_the_default_style_still_the_plain_op(video):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style
    model = video[0]
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda", matrix="bt601", full_range=True, order="bgr")
    before = s.y.clone(), s.uv.clone()
    host = s.to("cpu")
    pushes = (5, 3, 7, 2)
    plain, _, _ = _session(model, s, pushes, surface=True)                        # a session with Style(): the existing op, as ever
    assert _check_windows(model, plain, s, Style()) > 0
    for st in (Style(blur="tracks"), Style(blur="background", alpha=0.25, contour=2, blur_radius=5)):
        wins, res, _ = _session(model, s, pushes, surface=True, style=st)
        assert [w.frames for w in wins] == [(0, 6), (6, 12), (12, 17)]
        pal = st.palette_yuv_on("cpu", s.fmt, s.matrix, s.full_range, s.order)
        taps_np, taps_c_np = _taps(st.blur_radius)[1], _taps((st.blur_radius + 1) // 2)[1]
        differs = False
        for win, ref in zip(wins, plain):
            f0, f1 = win.frames
            assert torch.equal(win.labels, ref.labels)                            # the label map is the plain one
            pic = win.overlay
            assert isinstance(pic, YuvFrames) and not pic.is_cuda and len(pic) == f1 - f0 and pic.meta() == s.meta()
            wy, wc = REF.paint_yuv(host.y[f0:f1, :, :160].numpy(), host.uv[f0:f1, :, :160].numpy(), win.labels.numpy(),
                                   pal.view(torch.int16).numpy().astype(np.int64), st.actions().numpy(), "nv12", st.a256, st.contour,
                                   taps_np, taps_c_np)
            assert np.array_equal(pic.y[:, :, :160].numpy(), wy) and np.array_equal(pic.uv[:, :, :160].numpy(), wc), (st.blur, win.frames)
            want = ops.render_blur_yuv(win.labels, host[f0:f1], pal, st.actions(), st.taps_on("cpu"), st.taps_c_on("cpu"), None, 0,
                                       st.a256, st.contour)                       # ... and the host path says the same
            assert torch.equal(pic.y[:, :, :160], want.y) and torch.equal(pic.uv[:, :, :160], want.uv)
            differs |= not torch.equal(pic.y, ref.overlay.y)
        assert differs
        assert torch.equal(torch.cat([w.overlay.y for w in wins]), res["pred_overlay"].y)
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])           # the caller's surfaces are not painted on
