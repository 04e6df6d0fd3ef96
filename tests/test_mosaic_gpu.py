"""The mosaic overlay on the device: mdqe_render_mosaic_u8 and mdqe_render_mosaic_yuv420sp (ops.render_mosaic, ops.render_mosaic_yuv)
against the numpy oracle with loops over cells (tests/_mosaic_ref.py), their equality with the plain painters under the table
[0, 1, 1, ...], every output alignment, and the styles above them: forward() with model.overlay_style and online_video(style=...) with
mosaic "tracks", "background" and a mosaic of classes, RGB pictures and NV12 surfaces.  Integers only: every comparison is exact.

Kernel shapes and label sets are those of test_overlay_gpu.py / test_overlay_yuv_gpu.py plus (70, 300): with cell 64 it spans several
thread blocks' tiles and has partial cells on both edges; (5, 7, 1, 3) with cell 64 is one partial cell.  Per case the cells (2, 8, 16,
64) meet the four action tables (all mosaic, background only, a random mix of 0 / 1 / 2, the plain overlay's) with contour 0..3 and
a256 in {0, 128, 256} rotating through them."""
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

import _mosaic_ref as REF  # noqa: E402
import _overlay_yuv_ref as OYREF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402
from test_overlay_gpu import L, OUT, PLANS, _forward, _frames, _label_sets, _model, _online, _palettes, _same  # noqa: E402
from test_overlay_yuv_gpu import _check_windows, _layouts, _raw, _session, _surfaces, _typed  # noqa: E402
from test_overlay_yuv_gpu import _frames as _yuv_frames  # noqa: E402
from test_overlay_yuv_gpu import _palette as _yuv_palette  # noqa: E402

SIZES = [(61, 97, 61, 97), (60, 90, 120, 180), (96, 160, 61, 97), (5, 7, 1, 3), (70, 300, 70, 300)]      # (h0, w0, Ho, Wo)
YUV_SHAPES = [(1, 1), (2, 2), (3, 5), (7, 9), (6, 36), (5, 37), (16, 64), (9, 96), (70, 300)]
CELLS = (2, 8, 16, 64)
TABLES = REF.action_tables()
A256 = (0, 128, 256)
F = 3
SENTINEL = 0xCD


def _combos():
    """(cell, table name, contour, a256): every cell with every table; contour and a256 rotate with coprime periods."""
    k = 0
    for cell in CELLS:
        for name in TABLES:
            yield cell, name, k % 4, A256[k % 3]
            k += 5


# ---- the RGB kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32", "none", "strided"])
@pytest.mark.parametrize("size", SIZES)
def test_render_mosaic_against_the_reference(size, kind):
    from mdqe_cvpr2023_amd import ops
    h0, w0, Ho, Wo = size
    sets = _label_sets(Ho, Wo, seed=Ho * 1000 + Wo)
    fr_dev, fr_np = _frames(kind, F, h0, w0, seed=h0 + w0)
    pals = _palettes()
    acts = {k: torch.from_numpy(v).cuda() for k, v in TABLES.items()}
    n = 0
    for i, (cell, name, contour, a256) in enumerate(_combos()):
        lab, pal, f_off = sets[i % 2], pals[(i // 2) % 2], 1 - i % 2          # (f_off = 1: the output starts at an odd byte for odd Ho * Wo)
        out = torch.full((f_off + F + 1, Ho, Wo, 3), 0xAB, dtype=torch.uint8, device="cuda")
        lab_dev, pal_dev = torch.from_numpy(lab).cuda(), pal.cuda()
        assert ops.render_mosaic(lab_dev, fr_dev, pal_dev, acts[name], out, f_off, a256, contour, cell) is out
        o = out.cpu()
        want = torch.from_numpy(REF.paint(lab, fr_np, pal.numpy(), TABLES[name], a256, contour, cell))
        assert torch.equal(o[f_off:f_off + F], want), (size, kind, cell, name, contour, a256)
        assert bool((o[:f_off] == 0xAB).all()) and bool((o[f_off + F:] == 0xAB).all())           # the guard frames
        if name == "plain":                                                                      # the plain painter, bit for bit
            plain = torch.full_like(out, 0xAB)
            ops.render_overlay(lab_dev, fr_dev, pal_dev, plain, f_off, a256, contour)
            assert torch.equal(plain, out), (size, kind, cell)
        n += 1
    assert n == 16


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_alignment_of_the_output_and_runs_are_identical(shift):
    from mdqe_cvpr2023_amd import ops
    pal = _palettes()[1]
    act = torch.from_numpy(TABLES["mix"]).cuda()
    for n, Ho, Wo, cell in ((2, 13, 9, 2), (2, 13, 70, 4), (1, 1, 2, 16), (1, 2, 3, 2), (1, 1, 1, 64)):
        rng = np.random.default_rng(n * Ho + Wo)
        lab = rng.integers(0, 256, size=(n, Ho, Wo)).astype(np.uint8)
        fr = torch.randint(0, 256, (n, 3, Ho, Wo), generator=torch.Generator().manual_seed(Ho), dtype=torch.uint8)
        nb = n * Ho * Wo * 3
        raw = torch.full((nb + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        out = raw[shift:shift + nb].view(n, Ho, Wo, 3)
        assert out.is_contiguous() and out.data_ptr() % 4 == shift
        args = (torch.from_numpy(lab).cuda(), fr.cuda(), pal.cuda(), act)
        ops.render_mosaic(*args, out, 0, 77, 2, cell)
        want = torch.from_numpy(REF.paint(lab, fr.numpy(), pal.numpy(), TABLES["mix"], 77, 2, cell))
        r = raw.cpu()
        assert torch.equal(r[shift:shift + nb].view(n, Ho, Wo, 3), want), (shift, n, Ho, Wo)
        assert bool((r[:shift] == 0xAB).all()) and bool((r[shift + nb:] == 0xAB).all())
        again = torch.empty_like(out)
        ops.render_mosaic(*args, again, 0, 77, 2, cell)
        assert torch.equal(again, out)                                # identical from run to run


def test_no_frames_to_paint_is_no_launch():
    from mdqe_cvpr2023_amd import ops
    pal, act = _palettes()[0].cuda(), torch.from_numpy(TABLES["all"]).cuda()
    out = torch.full((2, 4, 5, 3), 0xAB, dtype=torch.uint8, device="cuda")
    ops.render_mosaic(torch.zeros(0, 4, 5, dtype=torch.uint8, device="cuda"), None, pal, act, out, 1)
    assert bool((out == 0xAB).all())


# ---- the surface kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", YUV_SHAPES)
def test_render_mosaic_yuv_against_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops
    ys, cs = YREF.make_content(H * 1000 + W, F, H, W, fmt)
    lab = OYREF.make_labels(H * 7 + W, F, H, W)
    pal_np, pal = _yuv_palette(H + W, fmt)
    combos = list(_combos())
    want = [REF.paint_yuv(ys, cs, lab, pal_np, TABLES[name], fmt, a256, contour, cell) for cell, name, contour, a256 in combos]
    lab_dev, pal_dev = torch.from_numpy(lab).cuda(), pal.cuda()
    acts = {k: torch.from_numpy(v).cuda() for k, v in TABLES.items()}
    for pitch, crow, extra, lead in _layouts(H, W, fmt):              # tight; padded (4-byte accesses where W allows); entered one sample late
        flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
        host = torch.from_numpy(flat)
        dev = host.cuda()
        src = _yuv_frames(dev, F, H, W, fmt, pitch, crow, rows, lead)
        blank = torch.full((lead + (F + 2) * rows * pitch,), SENTINEL, dtype=torch.uint8)
        for (cell, name, contour, a256), (wy, wc) in zip(combos, want):
            expect = blank.clone()
            e = _yuv_frames(expect, F + 2, H, W, fmt, pitch, crow, rows, lead)
            e.y[1:1 + F, :, :W] = _typed(wy, fmt)
            e.uv[1:1 + F, :, :wc.shape[2]] = _typed(wc, fmt)
            out_flat = blank.cuda()
            out = _yuv_frames(out_flat, F + 2, H, W, fmt, pitch, crow, rows, lead)
            assert ops.render_mosaic_yuv(lab_dev, src, pal_dev, acts[name], out, 1, a256, contour, cell) is out      # f_off = 1, sentinels around
            assert torch.equal(out_flat.cpu(), expect), (pitch, crow, extra, lead, cell, name, contour, a256)
            if name == "plain":                                       # the plain surface painter, bit for bit
                other = blank.cuda()
                ops.render_overlay_yuv(lab_dev, src, pal_dev, _yuv_frames(other, F + 2, H, W, fmt, pitch, crow, rows, lead), 1, a256, contour)
                assert torch.equal(other, out_flat), (pitch, cell)
        assert torch.equal(dev.cpu(), host), (pitch, crow, extra, lead)   # the input allocation, padding included, is unchanged
        with pytest.raises(RuntimeError, match="render_mosaic_yuv"):  # in place is refused (MDQE_EINVAL), and nothing is written
            ops.render_mosaic_yuv(lab_dev, src, pal_dev, acts["all"], src, 0, 128, 1, 16)
        assert torch.equal(dev.cpu(), host)
    # the output the wrapper allocates itself (tight), twice: identical from run to run
    cell, name, contour, a256 = combos[6]
    wy, wc = want[6]
    got = ops.render_mosaic_yuv(lab_dev, src, pal_dev, acts[name], None, 0, a256, contour, cell)
    assert got.is_cuda and len(got) == F and got.meta() == src.meta() and np.array_equal(_raw(got.y, fmt), wy) and np.array_equal(_raw(got.uv, fmt), wc)
    again = ops.render_mosaic_yuv(lab_dev, src, pal_dev, acts[name], None, 0, a256, contour, cell)
    assert torch.equal(again.y, got.y) and torch.equal(again.uv, got.uv)
    assert len(ops.render_mosaic_yuv(lab_dev[3:], src[3:], pal_dev, acts[name])) == 0


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _paint(labels, frames, style, cls_rows=None):
    """The oracle's picture of a label map in `style`; cls_rows: [((f0, f1), class rows)] per window for a style with classes."""
    pal = style.palette_on("cpu").numpy()
    fr = frames.cpu().numpy()
    if style.classes is None:
        return torch.from_numpy(REF.paint(labels.numpy(), fr, pal, style.actions().numpy(), style.a256, style.contour, style.cell))
    return torch.cat([torch.from_numpy(REF.paint(labels[f0:f1].numpy(), fr[f0:f1], pal, style.actions(c).numpy(), style.a256, style.contour,
                                                 style.cell)) for (f0, f1), c in cls_rows])


@pytest.fixture(scope="module")
def video():
    """The fixture of test_overlay_gpu.py at the lowered class threshold (many tracks compete): 17 frames of 96 x 160, output 90 x 150,
    windows of 6, 6 and 5 frames; the run with the default style, and the windows' class rows from an online session."""
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
    return {"tracks": Style(mosaic="tracks"), "background": Style(mosaic="background", alpha=0, contour=0, cell=8),
            "classes": Style(mosaic="tracks", classes=picked, cell=4)}


def test_forward_with_a_mosaic_style_on_both_paths_and_nothing_else_changes(video):
    model, frames, base, rows = video
    styles = _styles(rows)
    lm = base[True]["pred_label_map"]
    assert int(lm.max()) > 0
    tables = [styles["classes"].actions(c)[1:int(c.shape[0]) + 1].tolist() for _, c in rows]
    print("tracks per window:", [int(c.shape[0]) for _, c in rows], "classes:", styles["classes"].classes, "tables:", tables)
    assert any(2 in t for t in tables) and any(1 in t for t in tables)           # some tracks are selected and some are not
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


def test_online_nv12_surfaces_with_a_mosaic_and_the_default_style_still_the_plain_op(video):
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
    for st in (Style(mosaic="tracks"), Style(mosaic="background", alpha=0.25, contour=2, cell=6)):
        wins, res, _ = _session(model, s, pushes, surface=True, style=st)
        assert [w.frames for w in wins] == [(0, 6), (6, 12), (12, 17)]
        pal = st.palette_yuv_on("cpu", s.fmt, s.matrix, s.full_range, s.order)
        differs = False
        for win, ref in zip(wins, plain):
            f0, f1 = win.frames
            assert torch.equal(win.labels, ref.labels)                            # the label map is the plain one
            pic = win.overlay
            assert isinstance(pic, YuvFrames) and not pic.is_cuda and len(pic) == f1 - f0 and pic.meta() == s.meta()
            want = ops.render_mosaic_yuv(win.labels, host[f0:f1], pal, st.actions(), None, 0, st.a256, st.contour, st.cell)   # the host path
            assert torch.equal(pic.y[:, :, :160], want.y) and torch.equal(pic.uv[:, :, :160], want.uv), (st.mosaic, win.frames)
            differs |= not torch.equal(pic.y, ref.overlay.y)
        assert differs
        assert torch.equal(torch.cat([w.overlay.y for w in wins]), res["pred_overlay"].y)
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])           # the caller's surfaces are not painted on
