"""The annotation pass on the device: mdqe_annotate_u8 and mdqe_annotate_yuv420sp (ops.annotate, ops.annotate_yuv) against the numpy
painter's algorithm of tests/_annotate_ref.py, bit for bit; that they work in place and leave every other byte alone; the calls that
launch nothing and the refused ones; and the style above them: forward() with model.overlay_style and online_video(style=...) with
boxes and captions, RGB pictures and NV12 surfaces.  Integers only: every comparison is exact.

Kernel shapes: 37 x 53 (less than one tile each way, nothing divides by 4) and 70 x 150 (several tiles both ways for any tile up to 64
pixels, partial tiles on both edges); surfaces of 35 x 51 (odd both ways: chroma blocks of 1 and 2 pixels) and 36 x 64."""
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

import _annotate_ref as REF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402
from test_overlay_gpu import L, OUT, PLANS, _forward, _model, _online, _same  # noqa: E402
from test_overlay_yuv_gpu import _frames as _yuv_frames  # noqa: E402
from test_overlay_yuv_gpu import _layouts, _session, _surfaces  # noqa: E402

F = 2
MIN_AREA = 3
COMBOS = [(box, scale, caps) for box in (0, 1, 3) for scale in (1, 3) for caps in (True, False)]


def _geometry(Ho, Wo):
    """int32 [n = 12, F = 2, 5] and the captions uint8 [256, 32]: the rows the rule distinguishes, frame 1 a shifted frame 0."""
    rows = [
        (0, Wo, Ho, -1, -1),                                          # 1: the empty row
        (1, 20, 30, 20, 30),                                          # 2: a 1 x 1 box
        (Ho * Wo, 0, 0, Wo - 1, Ho - 1),                              # 3: touches all four borders
        (40, 25, 0, 40, 6),                                           # 4: on the top row: the plate goes inside
        (60, 8, 14, 30, 28),                                          # 5, 6: overlapping plates and frames
        (60, 11, 17, 36, 33),
        (90, 3, Ho - 9, 12, Ho - 2),                                  # 7: a caption wider than the picture
        (50, 5, 5, Wo, 10),                                           # 8: x1 >= Wo: skipped
        (50, -3, 5, 10, -1),                                          # 9: negative entries: skipped
        (MIN_AREA - 1, 40, 20, 44, 24),                               # 10: below min_area
        (MIN_AREA, Wo - 4, 12, Wo - 1, 15),                           # 11: at min_area, its plate clamped at the right edge
        (2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 7, 7),                   # 12: garbage
    ]
    g = np.array(rows, dtype=np.int64)
    g1 = g.copy()
    g1[[1, 3, 4, 5], 1:] += np.array([2, 1, 2, 1])                    # frame 1: some boxes moved
    g1[2] = (0, Wo, Ho, -1, -1)                                       # ... and the border box gone
    geom = np.stack([g, g1], 1).astype(np.int32)
    cap = np.zeros((256, 32), dtype=np.uint8)
    texts = {1: b"EMPTY", 2: b"1", 3: b"3 ALL 100%", 4: b"TOP", 5: b"5 CAT 87%", 6: b"6 dog\x7f", 7: bytes(range(0x20, 0x40)), 8: b"OUT", 9: b"NEG",
             10: b"SMALL", 11: b"11 [\\]^_@", 12: b"GARBAGE"}
    for l, t in texts.items():
        cap[l, :len(t)] = list(t)
    return geom, cap


def _tables(seed):
    from mdqe_cvpr2023_amd import render
    pal = torch.randint(0, 256, (256, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return pal, render.ink(pal), render.default_font()


def _noise(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ---- the RGB kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ho,Wo", [(37, 53), (70, 150)])
def test_annotate_against_the_reference_in_place_with_guard_frames(Ho, Wo):
    from mdqe_cvpr2023_amd import ops
    geom, cap = _geometry(Ho, Wo)
    n = geom.shape[0]
    pal, ink, font = _tables(Ho)
    src = _noise((F + 2, Ho, Wo, 3), Ho + Wo)
    dev = [t.cuda() for t in (torch.from_numpy(geom), pal, ink, torch.from_numpy(cap), font)]
    drawn = 0
    for box, scale, caps in COMBOS:
        pic = src.cuda()
        assert ops.annotate(pic, dev[0], n, dev[1], dev[2], dev[3] if caps else None, dev[4], 1, box, scale, MIN_AREA) is pic
        want = REF.annotate(src.numpy(), geom, n, pal.numpy(), ink.numpy(), cap if caps else None, font.numpy(), 1, box, scale, MIN_AREA)
        # (the whole buffer: what the reference does not touch keeps its bytes, the frames before f_off and behind the call included)
        assert np.array_equal(pic.cpu().numpy(), want), (Ho, Wo, box, scale, caps)
        assert (box == 0 and not caps) == np.array_equal(want, src.numpy())
        drawn += int((want != src.numpy()).any(-1).sum())
        again = src.cuda()
        ops.annotate(again, dev[0].view(-1, 5), n, dev[1], dev[2], dev[3] if caps else None, dev[4], 1, box, scale, MIN_AREA)
        assert torch.equal(again, pic)                                # identical from run to run, the table flat or [n, F, 5]
    assert drawn > 1000


def test_255_live_labels_of_small_boxes():
    from mdqe_cvpr2023_amd import ops
    Ho, Wo, n = 70, 150, 255
    rng = np.random.default_rng(255)
    geom = np.zeros((n, F, 5), dtype=np.int32)
    for k in range(n):
        for f in range(F):
            x0, y0 = 8 * (k % 17) + 3 * f + int(rng.integers(0, 4)), 4 * (k // 17) + 5 * f + int(rng.integers(0, 3))
            geom[k, f] = (9, x0, y0, x0 + int(rng.integers(0, 7)), y0 + int(rng.integers(0, 5)))
    assert all(REF.is_live(geom[k, f], Ho, Wo, 0) for k in range(n) for f in range(F))
    cap = np.zeros((256, 4), dtype=np.uint8)                          # (another cap_len than render.captions')
    for l in range(1, 256):
        t = str(l - 1).encode()
        cap[l, :len(t)] = list(t)
    pal, ink, font = _tables(7)
    src = _noise((F, Ho, Wo, 3), 9)
    for box, scale, caps in ((1, 1, True), (2, 1, False), (0, 2, True)):
        pic = src.cuda()
        ops.annotate(pic, torch.from_numpy(geom).cuda(), n, pal.cuda(), ink.cuda(), torch.from_numpy(cap).cuda() if caps else None, font.cuda(),
                     0, box, scale, 0)
        want = REF.annotate(src.numpy(), geom, n, pal.numpy(), ink.numpy(), cap if caps else None, font.numpy(), 0, box, scale, 0)
        assert np.array_equal(pic.cpu().numpy(), want), (box, scale, caps)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_byte_alignment_of_the_picture(shift):
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 37, 53
    geom, cap = _geometry(Ho, Wo)
    pal, ink, font = _tables(3)
    src = _noise((F, Ho, Wo, 3), 11)
    nb = src.numel()
    raw = torch.full((nb + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    pic = raw[shift:shift + nb].view(F, Ho, Wo, 3)
    pic.copy_(src)
    assert pic.is_contiguous() and pic.data_ptr() % 4 == shift
    ops.annotate(pic, torch.from_numpy(geom).cuda(), geom.shape[0], pal.cuda(), ink.cuda(), torch.from_numpy(cap).cuda(), font.cuda(), 0, 3, 1, MIN_AREA)
    want = REF.annotate(src.numpy(), geom, geom.shape[0], pal.numpy(), ink.numpy(), cap, font.numpy(), 0, 3, 1, MIN_AREA)
    r = raw.cpu()
    assert np.array_equal(r[shift:shift + nb].view(F, Ho, Wo, 3).numpy(), want), shift
    assert bool((r[:shift] == 0xAB).all()) and bool((r[shift + nb:] == 0xAB).all())


# ---- the surface kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(35, 51), (36, 64)])
def test_annotate_yuv_against_the_reference_padding_and_low_bits_kept(H, W, fmt):
    from mdqe_cvpr2023_amd import ops, render
    geom, cap = _geometry(H, W)
    n = geom.shape[0]
    pal, ink, font = _tables(H + W)
    pal_y, ink_y = (render.palette_yuv(t, fmt, "bt601", True, "rgb") for t in (pal, ink))
    ys, cs = YREF.make_content(H * 1000 + W, F + 1, H, W, fmt)        # (P010: noise in the low 6 bits of every word)
    dev = [t.cuda() for t in (torch.from_numpy(geom), pal_y, ink_y, torch.from_numpy(cap), font)]
    want = [REF.annotate_yuv(ys, cs, fmt, H, W, geom, n, pal_y.numpy().astype(np.int64), ink_y.numpy().astype(np.int64), cap if caps else None,
                             font.numpy(), 1, box, scale, MIN_AREA) for box, scale, caps in COMBOS]
    for pitch, crow, extra, lead in _layouts(H, W, fmt):              # tight; padded; padded and entered one sample late
        flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
        for (box, scale, caps), (wy, wc) in zip(COMBOS, want):
            buf = torch.from_numpy(flat).cuda()
            s = _yuv_frames(buf, F + 1, H, W, fmt, pitch, crow, rows, lead)
            assert ops.annotate_yuv(s, dev[0], n, dev[1], dev[2], dev[3] if caps else None, dev[4], 1, box, scale, MIN_AREA) is s
            # the whole allocation: the padding, surface 0 in front of f_off, and for P010 all 16 bits of every word the rule leaves alone
            assert np.array_equal(buf.cpu().numpy(), YREF.pack(wy, wc, fmt, pitch, crow, extra, lead)[0]), (pitch, crow, lead, box, scale, caps)
    for (box, scale, caps), (wy, wc) in zip(COMBOS, want):
        assert (box == 0 and not caps) == (np.array_equal(wy, ys) and np.array_equal(wc, cs))
        assert np.array_equal(wy[0], ys[0]) and np.array_equal(wc[0], cs[0])
        if fmt == "p010" and (box or caps):                           # written words are value << 6, the others kept their noise
            assert bool(((wy != ys) & ((wy & 63) != 0)).sum() == 0) and bool(((wy == ys) & ((wy & 63) != 0)).any())


# ---- calls that launch nothing, calls that are refused ----------------------------------------------------------------------------------
def _entries():
    from mdqe_cvpr2023_amd import _lib
    h = _lib.load_library()

    def rgb(F=1, Ho=8, Wo=8, f_off=0, n=1, cap_len=32, box=1, scale=1, min_area=0):
        return h.mdqe_annotate_u8(None, F, Ho, Wo, f_off, None, n, None, None, None, cap_len, None, box, scale, min_area, None)

    def yuv(F=1, H=32, W=64, f_off=0, n=1, cap_len=32, box=1, scale=1, min_area=0, fmt=0, yp=64, ys=64 * 48, cp=64, cs=64 * 48):
        return h.mdqe_annotate_yuv420sp(None, yp, ys, None, cp, cs, F, H, W, fmt, f_off, None, n, None, None, None, cap_len, None, box, scale,
                                        min_area, None)
    return rgb, yuv


def test_calls_that_launch_nothing_return_ok():
    from mdqe_cvpr2023_amd import ops
    rgb, yuv = _entries()
    for call in (rgb, yuv):                                           # (null pointers: a launch would have been refused as MDQE_ENULL first)
        assert call(F=0) == 0 and call(n=0) == 0 and call(box=0, cap_len=0) == 0
        assert call() == 3 and call(box=0) == 3 and call(cap_len=0) == 3
    geom, cap = _geometry(8, 9)
    pal, ink, font = _tables(1)
    src = _noise((2, 8, 9, 3), 2)
    pic = src.cuda()
    g = torch.from_numpy(geom).cuda()
    ops.annotate(pic, g[:, :0].contiguous(), 12, pal.cuda(), ink.cuda(), torch.from_numpy(cap).cuda(), font.cuda(), 1, 2, 1)     # F == 0
    ops.annotate(pic, g[:0], 0, pal.cuda(), ink.cuda(), torch.from_numpy(cap).cuda(), font.cuda(), 0, 2, 1)                       # n == 0
    ops.annotate(pic, g, 12, pal.cuda(), ink.cuda(), None, font.cuda(), 0, 0, 1)                                                  # nothing to draw
    assert torch.equal(pic.cpu(), src)


def test_every_refused_argument_returns_einval_with_null_pointers():
    rgb, yuv = _entries()
    EINVAL = 1
    bad = ({"box": -1}, {"box": 5}, {"scale": 0}, {"scale": 5}, {"n": -1}, {"n": 256}, {"cap_len": -1}, {"cap_len": 65}, {"min_area": -1},
           {"F": -1}, {"f_off": -1})
    for call in (rgb, yuv):
        for kw in bad:
            assert call(**kw) == EINVAL, (call.__name__, kw)
            if "F" not in kw and "n" not in kw:
                assert call(**dict(kw, F=0)) == EINVAL and call(**dict(kw, n=0)) == EINVAL, (call.__name__, kw)   # ... whatever else says "no launch"
    assert rgb(Ho=0) == EINVAL and rgb(Wo=-4) == EINVAL and yuv(H=0) == EINVAL and yuv(W=0) == EINVAL
    assert rgb(F=2, Ho=32768, Wo=32768) == EINVAL and rgb(F=1, Ho=46341, Wo=46341) == EINVAL and rgb(F=3, Ho=26755, Wo=26755) == EINVAL
    assert yuv(F=2 ** 15, H=256, W=256, ys=256 * 400, cs=256 * 400, yp=256, cp=256) == EINVAL                       # F*H*W = 2^31
    # the surface conditions of mdqe_render_overlay_yuv420sp
    for kw in ({"fmt": 2}, {"fmt": -1}, {"yp": 63}, {"cp": 63}, {"ys": -1}, {"cs": -1}, {"fmt": 1, "yp": 127}, {"fmt": 1, "yp": 129, "cp": 128},
               {"fmt": 1, "yp": 128, "cp": 128, "ys": 128 * 48 + 1}, {"F": 2, "ys": 64 * 32 - 1}, {"F": 2, "cs": 64 * 16 - 1}):
        assert yuv(**kw) == EINVAL, kw
        assert yuv(**dict(kw, n=0)) == EINVAL, kw
    assert yuv(fmt=1, yp=128, cp=128, ys=128 * 48, cs=128 * 48, n=0) == 0 and yuv(F=2, ys=64 * 32, cs=64 * 16, n=0) == 0


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _style():
    from mdqe_cvpr2023_amd.render import Style
    return Style(box=2, caption="id+class+score")


@pytest.fixture(scope="module")
def video():
    """The fixture of test_mosaic_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5 frames, many tracks."""
    from bench import synth_video
    _, model = _model(n_frames_window_test=6, apply_cls_thres=1e-6)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    return model, frames


def _pieces(pushes, windows):
    """How many (window, push) pairs share frames: the pieces a session paints, one annotate launch each."""
    ends = np.cumsum(pushes)
    return sum(1 for f0, f1 in windows for a, b in zip(ends - np.array(pushes), ends) if a < f1 and b > f0)


class _Spy:
    """Wraps ops.final_label_map, ops.annotate and ops.annotate_yuv: the geometry tables the first returned (one per window, in window
    order), and how often the other two ran."""

    def __init__(self, monkeypatch):
        from mdqe_cvpr2023_amd import ops
        self.geoms, self.calls = [], 0
        real = {k: getattr(ops, k) for k in ("final_label_map", "annotate", "annotate_yuv")}

        def label_map(*a, **kw):
            out, geom = real["final_label_map"](*a, **kw)
            self.geoms.append(None if geom is None else geom.clone())
            return out, geom

        def counted(name):
            def fn(*a, **kw):
                self.calls += 1
                return real[name](*a, **kw)
            return fn
        monkeypatch.setattr(ops, "final_label_map", label_map)
        monkeypatch.setattr(ops, "annotate", counted("annotate"))
        monkeypatch.setattr(ops, "annotate_yuv", counted("annotate_yuv"))

    def take(self):
        g, c = self.geoms, self.calls
        self.geoms, self.calls = [], 0
        return g, c


def _annotated(plain, geoms, rows, style):
    """The plain style's picture (uint8 [L, Ho, Wo, 3], host) passed through ops.annotate window by window, and the same through the
    reference: geoms from ops.final_label_map(..., geom=True), the text from render.captions."""
    from mdqe_cvpr2023_amd import ops, render
    pal, ink, font = style.palette_on("cpu"), style.ink_on("cpu"), style.font_on("cpu")
    parts = []
    assert len(geoms) == len(rows)
    for g, ((f0, f1), c) in zip(geoms, rows):
        n = int(c.shape[0])
        assert g is not None and tuple(g.shape) == (n * (f1 - f0), 5) and 0 < n <= 255
        text = render.captions(style, c, n)
        pic = plain[f0:f1].cuda()
        ops.annotate(pic, g, n, pal.cuda(), ink.cuda(), text.cuda(), font.cuda(), 0, style.box, style.text_scale, style.min_area)
        ref = REF.annotate(plain[f0:f1].numpy(), g.cpu().numpy(), n, pal.numpy(), ink.numpy(), text.numpy(), font.numpy(), 0, style.box,
                           style.text_scale, style.min_area)
        assert np.array_equal(pic.cpu().numpy(), ref), (f0, f1)
        parts.append(pic.cpu())
    return torch.cat(parts)


def test_forward_and_online_with_boxes_and_captions_and_nothing_else_changes(video, monkeypatch):
    model, frames = video
    st, spy = _style(), _Spy(monkeypatch)
    _, lab_wins, _ = _online(model, frames, [L], emit="labels")
    rows = [(w.frames, w.cls_probs) for w in lab_wins]
    assert [f for f, _ in rows] == [(0, 6), (6, 12), (12, 17)]
    spy.take()
    want = None
    for early in (True, False):
        base = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early)
        geoms, calls = spy.take()
        assert calls == 0 and all(g is None for g in geoms)           # Style(): no annotate launch, no geometry asked for
        got = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=st)
        geoms, calls = spy.take()
        assert calls == 3                                             # one launch per window (each window one piece)
        if want is None:
            want = _annotated(base["pred_overlay"], geoms, rows, st)
            spy.take()
            changed = int((want != base["pred_overlay"]).any(-1).sum())
            print("tracks per window:", [int(c.shape[0]) for _, c in rows], "annotated pixels:", changed)
            assert changed > 500
        assert set(got) == set(base), early                           # the geometry table the pass asked for does not come out
        assert torch.equal(got["pred_overlay"], want), early
        for k in base:                                                # every other key: the bits of the default style's run
            if k != "pred_overlay":
                assert _same(got[k], base[k]), (early, k)
    # with geometry_output the labels' geometry comes out as ever, and is the plain run's
    geo = _forward(model, frames, overlay_output=True, label_output=True, geometry_output=True, overlay_style=st)
    ref = _forward(model, frames, overlay_output=True, label_output=True, geometry_output=True)
    assert torch.equal(geo["pred_overlay"], want) and set(geo) == set(ref) and _same(geo["pred_label_boxes"], ref["pred_label_boxes"])
    spy.take()
    # online: the windows concatenate to the offline picture, whatever the pushes (a window of several pushes: one launch per piece)
    for sizes in PLANS:
        ov, wins, _ = _online(model, frames, sizes, emit="overlay", style=st)
        _, calls = spy.take()
        assert calls == _pieces(sizes, [f for f, _ in rows]), (sizes, calls)
        assert [w.frames for w in wins] == [f for f, _ in rows] and all(w.boxes is None for w in wins)
        assert torch.equal(torch.cat([w.overlay for w in wins]), want), sizes
    ov, wins, _ = _online(model, frames, PLANS[2], emit="overlay")   # Style(): the painter alone
    assert spy.take()[1] == 0
    assert not torch.equal(torch.cat([w.overlay for w in wins]), want)
    # the mosaic painter under the same pass
    from mdqe_cvpr2023_amd.render import Style
    mo = Style(mosaic="tracks", box=1, caption="id", text_scale=2, min_area=20)
    plain = _forward(model, frames, overlay_output=True, overlay_style=Style(mosaic="tracks"))
    spy.take()
    got = _forward(model, frames, overlay_output=True, overlay_style=mo)
    geoms, calls = spy.take()
    assert calls == 3 and torch.equal(got["pred_overlay"], _annotated(plain["pred_overlay"], geoms, rows, mo))


def test_nv12_surfaces_with_boxes_and_captions_online_and_offline(video, monkeypatch):
    from mdqe_cvpr2023_amd import ops, render
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    model, _ = video
    st, spy = _style(), _Spy(monkeypatch)
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda", matrix="bt601", full_range=True, order="bgr")
    before = s.y.clone(), s.uv.clone()
    pushes = (5, 3, 7, 2)
    plain, _, _ = _session(model, s, pushes, surface=True)
    assert spy.take()[1] == 0
    wins, res, _ = _session(model, s, pushes, surface=True, style=st)
    geoms, calls = spy.take()
    assert [w.frames for w in wins] == [(0, 6), (6, 12), (12, 17)] and calls == _pieces(pushes, [w.frames for w in wins]) == 6
    pal, ink = (f("cuda", s.fmt, s.matrix, s.full_range, s.order) for f in (st.palette_yuv_on, st.ink_yuv_on))
    changed = 0
    for win, ref, g in zip(wins, plain, geoms):
        f0, f1 = win.frames
        n = int(win.cls_probs.shape[0])
        assert torch.equal(win.labels, ref.labels) and torch.equal(win.cls_probs, ref.cls_probs) and tuple(g.shape) == (n * (f1 - f0), 5)
        want = ref.overlay.to("cuda")
        ops.annotate_yuv(want, g, n, pal, ink, render.captions(st, win.cls_probs, n).cuda(), st.font_on("cuda"), 0, st.box, st.text_scale, st.min_area)
        pic = win.overlay
        assert isinstance(pic, YuvFrames) and not pic.is_cuda and pic.meta() == s.meta()
        assert torch.equal(pic.y, want.y.cpu()) and torch.equal(pic.uv, want.uv.cpu()), win.frames
        changed += int((pic.y != ref.overlay.y).sum())
    assert changed > 500
    assert torch.equal(torch.cat([w.overlay.y for w in wins]), res["pred_overlay"].y)
    assert torch.equal(torch.cat([w.overlay.uv for w in wins]), res["pred_overlay"].uv)
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])           # the caller's surfaces are not drawn on
    saved = model.overlay_style
    model.overlay_output, model.overlay_style = "surface", st
    try:
        off = model([{"image": s}])
    finally:
        model.overlay_output, model.overlay_style = False, saved
    assert torch.equal(off["pred_overlay"].y, res["pred_overlay"].y) and torch.equal(off["pred_overlay"].uv, res["pred_overlay"].uv)
