"""The blur overlay, the host side: the numpy oracle (tests/_blur_ref.py) against the plain overlay's oracles and against its own rule as
loops per pixel; render.blur_taps; render.Style's new fields and its action table; the host path of ops.render_blur_yuv against the
oracle; the wrappers' refusals; the two ABI entries; and the launches merge.overlay_frames makes, with the ops painters replaced by
recorders.  Integers only: every comparison is exact.  No GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _blur_ref as REF  # noqa: E402
import _overlay_ref as OREF  # noqa: E402
import _overlay_yuv_ref as OYREF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402

TABLES = REF.action_tables()


def _taps(radius):
    from mdqe_cvpr2023_amd.render import blur_taps
    return blur_taps(radius).view(torch.int16).numpy().view(np.uint16)


def _rgb_case(seed, F, Ho, Wo, h0, w0):
    rng = np.random.default_rng(seed)
    lab = OYREF.make_labels(seed, F, Ho, Wo)
    fr = rng.integers(0, 256, size=(F, 3, h0, w0)).astype(np.uint8)
    pal = rng.integers(0, 256, size=(256, 3)).astype(np.uint8)
    return lab, fr, pal


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [0, 2, 32])
def test_reference_under_the_plain_table_is_the_plain_overlay(radius):
    taps = _taps(radius)
    lab, fr, pal = _rgb_case(3, 2, 13, 21, 9, 30)
    for contour in range(4):
        for a256 in (0, 77, 256):
            assert np.array_equal(REF.paint(lab, fr, pal, TABLES["plain"], a256, contour, taps), OREF.paint(lab, fr, pal, a256, contour))
    for fmt in ("nv12", "p010"):
        for H, W in ((7, 9), (6, 36)):
            ys, cs = YREF.make_content(H + W, 2, H, W, fmt)
            lab = OYREF.make_labels(H * 7 + W, 2, H, W)
            pal = np.random.default_rng(1).integers(0, 256 if fmt == "nv12" else 1024, size=(256, 3))
            for contour, a256 in ((0, 128), (1, 0), (2, 255), (3, 256)):
                wy, wc = OYREF.paint(ys, cs, lab, pal, fmt, a256, contour)
                gy, gc = REF.paint_yuv(ys, cs, lab, pal, TABLES["plain"], fmt, a256, contour, taps, _taps((radius + 1) // 2))
                assert np.array_equal(gy, wy) and np.array_equal(gc, wc), (fmt, H, W, contour, a256)


def test_the_loop_reference_equals_the_vectorised_one():
    lab, fr, pal = _rgb_case(5, 2, 9, 14, 9, 14)
    for radius in (1, 5, 17):                                        # 17: more than either side of the picture
        taps = _taps(radius)
        a = REF.paint(lab, fr, pal, TABLES["mix"], 128, 1, taps)
        b = REF.paint(lab, fr, pal, TABLES["mix"], 128, 1, taps, blur_fn=REF.blur_loops)
        assert np.array_equal(a, b), radius
    assert not np.array_equal(a, OREF.paint(lab, fr, pal, 128, 1))
    ys, cs = YREF.make_content(11, 2, 7, 9, "p010")
    lab = OYREF.make_labels(4, 2, 7, 9)
    pal = np.random.default_rng(2).integers(0, 1024, size=(256, 3))
    a = REF.paint_yuv(ys, cs, lab, pal, TABLES["mix"], "p010", 77, 2, _taps(5), _taps(3))
    b = REF.paint_yuv(ys, cs, lab, pal, TABLES["mix"], "p010", 77, 2, _taps(5), _taps(3), blur_fn=REF.blur_loops)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_constant_picture_and_radius_0_are_identities_and_other_actions_keep():
    lab, fr, pal = _rgb_case(7, 2, 11, 19, 11, 19)
    assert np.array_equal(REF.paint(lab, fr, pal, TABLES["all"], 128, 1, _taps(0)), np.moveaxis(fr, 1, -1))
    for radius in (1, 8, 32):
        for v in (0, 1, 127, 255, 1023):                              # (1023: a P010 plane)
            assert np.array_equal(REF.blur(np.full((1, 11, 19), v, dtype=np.int64), _taps(radius)), np.full((1, 11, 19), v))
    const = np.broadcast_to(np.array([3, 200, 255], dtype=np.uint8)[None, :, None, None], (2, 3, 11, 19)).copy()
    assert np.array_equal(REF.paint(lab, const, pal, TABLES["all"], 128, 1, _taps(8)), np.moveaxis(const, 1, -1))
    odd = np.where(TABLES["mix"] == 0, np.uint8(2), TABLES["mix"])    # 2 (the mosaic's value) and the like act as 0
    odd[::7] = np.where(odd[::7] == 2, np.uint8(200), odd[::7])
    assert np.array_equal(REF.paint(lab, fr, pal, odd, 128, 1, _taps(3)), REF.paint(lab, fr, pal, TABLES["mix"], 128, 1, _taps(3)))


# ---- render.blur_taps ----------------------------------------------------------------------------------------------------------------
def test_blur_taps_properties_and_pinned_values():
    from mdqe_cvpr2023_amd.render import blur_taps
    assert blur_taps(0).tolist() == [4096] and blur_taps(0).dtype == torch.uint16 and not blur_taps(3).is_cuda
    assert blur_taps(1).tolist() == [3224, 436]
    assert blur_taps(2).tolist() == [1650, 1000, 223]
    assert blur_taps(5).tolist()[:3] == [670, 620, 488]
    assert blur_taps(32).tolist()[-2:] == [16, 14]
    for radius in range(1, 33):
        w = blur_taps(radius).tolist()
        assert len(w) == radius + 1 and w[0] + 2 * sum(w[1:]) == 4096 and min(w) >= 1, radius
        assert all(w[d] >= w[d + 1] for d in range(1, radius)), radius
        g = [math.exp(-2.0 * d * d / (radius * radius)) for d in range(radius + 1)]
        total = g[0] + 2 * sum(g[1:])
        for d in range(1, radius + 1):                                # no product near a rounding tie: the table is the host's libm's to any ulp
            x = 4096 * g[d] / total
            assert abs(x - math.floor(x) - 0.5) > 1.5e-3 and w[d] == math.floor(x + 0.5), (radius, d, x)
    for bad in (-1, 33, 8.0, "8", True, None):
        with pytest.raises(ValueError, match="radius"):
            blur_taps(bad)


# ---- render.Style --------------------------------------------------------------------------------------------------------------------
def test_style_defaults_validation_and_actions():
    from mdqe_cvpr2023_amd.render import Style, blur_taps
    st = Style()
    assert (st.blur, st.blur_radius, st.mosaic, st.classes) == (None, 8, None, None) and st == Style(blur=None, blur_radius=8)
    for bad in ("track", "Tracks", "", 1, True):
        with pytest.raises(ValueError, match="blur"):
            Style(blur=bad)
    for bad in (0, 33, -2, 8.0, "8", True, None):
        with pytest.raises(ValueError, match="blur_radius"):
            Style(blur="tracks", blur_radius=bad)
    for mosaic in ("tracks", "background"):
        for blur in ("tracks", "background"):
            with pytest.raises(ValueError, match="(?s)mosaic.*blur"):
                Style(mosaic=mosaic, blur=blur)
    for kw in ({}, {"mosaic": "background"}, {"blur": "background"}):
        with pytest.raises(ValueError, match="classes"):
            Style(classes=[1], **kw)
    assert Style(blur="tracks", classes={7, 2, 2, 0}).classes == (0, 2, 7) and Style(mosaic="tracks", classes=[1]).classes == (1,)
    plain = [0] + [1] * 255
    assert Style(blur_radius=3).actions().tolist() == plain and Style().actions().dtype == torch.uint8
    assert Style(blur="background").actions().tolist() == [3] + [1] * 255
    assert Style(blur="tracks").actions().tolist() == [0] + [3] * 255
    assert Style(blur="tracks").actions(torch.zeros(3, 4)).tolist() == [0] + [3] * 255            # (the rows are not looked at)
    assert Style(mosaic="background").actions().tolist() == [2] + [1] * 255 and Style(mosaic="tracks").actions().tolist() == [0] + [2] * 255
    rows = torch.tensor([[0.1, 0.9, 0.2, 0.0],       # class 1
                         [0.5, 0.1, 0.5, 0.3],       # a tie of 0 and 2: class 0
                         [0.0, 0.2, 0.7, 0.7],       # a tie of 2 and 3: class 2
                         [0.0, 0.0, 0.0, 0.6]])      # class 3
    assert Style(blur="tracks", classes=[2]).actions(rows).tolist() == [0, 1, 1, 3, 1] + [1] * 251
    assert Style(blur="tracks", classes=[0, 3]).actions(rows).tolist() == [0, 1, 3, 1, 3] + [1] * 251
    assert Style(mosaic="tracks", classes=[0, 3]).actions(rows).tolist() == [0, 1, 2, 1, 2] + [1] * 251
    assert Style(blur="tracks", classes=[1]).actions(torch.zeros(0, 4)).tolist() == plain
    with pytest.raises(ValueError, match="class rows"):
        Style(blur="tracks", classes=[1]).actions()
    # the device tables: cached per device
    st = Style(blur="background", blur_radius=5)
    assert st.actions_on("cpu") is st.actions_on("cpu") and st.actions_on("cpu").tolist() == [3] + [1] * 255
    assert st.taps_on("cpu") is st.taps_on("cpu") and st.taps_c_on("cpu") is st.taps_c_on("cpu")
    assert st.taps_on("cpu").tolist() == blur_taps(5).tolist() and st.taps_c_on("cpu").tolist() == blur_taps(3).tolist()
    assert Style(blur="tracks").taps_c_on("cpu").tolist() == blur_taps(4).tolist() and Style(blur="tracks", blur_radius=32).taps_c_on("cpu").numel() == 17
    assert Style(blur="tracks", blur_radius=1).taps_c_on("cpu").tolist() == blur_taps(1).tolist()


# ---- the host path of ops.render_blur_yuv --------------------------------------------------------------------------------------------
def _typed(a, fmt):
    t = torch.from_numpy(a)
    return t if fmt == "nv12" else t.view(torch.int16)


def _raw(t, fmt):
    return t.numpy() if fmt == "nv12" else t.numpy().view(np.uint16)


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (7, 9), (9, 96)])
def test_host_path_equals_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import blur_taps
    F = 2
    ys, cs = YREF.make_content(H * 1000 + W, F, H, W, fmt)
    lab = OYREF.make_labels(H * 7 + W, F, H, W)
    pal_np = np.random.default_rng(H + W).integers(0, 256 if fmt == "nv12" else 1024, size=(256, 3)).astype(np.int64)
    pal = torch.from_numpy(pal_np.astype(np.uint16))
    tight = YREF.tight_pitch(W, fmt)
    flat, rows = YREF.pack(ys, cs, fmt, tight + 16, H + 1, extra_rows=2, lead=2)
    before = flat.copy()
    src = YuvFrames(*YREF.plane_views(torch.from_numpy(flat), F, H, W, fmt, tight + 16, H + 1, rows, 2), H, W, fmt=fmt, matrix="bt601")
    k = 0
    for radius in (0, 1, 5, 32):
        taps, taps_c = blur_taps(radius), blur_taps((radius + 1) // 2)
        for name, act in TABLES.items():
            a256, contour = (0, 128, 255, 256)[k % 4], k % 4
            wy, wc = REF.paint_yuv(ys, cs, lab, pal_np, act, fmt, a256, contour, _taps(radius), _taps((radius + 1) // 2))
            act_t = torch.from_numpy(act)
            if k % 2:                                                 # into a larger padded output at f_off = 1: nothing else is written
                oflat, orows = YREF.pack(np.zeros_like(ys).repeat(2, 0)[:F + 2], np.zeros_like(cs).repeat(2, 0)[:F + 2], fmt, tight + 8, H, 1)
                osave = oflat.copy()
                out = YuvFrames(*YREF.plane_views(torch.from_numpy(oflat), F + 2, H, W, fmt, tight + 8, H, orows), H, W, fmt=fmt)
                assert ops.render_blur_yuv(torch.from_numpy(lab), src, pal, act_t, taps, taps_c, out, 1, a256, contour) is out
                want = YuvFrames(*YREF.plane_views(torch.from_numpy(osave), F + 2, H, W, fmt, tight + 8, H, orows), H, W, fmt=fmt)
                want.y[1:1 + F, :, :W] = _typed(wy, fmt)
                want.uv[1:1 + F, :, :wc.shape[2]] = _typed(wc, fmt)
                assert np.array_equal(oflat, osave), (radius, name)
            else:                                                     # the output the wrapper makes: tight, the source's kind
                got = ops.render_blur_yuv(torch.from_numpy(lab), src, pal, act_t, taps, taps_c, a256=a256, contour=contour)
                assert (len(got), got.meta()) == (F, src.meta()) and tuple(got.y.shape) == (F, H, W)
                assert np.array_equal(_raw(got.y, fmt), wy) and np.array_equal(_raw(got.uv, fmt), wc), (radius, name)
            if name == "plain":                                       # ... and the plain overlay's host path
                ref = ops.render_overlay_yuv(torch.from_numpy(lab), src, pal, a256=a256, contour=contour)
                assert np.array_equal(_raw(ref.y, fmt), wy) and np.array_equal(_raw(ref.uv, fmt), wc)
            k += 1
    assert np.array_equal(flat, before)


def test_an_overlapping_out_is_refused():
    from mdqe_cvpr2023_amd import ops, render
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    act = render.Style(blur="background").actions()
    taps, taps_c = render.blur_taps(4), render.blur_taps(2)
    pal = render.palette_yuv(render.default_palette(), "nv12", "bt709", False, "rgb")
    lab = torch.zeros(2, 6, 8, dtype=torch.uint8)
    s = YuvFrames.empty(3, 6, 8)
    s.y.zero_(); s.uv.zero_()
    with pytest.raises(RuntimeError, match="render_blur_yuv: out must not share memory"):
        ops.render_blur_yuv(lab, s[:2], pal, act, taps, taps_c, s[:2])                  # in place
    with pytest.raises(RuntimeError, match="render_blur_yuv: out must not share memory"):
        ops.render_blur_yuv(lab, s[:2], pal, act, taps, taps_c, s, 1)                   # surface 1 is read and written
    other = ops.render_blur_yuv(lab, s[:2], pal, act, taps, taps_c, YuvFrames.empty(2, 6, 8))      # (apart: fine)
    assert len(other) == 2


# ---- the wrappers' refusals ----------------------------------------------------------------------------------------------------------
def test_wrapper_argument_checks():
    from mdqe_cvpr2023_amd import ops, render
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    act = render.Style(blur="tracks").actions()
    taps, taps_c = render.blur_taps(8), render.blur_taps(4)
    s = YuvFrames.empty(2, 6, 9, fmt="nv12")
    lab = torch.zeros(2, 6, 9, dtype=torch.uint8)
    pal = render.palette_yuv(render.default_palette(), "nv12", "bt709", False, "rgb")
    with pytest.raises(RuntimeError, match="render_blur_yuv: yuv must be a preprocess.YuvFrames"):
        ops.render_blur_yuv(lab, torch.zeros(2, 3, 6, 9, dtype=torch.uint8), pal, act, taps, taps_c)
    for bad in (lab.float(), lab[:1], lab[:, :, :8], torch.zeros(2, 6, 18, dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(RuntimeError, match="labels must be contiguous uint8"):
            ops.render_blur_yuv(bad, s, pal, act, taps, taps_c)
    for kw in ({"a256": 257}, {"a256": 128.0}, {"contour": 4}, {"contour": -1}):
        with pytest.raises(RuntimeError, match="a256 must be an int in 0..256 and contour an int in 0..3"):
            ops.render_blur_yuv(lab, s, pal, act, taps, taps_c, **kw)
    out = torch.zeros(2, 6, 9, 3, dtype=torch.uint8)
    rgb = render.default_palette()
    for bad in (act.float(), act[:255], torch.zeros(512, dtype=torch.uint8)[::2], None, act.tolist()):
        with pytest.raises(RuntimeError, match="action must be contiguous uint8 .256."):
            ops.render_blur_yuv(lab, s, pal, bad, taps, taps_c)
        with pytest.raises(RuntimeError, match="action must be contiguous uint8 .256."):
            ops.render_blur(lab, None, rgb, bad, taps, out)
    long_taps = torch.ones(34, dtype=torch.int32).to(torch.uint16)
    for bad in (taps.to(torch.int32), taps[:0], long_taps, long_taps[::2], taps.view(1, -1), None, taps.tolist()):
        with pytest.raises(RuntimeError, match="render_blur_yuv: taps must be contiguous uint16 .radius \\+ 1., radius in 0..32"):
            ops.render_blur_yuv(lab, s, pal, act, bad, taps_c)
        with pytest.raises(RuntimeError, match="render_blur: taps must be contiguous uint16 .radius \\+ 1., radius in 0..32"):
            ops.render_blur(lab, None, rgb, act, bad, out)
    for bad in (taps_c.to(torch.int32), long_taps[:18], None):
        with pytest.raises(RuntimeError, match="taps_c must be contiguous uint16 .radius \\+ 1., radius in 0..16"):
            ops.render_blur_yuv(lab, s, pal, act, taps, bad)
    for bad in (rgb, pal[:255]):
        with pytest.raises(RuntimeError, match="palette_yuv must be contiguous uint16"):
            ops.render_blur_yuv(lab, s, bad, act, taps, taps_c)
    for bad, f_off in ((YuvFrames.empty(2, 6, 8), 0), (YuvFrames.empty(2, 6, 9, fmt="p010"), 0), (YuvFrames.empty(2, 6, 9), 1), (lab, 0)):
        with pytest.raises(RuntimeError, match="out must be a YuvFrames"):
            ops.render_blur_yuv(lab, s, pal, act, taps, taps_c, bad, f_off)
    # the RGB wrapper: shapes and dtypes first, devices after (a host without a GPU gets as far as the device check)
    with pytest.raises(RuntimeError, match="render_blur: labels must be contiguous uint8"):
        ops.render_blur(lab.float(), None, rgb, act, taps, out)
    with pytest.raises(RuntimeError, match="palette must be contiguous uint8"):
        ops.render_blur(lab, None, pal, act, taps, out)
    with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
        ops.render_blur(lab, None, rgb, act, taps, out[:1])
    with pytest.raises(RuntimeError, match="frames must be uint8 or float32"):
        ops.render_blur(lab, torch.zeros(2, 4, 6, 9), rgb, act, taps, out)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor on out's device"):
        ops.render_blur(lab, None, rgb, act, taps, out)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_both_entries_and_they_refuse_bad_arguments():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    for name, n_args in (("mdqe_render_blur_u8", 18), ("mdqe_render_blur_yuv420sp", 27)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
        assert hasattr(h, name) and name in _lib.SIGNATURES
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == n_args
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # new entries only
    EINVAL, ENULL = 1, 3

    def rgb(F=1, Ho=8, Wo=8, a256=128, contour=1, radius=8, f_off=0):
        return h.mdqe_render_blur_u8(None, 1, 0, 0, 0, None, F, Ho, Wo, None, None, a256, contour, None, radius, None, f_off, None)

    def yuv(F=1, H=32, W=64, fmt=0, a256=128, contour=1, radius=8, radius_c=4, f_off=0, yp=64, ptrs=None, **kw):
        q = dict({"y": None, "uv": None, "labels": None, "pal": None, "act": None, "taps": None, "taps_c": None, "oy": None, "ouv": None},
                 **(ptrs or {}))
        q.update(kw)
        return h.mdqe_render_blur_yuv420sp(q["y"], yp, 64 * 48, q["uv"], 64, 64 * 48, F, H, W, fmt, q["labels"], q["pal"], q["act"],
                                           a256, contour, q["taps"], radius, q["taps_c"], radius_c, q["oy"], 64, 64 * 48, q["ouv"], 64,
                                           64 * 48, f_off, None)
    for call in (rgb, yuv):
        for kw in ({"radius": -1}, {"radius": 33}, {"contour": 4}, {"a256": 257}, {"F": -1}, {"f_off": -1}):
            assert call(**kw) == EINVAL, (call.__name__, kw)
            if "F" not in kw:
                assert call(**dict(kw, F=0)) == EINVAL, (call.__name__, kw)                       # ... whatever F says
        for radius in (0, 1, 32):
            assert call(F=0, radius=radius) == 0                                                   # F = 0: OK, nothing launched
        assert call() == ENULL
    for radius_c in (-1, 17):
        assert yuv(radius_c=radius_c) == EINVAL and yuv(radius_c=radius_c, F=0) == EINVAL
    assert yuv(F=0, radius_c=0) == 0 and yuv(F=0, radius_c=16) == 0
    assert yuv(yp=63) == EINVAL and yuv(fmt=2) == EINVAL and rgb(Ho=0) == EINVAL
    # never dereferenced (the refusals come before the launch): any overlap of an output plane, in place included, and the tap tables
    ptrs = {"y": 1 << 20, "uv": 2 << 20, "labels": 3 << 20, "pal": 4 << 20, "act": 7 << 20, "taps": 8 << 20, "taps_c": 9 << 20,
            "oy": 5 << 20, "ouv": 6 << 20}
    for kw in ({"oy": ptrs["y"]}, {"ouv": ptrs["uv"]}, {"oy": ptrs["y"] + 64}, {"oy": ptrs["uv"]}, {"ouv": ptrs["y"]},
               {"ouv": ptrs["oy"] + 64 * 31}, {"oy": ptrs["labels"] + 5}, {"ouv": ptrs["pal"] + 1024}, {"oy": ptrs["act"] - 64 * 31},
               {"oy": ptrs["taps"] - 64 * 31}, {"ouv": ptrs["taps_c"] + 8}, {"taps": ptrs["oy"] + 100}, {"taps_c": ptrs["ouv"] + 64 * 15},
               {"taps": ptrs["taps"] + 1}):
        assert yuv(ptrs=ptrs, **kw) == EINVAL, kw
    for missing in ("act", "taps", "taps_c"):
        assert yuv(ptrs=dict(ptrs, **{missing: None})) == ENULL


# ---- merge.overlay_frames: which launches a style makes ---------------------------------------------------------------------------------
class _Store:
    """A FrameStore's `pieces` for frames [10, 15): two pieces of 3 and 2 frames."""
    def __init__(self, make):
        self.make = make

    def pieces(self, f0, f1, stream=None):
        assert (f0, f1) == (10, 15)
        return [(self.make(3), 10), (self.make(2), 13)]


def _record(monkeypatch, style, surface):
    """The (name, args) of every ops painter call merge.overlay_frames makes for one window of 5 frames of 6 x 8 and 2 tracks."""
    from mdqe_cvpr2023_amd import merge, ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    calls = []
    for name in ("render_overlay", "render_overlay_yuv", "render_mosaic", "render_mosaic_yuv", "render_blur", "render_blur_yuv",
                 "annotate", "annotate_yuv", "render_trails", "render_trails_yuv"):
        monkeypatch.setattr(ops, name, (lambda n: lambda *a, **kw: calls.append((n, a, kw)))(name))
    monkeypatch.setattr(merge, "label_maps", lambda *a: torch.zeros(2, 5, 5, dtype=torch.int32))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    m = torch.zeros(2, 5, 3, 4)
    labels = torch.arange(7 * 6 * 8, dtype=torch.int64).remainder(3).to(torch.uint8).view(7, 6, 8)
    if surface:
        out = YuvFrames.empty(6, 6, 8, fmt="nv12", matrix="bt601", full_range=True, order="bgr")
        store = _Store(lambda k: YuvFrames.empty(k, 6, 8, fmt="nv12", matrix="bt601", full_range=True, order="bgr"))
    else:
        out = torch.zeros(6, 6, 8, 3, dtype=torch.uint8)
        store = _Store(lambda k: torch.zeros(k, 3, 6, 8, dtype=torch.uint8))
    cls = torch.tensor([[0.9, 0.1], [0.2, 0.8]])
    assert merge.overlay_frames(m, 8, (6, 8), (6, 8), False, labels, 1, store, 10, style, cls, out, 1) is None
    return calls, labels, out


@pytest.mark.parametrize("surface", [False, True])
def test_overlay_frames_makes_the_former_calls_by_default_and_the_blur_calls_for_a_blur_style(monkeypatch, surface):
    from mdqe_cvpr2023_amd.render import Style, blur_taps
    sfx = "_yuv" if surface else ""

    def pal_of(st):
        return st.palette_yuv_on("cpu", "nv12", "bt601", True, "bgr") if surface else st.palette_on("cpu")
    # the default style: exactly the plain painter's calls, one per piece, with the plain painter's arguments
    st = Style()
    calls, labels, out = _record(monkeypatch, st, surface)
    assert [c[0] for c in calls] == ["render_overlay" + sfx] * 2 and all(not c[2] for c in calls)
    for (_, a, _), (l0, k, off) in zip(calls, ((1, 3, 1), (4, 2, 4))):
        assert len(a) == 7 and torch.equal(a[0], labels[l0:l0 + k]) and len(a[1]) == k and a[2] is pal_of(st)
        assert a[3] is out and a[4:] == (off, 128, 1)
    # a mosaic style: the mosaic's calls, as before
    st = Style(mosaic="tracks", cell=4)
    calls, labels, out = _record(monkeypatch, st, surface)
    assert [c[0] for c in calls] == ["render_mosaic" + sfx] * 2
    assert all(len(a) == 9 and a[3] is st.actions_on("cpu") and a[4] is out and a[5:] == (off, 128, 1, 4) for (_, a, _), off in zip(calls, (1, 4)))
    # blur styles: the blur's calls with the style's tables
    for st in (Style(blur="tracks", alpha=0.25, contour=2), Style(blur="background", blur_radius=5), Style(blur="tracks", classes=[1], blur_radius=32)):
        calls, labels, out = _record(monkeypatch, st, surface)
        assert [c[0] for c in calls] == ["render_blur" + sfx] * 2 and all(not c[2] for c in calls)
        want_act = st.actions().tolist() if st.classes is None else [0, 1, 3] + [1] * 253         # (track 1's first maximum is class 1)
        for (_, a, _), (l0, k, off) in zip(calls, ((1, 3, 1), (4, 2, 4))):
            assert torch.equal(a[0], labels[l0:l0 + k]) and len(a[1]) == k and a[2] is pal_of(st) and a[3].tolist() == want_act
            assert a[4] is st.taps_on("cpu") and a[4].tolist() == blur_taps(st.blur_radius).tolist()
            rest = a[5:]
            if surface:
                assert rest[0] is st.taps_c_on("cpu") and rest[0].tolist() == blur_taps((st.blur_radius + 1) // 2).tolist()
                rest = rest[1:]
            assert rest[0] is out and rest[1:] == (off, st.a256, st.contour)
    # trails and annotations run behind a blur as behind every painter
    st = Style(blur="tracks", box=2, caption="id")
    calls, _, _ = _record(monkeypatch, st, surface)
    assert [c[0] for c in calls] == ["render_blur" + sfx] * 2 + ["annotate" + sfx] * 2
