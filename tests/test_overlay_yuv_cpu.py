"""Overlays painted onto decoder surfaces, the host side: the ABI entry's declaration, binding and refusals; render.palette_yuv (greys,
nominal codes, the table against the reference's own derivation, the pinned round trip through the existing YUV -> RGB rule); the host
restatement of ops.render_overlay_yuv against the numpy oracle (tests/_overlay_yuv_ref.py) over the shape list of the GPU tests; the
setter, every refusal, and the frame store on YuvFrames chunks.  No GPU."""
import dataclasses
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _overlay_yuv_ref as REF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402

SHAPES = [(1, 1), (2, 2), (3, 5), (7, 9), (6, 36), (5, 37), (16, 64), (9, 96)]
ROWS = [(fmt, matrix, full) for fmt in ("nv12", "p010") for matrix in ("bt601", "bt709") for full in (False, True)]
BITS = {"nv12": 8, "p010": 10}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)


# ---- the ABI entry -------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_entry_and_it_refuses_bad_arguments():
    from mdqe_cvpr2023_amd import _lib
    name = "mdqe_render_overlay_yuv420sp"
    src = _header()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
    assert hasattr(h, name) and name in _lib.SIGNATURES
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == 22
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # a new entry only: nothing existing changed
    fn = getattr(h, name)

    def call(y=None, yp=64, ys=64 * 48, uv=None, cp=64, cs=64 * 48, F=1, H=32, W=64, fmt=0, labels=None, pal=None, a256=128, contour=1,
             oy=None, oyp=64, oys=64 * 48, ouv=None, ocp=64, ocs=64 * 48, f_off=0):
        return fn(y, yp, ys, uv, cp, cs, F, H, W, fmt, labels, pal, a256, contour, oy, oyp, oys, ouv, ocp, ocs, f_off, None)
    # refused before any pointer is looked at (NULL everywhere: nothing can be launched)
    EINVAL, ENULL = 1, 3
    p010 = {"fmt": 1, "yp": 128, "cp": 128, "oyp": 128, "ocp": 128}
    for kw in ({"contour": 4}, {"contour": -1}, {"a256": 257}, {"a256": -1}, {"F": -1}, {"H": 0}, {"W": 0}, {"W": -4}, {"fmt": 2}, {"fmt": -1},
               {"f_off": -1},
               {"yp": 63}, {"cp": 63}, {"oyp": 63}, {"ocp": 63},                                    # a pitch below a row
               {"W": 63, "yp": 63, "cp": 63}, {"W": 63, "oyp": 63, "ocp": 63},                      # 63 pixels: 32 chroma pairs = 64 bytes
               dict(p010, yp=127), dict(p010, ocp=126),                                             # P010: a row is 2 * W bytes
               dict(p010, yp=129), dict(p010, cp=131), dict(p010, oyp=129), dict(p010, ocp=131),    # odd P010 pitches
               dict(p010, ys=128 * 48 + 1), dict(p010, ocs=128 * 48 + 1),                           # ... and strides
               {"ys": -64}, {"cs": -1}, {"oys": -64}, {"ocs": -1},
               {"F": 1 << 20, "H": 1024, "W": 1024, "yp": 1024, "cp": 1024, "oyp": 1024, "ocp": 1024,
                "oys": 1 << 20, "ocs": 1 << 19}):                                                  # F * H * W >= 2^31 - 1
        assert call(**kw) == EINVAL, kw
        if "F" not in kw:
            assert call(**dict(kw, F=0)) == EINVAL, kw                                              # ... whatever F says
    assert call(F=2, oys=64 * 31 + 63) == EINVAL and call(F=2, ocs=64 * 15 + 63) == EINVAL          # two output surfaces would share bytes
    assert call(F=0) == 0 and call(**dict(p010, F=0)) == 0                                          # F = 0: OK, nothing launched
    assert call(W=63, yp=63, cp=64, oyp=63, ocp=64, F=0) == 0                                       # the tightest legal pitches
    assert call() == ENULL
    # never dereferenced (the refusals come before the launch): odd P010 plane pointers, an odd palette pointer, overlapping planes
    ptrs = {"y": 1 << 20, "uv": 2 << 20, "labels": 3 << 20, "pal": 4 << 20, "oy": 5 << 20, "ouv": 6 << 20}
    for k in ("y", "uv", "oy", "ouv"):
        assert call(**dict(p010, **dict(ptrs, **{k: ptrs[k] + 1}))) == EINVAL, k
    assert call(**dict(ptrs, pal=ptrs["pal"] + 1)) == EINVAL
    for kw in ({"oy": ptrs["y"] + 64}, {"ouv": ptrs["uv"] + 2}, {"oy": ptrs["y"], "oyp": 128}, {"oy": ptrs["uv"]}, {"ouv": ptrs["y"]},
               {"ouv": ptrs["oy"] + 64 * 31}, {"oy": ptrs["labels"] + 5}, {"ouv": ptrs["pal"] + 1024},
               {"oy": ptrs["y"] - 64 * 47, "f_off": 1, "F": 2}):                                   # (in place only at the SAME surfaces)
        assert call(**dict(ptrs, **kw)) == EINVAL, kw


# ---- the palette in YUV --------------------------------------------------------------------------------------------------------------
def _ramp(values):
    """A 256-row palette whose first rows are the greys `values` (the rest black)."""
    pal = torch.zeros(256, 3, dtype=torch.uint8)
    v = torch.tensor(list(values), dtype=torch.uint8)
    pal[:len(v)] = v[:, None]
    return pal


@pytest.mark.parametrize("fmt,matrix,full", ROWS)
def test_palette_yuv_greys_nominal_codes_and_the_table(fmt, matrix, full):
    from mdqe_cvpr2023_amd import render
    bits = BITS[fmt]
    assert render.YUV_FORWARD[(fmt, matrix, full)] == REF.forward_table(matrix, full, bits)
    yo, co, ky, ku, kv = render.YUV_FORWARD[(fmt, matrix, full)]
    assert sum(ku) == 0 and sum(kv) == 0
    scale = ((1 << bits) - 1 if full else 219 << (bits - 8)) / 255.0
    assert sum(ky) == int(np.rint(scale * 65536))
    greys = render.palette_yuv(_ramp(range(256)), fmt, matrix, full, "rgb")
    assert greys.dtype == torch.uint16 and tuple(greys.shape) == (256, 3) and not greys.is_cuda
    g = greys.view(torch.int16).numpy().astype(np.int64)
    assert bool((g[:, 1:] == co).all())                                # every grey: exactly neutral chroma
    lo, hi = {(8, False): (16, 235), (8, True): (0, 255), (10, False): (64, 940), (10, True): (0, 1023)}[(bits, full)]
    assert (int(g[0, 0]), int(g[255, 0])) == (lo, hi)                  # black and white on the nominal codes
    assert bool((np.diff(g[:, 0]) >= 0).all())
    # any palette, both orders: the reference's table
    rng = np.random.default_rng(5)
    pal = torch.from_numpy(rng.integers(0, 256, size=(256, 3)).astype(np.uint8))
    pal[1], pal[2], pal[3] = torch.tensor([255, 0, 0]), torch.tensor([0, 0, 255]), torch.tensor([0, 255, 0])      # (the corners of chroma)
    for order in ("rgb", "bgr"):
        got = render.palette_yuv(pal, fmt, matrix, full, order).view(torch.int16).numpy().astype(np.int64)
        assert np.array_equal(got, REF.palette_yuv(pal.numpy(), fmt, matrix, full, order)), order
        assert int(got.min()) >= 0 and int(got.max()) <= (1 << bits) - 1
    assert torch.equal(render.palette_yuv(pal, fmt, matrix, full, "bgr"), render.palette_yuv(pal.flip(1), fmt, matrix, full, "rgb"))


@pytest.mark.parametrize("fmt,matrix,full", ROWS)
def test_default_palette_round_trip_is_pinned(fmt, matrix, full):
    """default palette -> palette_yuv -> the existing YUV -> RGB rule: the worst channel error, asserted as measured (a pin)."""
    from mdqe_cvpr2023_amd import render
    pal = render.default_palette()
    t = render.palette_yuv(pal, fmt, matrix, full, "rgb").view(torch.int16).numpy().astype(np.int64)
    (r, g, b), _ = YREF.rule(t[:, 0], t[:, 1], t[:, 2], matrix, full, BITS[fmt])
    worst = int(np.abs(np.stack([r, g, b], 1) - pal.numpy().astype(np.int64)).max())
    print(fmt, matrix, full, "round-trip worst channel error", worst)
    assert worst == REF.ROUND_TRIP_WORST[(fmt, matrix, full)]


def test_palette_yuv_validation_and_the_style_cache():
    from mdqe_cvpr2023_amd import render
    pal = render.default_palette()
    for bad in (pal.float(), pal[:255], pal.numpy()):
        with pytest.raises(ValueError, match="palette_rgb"):
            render.palette_yuv(bad, "nv12", "bt709", False, "rgb")
    for kw in ({"fmt": "i420"}, {"matrix": "bt2020"}, {"full_range": 1}, {"order": "gbr"}):
        with pytest.raises(ValueError, match="palette_yuv"):
            render.palette_yuv(pal, **dict({"fmt": "nv12", "matrix": "bt709", "full_range": False, "order": "rgb"}, **kw))
    st = render.Style()
    a = st.palette_yuv_on("cpu", "nv12", "bt709", False, "rgb")
    assert st.palette_yuv_on("cpu", "nv12", "bt709", False, "rgb") is a and torch.equal(a, render.palette_yuv(pal, "nv12", "bt709", False, "rgb"))
    b = st.palette_yuv_on("cpu", "p010", "bt601", True, "bgr")
    assert b is not a and torch.equal(b, render.palette_yuv(pal, "p010", "bt601", True, "bgr"))
    assert st == render.Style()                                       # (the caches are no fields)


# ---- the host restatement of the op --------------------------------------------------------------------------------------------------
def _typed(a, fmt):
    t = torch.from_numpy(a)
    return t if fmt == "nv12" else t.view(torch.int16)


def _raw(t, fmt):
    return t.numpy() if fmt == "nv12" else t.numpy().view(np.uint16)


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_host_restatement_equals_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops, render
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    F = 3
    ys, cs = YREF.make_content(H * 1000 + W, F, H, W, fmt)
    lab = REF.make_labels(H * 7 + W, F, H, W)
    pal = render.palette_yuv(render.default_palette(), fmt, "bt601", False, "rgb")
    pal_np = pal.view(torch.int16).numpy().astype(np.int64)
    tight = YREF.tight_pitch(W, fmt)
    flat, rows = YREF.pack(ys, cs, fmt, tight + 16, H + 1, extra_rows=2, lead=2)
    before = flat.copy()
    src = YuvFrames(*YREF.plane_views(torch.from_numpy(flat), F, H, W, fmt, tight + 16, H + 1, rows, 2), H, W, fmt=fmt, matrix="bt601")
    k = 0
    for contour in range(4):
        for a256 in (0, 1, 128, 255, 256):
            wy, wc = REF.paint(ys, cs, lab, pal_np, fmt, a256, contour)
            if k % 2:                                                 # into a larger padded output at f_off = 1: nothing else is written
                oflat, orows = YREF.pack(np.zeros_like(ys).repeat(2, 0)[:F + 2], np.zeros_like(cs).repeat(2, 0)[:F + 2], fmt, tight + 8, H, 1)
                osave = oflat.copy()
                out = YuvFrames(*YREF.plane_views(torch.from_numpy(oflat), F + 2, H, W, fmt, tight + 8, H, orows), H, W, fmt=fmt)
                got = ops.render_overlay_yuv(torch.from_numpy(lab), src, pal, out, 1, a256, contour)
                assert got is out
                want = YuvFrames(*YREF.plane_views(torch.from_numpy(osave), F + 2, H, W, fmt, tight + 8, H, orows), H, W, fmt=fmt)
                want.y[1:1 + F, :, :W] = _typed(wy, fmt)
                want.uv[1:1 + F, :, :wc.shape[2]] = _typed(wc, fmt)
                assert np.array_equal(oflat, osave), (contour, a256)
            else:                                                     # the output the wrapper makes: tight, the source's kind
                got = ops.render_overlay_yuv(torch.from_numpy(lab), src, pal, a256=a256, contour=contour)
                assert (len(got), got.meta()) == (F, src.meta()) and got.y.is_contiguous() and tuple(got.y.shape) == (F, H, W)
                assert np.array_equal(_raw(got.y, fmt), wy) and np.array_equal(_raw(got.uv, fmt), wc), (contour, a256)
            k += 1
    assert np.array_equal(flat, before)
    # in place: the output IS the input
    mine = YuvFrames(_typed(ys.copy(), fmt), _typed(cs.copy(), fmt), H, W, fmt=fmt)
    assert ops.render_overlay_yuv(torch.from_numpy(lab), mine, pal, mine, 0, 77, 2) is mine
    wy, wc = REF.paint(ys, cs, lab, pal_np, fmt, 77, 2)
    assert np.array_equal(_raw(mine.y, fmt), wy) and np.array_equal(_raw(mine.uv, fmt), wc)


def test_reference_properties_on_a_hand_case():
    """The oracle itself on cases worked out by hand: a 3 x 3 NV12 picture, label 9 on the left column, colour (200, 60, 240)."""
    pal = np.zeros((256, 3), dtype=np.int64)
    pal[9] = (200, 60, 240)
    ys = np.full((1, 3, 3), 100, dtype=np.uint8)
    cs = np.array([[[120, 130, 121, 131], [122, 132, 123, 133]]], dtype=np.uint8)
    lab = np.zeros((1, 3, 3), dtype=np.uint8)
    lab[0, :, 0] = 9
    oy, oc = REF.paint(ys, cs, lab, pal, "nv12", 128, 0)
    assert oy[0].tolist() == [[150, 100, 100]] * 3                    # (100 * 128 + 200 * 128 + 128) >> 8
    # block (0, 0): two pixels painted, two kept: U = (2 * ((120 * 128 + 60 * 128 + 128) >> 8) + 2 * 120 + 2) >> 2 = (180 + 240 + 2) >> 2
    # = 105, V = (2 * 185 + 2 * 130 + 2) >> 2 = 158; block (0, 1) (one column, two rows, background): kept; block (1, 0) (one row, two
    # columns): U = (((122 * 128 + 60 * 128 + 128) >> 8) + 122 + 1) >> 1 = (91 + 122 + 1) >> 1 = 107, V = (186 + 132 + 1) >> 1 = 159
    assert oc[0].tolist() == [[105, 158, 121, 131], [107, 159, 123, 133]]
    oy, oc = REF.paint(ys, cs, lab, pal, "nv12", 128, 1)              # every pixel of the column has a background neighbour: the colour
    assert oy[0].tolist() == [[200, 100, 100]] * 3
    assert oc[0].tolist() == [[(2 * 60 + 2 * 120 + 2) >> 2, (2 * 240 + 2 * 130 + 2) >> 2, 121, 131], [(60 + 122 + 1) >> 1, (240 + 132 + 1) >> 1, 123, 133]]
    # P010: untouched words keep their low bits, painted ones are value << 6
    ys10 = ((ys.astype(np.uint16) * 4) << 6) | 0x2A
    cs10 = ((cs.astype(np.uint16) * 4) << 6) | 0x15
    oy, oc = REF.paint(ys10, cs10, lab, pal * 4, "p010", 256, 0)
    assert oy[0].tolist() == [[800 << 6, (400 << 6) | 0x2A, (400 << 6) | 0x2A]] * 3
    assert oc[0, 0].tolist() == [((2 * 240 + 2 * 480 + 2) >> 2) << 6, ((2 * 960 + 2 * 520 + 2) >> 2) << 6, (484 << 6) | 0x15, (524 << 6) | 0x15]


def test_wrapper_argument_checks():
    from mdqe_cvpr2023_amd import ops, render
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    s = YuvFrames.empty(2, 6, 9, fmt="nv12")
    lab = torch.zeros(2, 6, 9, dtype=torch.uint8)
    pal = render.palette_yuv(render.default_palette(), "nv12", "bt709", False, "rgb")
    with pytest.raises(RuntimeError, match="yuv must be a preprocess.YuvFrames"):
        ops.render_overlay_yuv(lab, torch.zeros(2, 3, 6, 9, dtype=torch.uint8), pal)
    for bad in (lab.float(), lab[:1], lab[:, :, :8], torch.zeros(2, 6, 18, dtype=torch.uint8)[:, :, ::2], torch.zeros(2, 5, 8, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="labels must be contiguous uint8"):
            ops.render_overlay_yuv(bad, s, pal)
    for kw in ({"a256": 257}, {"a256": -1}, {"a256": 128.0}, {"contour": 4}, {"contour": -1}):
        with pytest.raises(RuntimeError, match="a256 must be an int in 0..256 and contour an int in 0..3"):
            ops.render_overlay_yuv(lab, s, pal, **kw)
    for bad in (render.default_palette(), pal[:255], pal.view(torch.int16).to(torch.int32)):
        with pytest.raises(RuntimeError, match="palette_yuv must be contiguous uint16"):
            ops.render_overlay_yuv(lab, s, bad)
    for bad, f_off in ((YuvFrames.empty(2, 6, 8), 0), (YuvFrames.empty(2, 6, 9, fmt="p010"), 0), (YuvFrames.empty(2, 6, 9), 1), (lab, 0),
                       (YuvFrames.empty(3, 6, 9), -1)):
        with pytest.raises(RuntimeError, match="out must be a YuvFrames"):
            ops.render_overlay_yuv(lab, s, pal, bad, f_off)


def test_yuvframes_empty_cat_and_meta():
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    a = YuvFrames.empty(2, 5, 9, fmt="p010", matrix="bt601", full_range=True, order="bgr")
    assert (tuple(a.y.shape), tuple(a.uv.shape), a.y.dtype) == ((2, 5, 9), (2, 3, 10), torch.int16)
    assert a.meta() == (5, 9, "p010", "bt601", True, "bgr") and not a.is_cuda
    b = YuvFrames.empty(3, 5, 9, fmt="p010", pitch_align=64, matrix="bt601", full_range=True, order="bgr")
    assert (tuple(b.y.shape), tuple(b.uv.shape)) == ((3, 5, 32), (3, 3, 32)) and not bool(b.y.any()) and not bool(b.uv.any())
    c = YuvFrames.empty(1, 4, 6, pitch_align=4)
    assert (tuple(c.y.shape), tuple(c.uv.shape)) == ((1, 4, 8), (1, 2, 8))
    for k in (0, -4, 2.0, True):
        with pytest.raises(ValueError, match="pitch_align"):
            YuvFrames.empty(1, 4, 6, pitch_align=k)
    with pytest.raises(ValueError, match="pitch_align"):
        YuvFrames.empty(1, 4, 6, fmt="p010", pitch_align=3)
    a.y.fill_(7), a.uv.fill_(9)
    a2 = a.clone()
    a2.y.fill_(8)
    both = YuvFrames.cat([a, a2])
    assert len(both) == 4 and both.meta() == a.meta() and both.y[:, 0, 0].tolist() == [7, 7, 8, 8] and bool((both.uv == 9).all())
    for bad in ([], [a, b[:1].used_rows()._like(b.y[:1, :, :9], b.uv[:1, :, :10]), torch.zeros(1)], [a, YuvFrames.empty(1, 5, 9, fmt="p010")]):
        with pytest.raises(ValueError, match="YuvFrames.cat"):
            YuvFrames.cat(bad)


# ---- setters and refusals ------------------------------------------------------------------------------------------------------------
def _standin(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)

    def check():
        from mdqe_cvpr2023_amd.meta_arch import MDQE
        MDQE.check_label_capacity(types.SimpleNamespace(cfg=cfg))
    return types.SimpleNamespace(cfg=cfg, device=torch.device("cuda", 0), check_label_capacity=check)


def _cpu_model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    return MDQE(dataclasses.replace(PRESETS["R50_ovis_360"], **kw), seed=1)


def test_overlay_output_surface_round_trips_and_resolves_into_the_forms():
    from mdqe_cvpr2023_amd.merge import Forms
    m = _cpu_model()
    assert m.overlay_output is False and Forms.of_model(m).surface is False
    m.overlay_output = "surface"
    assert m.overlay_output == "surface"
    f = Forms.of_model(m)
    assert f.overlay and f.surface and not f.labels and f.planes == "dense"
    m.overlay_output = True
    assert m.overlay_output is True and Forms.of_model(m).overlay and not Forms.of_model(m).surface
    for bad in ("surfaces", "yuv", 1, None):
        with pytest.raises(ValueError, match="overlay_output"):
            m.overlay_output = bad
    m.overlay_output = False
    assert Forms.of_model(m) == Forms(planes="dense")
    with pytest.raises(ValueError, match="n_max_inst"):
        _cpu_model(n_max_inst=256).overlay_output = "surface"
    assert Forms.of_emit("overlay", surface=True).surface and not Forms.of_emit("overlay").surface
    assert not Forms.of_emit("labels", surface=True).surface          # (the session refuses it before; the record never claims it)


def test_online_refusals_name_the_remedy():
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    ov = MDQE.online_video(_standin(), emit="overlay", surface=True, surface_pitch_align=64)
    assert ov.surface is True and ov.surface_pitch_align == 64 and ov.frames_held == 0
    assert MDQE.online_video(_standin(), emit="overlay").surface is False
    for emit in ("masks", "rle", "labels"):                           # surface without emit="overlay"
        with pytest.raises(ValueError, match="emit='overlay'"):
            MDQE.online_video(_standin(), emit=emit, surface=True)
    with pytest.raises(ValueError, match="surface must be a bool"):
        MDQE.online_video(_standin(), emit="overlay", surface="nv12")
    for k, kw in ((0, {"surface": True}), (2.0, {"surface": True}), (64, {})):
        with pytest.raises(ValueError, match="surface_pitch_align"):
            MDQE.online_video(_standin(), emit="overlay", surface_pitch_align=k, **kw)
    with pytest.raises(ValueError, match="COCO image config.*video config"):
        MDQE.online_video(_standin(is_coco=True), emit="overlay", surface=True)
    # a push of RGB tensors
    assert ov.push(torch.empty(0, 3, 8, 8, dtype=torch.uint8)) == []
    for rgb in (torch.zeros(2, 3, 8, 8, dtype=torch.uint8), [torch.zeros(3, 8, 8)]):
        with pytest.raises(ValueError, match="takes pushes of preprocess.YuvFrames.*surface=False"):
            ov.push(rgb)
    # an output size that is not the surfaces'
    small = MDQE.online_video(_standin(), height=90, width=150, emit="overlay", surface=True)
    with pytest.raises(ValueError, match=r"height=96, width=160.*model\.resize_on_device"):
        small._start(torch.zeros(1, 3, 96, 160, dtype=torch.uint8), 96, 160)
    assert small.merger is None
    # surfaces of another kind than the first push's
    from mdqe_cvpr2023_amd.merge import FrameStore
    ov.store, ov.in_hw = FrameStore(), (8, 8)
    ov.store.add(0, YuvFrames.empty(2, 8, 8))
    with pytest.raises(ValueError, match="one session's surfaces are of one kind"):
        ov.push(YuvFrames.empty(2, 8, 8, matrix="bt601"))
    with pytest.raises(RuntimeError, match="differs from the first push"):
        ov.push(YuvFrames.empty(2, 8, 10))


def test_offline_refusals_name_the_remedy():
    from mdqe_cvpr2023_amd import merge, sharding
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    m = _cpu_model()
    m.overlay_output = "surface"
    with pytest.raises(ValueError, match="RGB tensors.*preprocess.YuvFrames.*overlay_output = True"):       # a video of RGB tensors
        m._frame_source(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), None)
    store = m._frame_source(YuvFrames.empty(4, 8, 12, fmt="p010", matrix="bt601"), None)
    assert store.surface == (8, 12, "p010", "bt601", False, "rgb") and store.frames_held == 4
    pic = merge.surface_picture(store, 3, (8, 12), "cpu", pitch_align=32)
    assert len(pic) == 3 and pic.meta() == store.surface and tuple(pic.y.shape) == (3, 8, 16)
    with pytest.raises(ValueError, match=r"height=8, width=12.*model\.resize_on_device"):                    # another output size
        merge.surface_picture(store, 3, (6, 9), "cpu")
    rgb = merge.FrameStore()
    rgb.add(0, torch.zeros(2, 3, 8, 12, dtype=torch.uint8))
    for src in (rgb, None):
        with pytest.raises(ValueError, match="preprocess.YuvFrames"):
            merge.surface_picture(src, 2, (8, 12), "cpu")
    m.overlay_output = True
    assert m._frame_source(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), None).surface is None
    m.overlay_output = False
    assert m._frame_source(YuvFrames.empty(4, 8, 12), None) is None
    # a COCO image config
    cfg = m.cfg
    coco = types.SimpleNamespace(cfg=dataclasses.replace(cfg, is_coco=True), engine=None, device=torch.device("cpu"), overlay_output="surface")
    with pytest.raises(ValueError, match="COCO image branch has no overlay.*video config"):
        MDQE.inference_image(coco, [{"image": torch.zeros(3, 3, 8, 8)}])
    # the sharded driver
    geo = types.SimpleNamespace(Hp=8, Wp=8, N=4)
    model = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), engine=types.SimpleNamespace(geometry=lambda h, w: geo), overlay_output="surface")
    with pytest.raises(ValueError, match="overlay_output is not offered by the sharded driver.*one device"):
        sharding.run_round_robin(model, {0: torch.zeros(4, 3, 8, 8)}, [(0, 0, 4)], 0, 1, None, (8, 8))


# ---- the frame store on surfaces -----------------------------------------------------------------------------------------------------
def test_frame_store_with_surface_chunks():
    from mdqe_cvpr2023_amd.merge import FrameStore
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    st, at, chunks = FrameStore(), 0, []
    for n in (4, 0, 3, 5):                                             # frames 0..3, 4..6, 7..11 (an empty push holds nothing)
        s = YuvFrames.empty(n, 4, 6, pitch_align=8)
        s.y[:] = torch.arange(at, at + n, dtype=torch.uint8).view(n, 1, 1)
        s.uv[:] = 100 + torch.arange(at, at + n, dtype=torch.uint8).view(n, 1, 1)
        st.add(at, s)
        chunks.append(s)
        at += n
    assert st.frames_held == 12 and len(st.chunks) == 3 and st.surface == (4, 6, "nv12", "bt709", False, "rgb")
    one = st.pieces(1, 3)
    assert [(type(t), len(t), f) for t, f in one] == [(YuvFrames, 2, 1)] and one[0][0].y[:, 0, 0].tolist() == [1, 2]
    assert one[0][0].y.untyped_storage().data_ptr() == chunks[0].y.untyped_storage().data_ptr()          # views: no copy
    two = st.pieces(2, 6)                                             # a window that spans two pushes: two pieces
    assert [(len(t), f) for t, f in two] == [(2, 2), (2, 4)]
    assert sum((t.y[:, 0, 0].tolist() for t, _ in two), []) == [2, 3, 4, 5] and sum((t.uv[:, 0, 0].tolist() for t, _ in two), []) == [102, 103, 104, 105]
    assert [(len(t), f) for t, f in st.pieces(3, 9)] == [(1, 3), (3, 4), (2, 7)]
    with pytest.raises(RuntimeError, match="does not hold"):
        st.pieces(10, 13)
    st.drop_before(3)                                                 # chunk 0 still holds frame 3
    assert st.frames_held == 12
    st.drop_before(4)
    assert st.frames_held == 8 and [c[0] for c in st.chunks] == [4, 7]
    with pytest.raises(RuntimeError, match="does not hold"):
        st.pieces(3, 5)
    st.drop_before(12)
    assert st.frames_held == 0 and st.chunks == []
    with pytest.raises(ValueError, match="one video's surfaces are of one kind"):
        st.add(12, YuvFrames.empty(1, 4, 6, full_range=True))
    # a chunk that may be the caller's memory is copied by own(); an owned one is left alone
    st, mine, theirs = FrameStore(), YuvFrames.empty(2, 4, 6), YuvFrames.empty(2, 4, 6)
    theirs.y.fill_(1), theirs.uv.fill_(2)
    st.add(0, mine, owned=True)
    st.add(2, theirs, owned=False)
    st.own()
    assert st.chunks[0][1] is mine and st.chunks[1][1] is not theirs and st.chunks[1][1].meta() == theirs.meta()
    theirs.y.zero_(), theirs.uv.zero_()                               # the caller refills its buffers
    got = st.pieces(2, 4)[0][0]
    assert bool((got.y == 1).all()) and bool((got.uv == 2).all())
