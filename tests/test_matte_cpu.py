"""What can be said about the soft matte and the compositing painter without a GPU: the two forms of the reference agree, the margin the
bit-certain GPU test rests on, render.Style's replace fields (validation, every refusal, the action and take tables in both modes with
and without classes, nothing changed for the existing styles), the bound signatures against the header, the entry points' argument
checks (made before any pointer is looked at, so NULL pointers get that far on any host) and the wrappers' shape and dtype checks."""
import dataclasses
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

import _matte_ref as REF  # noqa: E402


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def test_the_two_forms_of_the_matte_reference_agree():
    rng = np.random.default_rng(0)
    for k, gain in ((3, 1.0), (1, 0.37), (4, 4.0), (0, 1.0)):
        lg = torch.from_numpy(rng.normal(size=(k, 2, 4, 6)).astype(np.float32) * 4)
        if k:
            lg[0, 0, :2] = torch.tensor([1.0, -1.0, 2.0, -2.0, 3.0, -3.0])            # blends that give exactly 0
        v, bits = REF.oracle_values(lg, 14, 22, 9, 13)
        assert v.shape == (k, 2, 9, 13) and v.dtype == np.float64
        plane, level, vmax = REF.matte(v, bits, gain)
        assert plane.dtype == np.uint8 and np.array_equal(plane, REF.matte_pixelwise(v, bits, gain))
        if k:
            assert np.array_equal(plane >= 128, bits.any(0)) and np.array_equal(bits, v > 0)
        else:
            assert not plane.any()
    # U, not the rounded level, decides the side of 128: a level of 127.6 without a bit stays 127, one of 127.4 with a bit becomes 128
    v = np.array([[[[0.0010]]], [[[-0.5]]]])
    assert REF.matte(v, np.array([[[[False]]], [[[False]]]]), 1.0)[0].item() == 127
    v[0] = -0.0010
    assert REF.matte(v, np.array([[[[True]]], [[[False]]]]), 1.0)[0].item() == 128


def test_integer_logits_stay_clear_of_rounding_ties():
    """What the bit-certain GPU cases rest on: 255 * sigmoid(gain * k / 16) for k = -48..48, k != 0, is at least 3.3e-3 levels from a
    half-integer for the gains used there (8.68e-3 at gain 4), some fifty times the fp32 path's error."""
    worst = {}
    for gain in (0.5, 1.0, 2.0, 4.0):
        d = [abs(255.0 / (1.0 + math.exp(-gain * k / 16.0)) % 1.0 - 0.5) for k in range(-48, 49) if k != 0]
        worst[gain] = min(d)
    assert min(worst.values()) >= 3.3e-3 and worst[4.0] >= 8.6e-3, worst


def test_mix_is_exact_at_the_ends_and_has_no_ties():
    s, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64))
    assert np.array_equal(REF.mix(s, b, 255), s) and np.array_equal(REF.mix(s, b, 0), b)
    for w in (1, 77, 128, 254):
        exact = (s * w + b * (255 - w)) / 255.0
        got = REF.mix(s, b, w)
        assert np.abs(got - exact).max() < 0.5 and ((exact % 1.0) != 0.5).all()
        assert (got >= np.minimum(s, b)).all() and (got <= np.maximum(s, b)).all()


def test_the_two_forms_of_the_painter_reference_agree():
    rng = np.random.default_rng(1)
    for (F, Ho, Wo, h0, w0), mode, contour, a256 in (((2, 5, 7, 5, 7), 0, 1, 128), ((1, 6, 8, 3, 5), 1, 2, 77), ((2, 4, 3, 9, 4), 0, 0, 256)):
        lab = rng.integers(0, 6, size=(F, Ho, Wo)).astype(np.uint8)
        fr = rng.integers(0, 256, size=(F, 3, h0, w0)).astype(np.uint8)
        pal = rng.integers(0, 256, size=(256, 3)).astype(np.uint8)
        act = np.array([4, 1, 0, 4, 1, 2] + [0] * 250, dtype=np.uint8)
        mat = REF.ramp_matte(F, Ho, Wo, seed=F)
        for back in (np.array([3, 200, 90], dtype=np.uint8), rng.integers(0, 256, size=(Ho, Wo, 3)).astype(np.uint8)):
            a = REF.replace_rgb(lab, fr, pal, act, mat, back, a256, contour, mode)
            assert a.dtype == np.uint8 and np.array_equal(a, REF.replace_rgb_pixelwise(lab, fr, pal, act, mat, back, a256, contour, mode))
        none = REF.replace_rgb(lab, None, pal, act, mat, back, a256, contour, mode)
        assert np.array_equal(none, REF.replace_rgb_pixelwise(lab, None, pal, act, mat, back, a256, contour, mode))
    # full weight keeps the base, none gives the backdrop
    full = np.full_like(mat, 255)
    kept = REF.replace_rgb(lab, fr, pal, np.zeros(256, dtype=np.uint8), full, back, 128, 1, 0)
    sy, sx = (np.arange(Ho) * h0) // Ho, (np.arange(Wo) * w0) // Wo
    assert np.array_equal(kept, np.moveaxis(fr[:, :, sy][:, :, :, sx], 1, -1))
    gone = REF.replace_rgb(lab, fr, pal, act, full, back, 128, 1, 1)
    assert np.array_equal(gone, np.broadcast_to(back, gone.shape))


# ---- the style -----------------------------------------------------------------------------------------------------------------------
def test_style_defaults_and_the_existing_tables_are_unchanged():
    from mdqe_cvpr2023_amd.render import Style
    st = Style()
    assert (st.replace, st.backdrop, st.matte_gain) == (None, (0, 255, 0), 1.0)
    assert [f.name for f in dataclasses.fields(Style)][:15] == ["alpha", "contour", "palette", "mosaic", "cell", "classes", "blur", "blur_radius",
                                                                 "box", "caption", "class_names", "text_scale", "min_area", "trail", "trail_width"]
    ones = [1] * 255
    assert st.actions().tolist() == [0] + ones
    assert Style(mosaic="background").actions().tolist() == [2] + ones and Style(mosaic="tracks").actions().tolist() == [0] + [2] * 255
    assert Style(blur="background").actions().tolist() == [3] + ones and Style(blur="tracks").actions().tolist() == [0] + [3] * 255
    cls = torch.tensor([[0.1, 0.9], [0.8, 0.2], [0.3, 0.7]])
    assert Style(mosaic="tracks", classes=[1]).actions(cls).tolist() == [0, 2, 1, 2] + [1] * 252
    assert Style(blur="tracks", classes=[0]).actions(cls).tolist() == [0, 1, 3, 1] + [1] * 252
    with pytest.raises(ValueError, match="classes selects the tracks"):
        Style(classes=[1])
    with pytest.raises(ValueError, match="classes selects the tracks"):
        Style(mosaic="background", classes=[1])
    with pytest.raises(ValueError, match="takes"):
        st.takes()


def test_replace_tables_in_both_modes_with_and_without_classes():
    from mdqe_cvpr2023_amd.render import Style
    ones = [1] * 255
    bg, tr = Style(replace="background"), Style(replace="tracks")
    assert bg.actions().tolist() == [4] + ones and bg.takes().tolist() == [0] + ones
    assert tr.actions().tolist() == [0] + [4] * 255 and tr.takes().tolist() == [0] + ones
    cls = torch.tensor([[0.1, 0.9], [0.8, 0.2], [0.3, 0.7], [0.5, 0.5]])               # first maxima: 1, 0, 1, 0 (a tie takes the first)
    v = Style(replace="background", classes=[1])
    assert v.actions(cls).tolist() == [4, 1, 4, 1, 4] + [4] * 251                      # the listed kept, the others and the labels above n go
    assert v.takes(cls).tolist() == [0, 1, 0, 1, 0] + [0] * 251
    t = Style(replace="tracks", classes=(1, 1, 7))
    assert t.classes == (1, 7)
    assert t.actions(cls).tolist() == [0, 4, 1, 4, 1] + [1] * 251                      # as the mosaic with r = 4
    assert t.takes(cls).tolist() == [0, 1, 0, 1, 0] + [0] * 251
    for st in (v, t):
        with pytest.raises(ValueError, match="class rows"):
            st.actions()
        with pytest.raises(ValueError, match="class rows"):
            st.takes()
    empty = torch.zeros(0, 2)
    assert v.actions(empty).tolist() == [4] * 256 and not v.takes(empty).any()
    assert t.actions(empty).tolist() == [0] + ones and not t.takes(empty).any()
    # cached per device without classes, built per window with them
    assert bg.takes_on("cpu") is bg.takes_on("cpu") and bg.actions_on("cpu") is bg.actions_on("cpu")
    assert v.takes_on("cpu", cls) is not v.takes_on("cpu", cls) and v.takes_on("cpu", cls).tolist() == v.takes(cls).tolist()


def test_replace_validation_and_every_refusal():
    from mdqe_cvpr2023_amd.render import Style
    for bad in ("both", "foreground", True, 1):
        with pytest.raises(ValueError, match="replace must be None, 'tracks' or 'background'"):
            Style(replace=bad)
    for kw in ({"mosaic": "tracks"}, {"blur": "background"}):
        with pytest.raises(ValueError, match="at most one of mosaic, blur and replace"):
            Style(replace="tracks", **kw)
    for bad in (0, 0.0, -1.0, 64.5, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match=r"matte_gain must be a number in \(0, 64\]"):
            Style(replace="tracks", matte_gain=bad)
    assert Style(matte_gain=64).matte_gain == 64 and Style(matte_gain=1e-3).matte_gain == 1e-3
    for bad in ((0, 255), (0, 255, 256), (0, -1, 0), (0.5, 1, 2), "green", None, (True, 0, 0), 7):
        with pytest.raises(ValueError, match="backdrop must be three ints"):
            Style(backdrop=bad)
    for bad in (torch.zeros(4, 5, 3), torch.zeros(3, 4, 5, dtype=torch.uint8), torch.zeros(4, 5, dtype=torch.uint8),
                torch.zeros(0, 5, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="backdrop picture must be a uint8 tensor"):
            Style(backdrop=bad)
    assert Style(backdrop=[1, 2, 3]).backdrop == (1, 2, 3)
    st = Style(replace="background", backdrop=(9, 8, 7))
    b = st.backdrop_on("cpu")
    assert b.dtype == torch.uint8 and b.tolist() == [9, 8, 7] and st.backdrop_on("cpu") is b
    pic = torch.arange(4 * 5 * 3, dtype=torch.uint8).view(4, 5, 3)
    st = Style(replace="tracks", backdrop=pic.permute(1, 0, 2))
    assert st.backdrop_on("cpu").is_contiguous() and torch.equal(st.backdrop_on("cpu"), pic.permute(1, 0, 2))


def test_what_the_merger_refuses_names_the_remedy():
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.render import Style
    pic = torch.zeros(90, 150, 3, dtype=torch.uint8)
    merge.check_replace(Style(replace="background", backdrop=pic), (90, 150), False)
    merge.check_replace(Style(replace="tracks"), (61, 97), False)
    with pytest.raises(ValueError, match="resize the picture to the output's size"):
        merge.check_replace(Style(replace="background", backdrop=pic), (150, 90), False)
    merge.check_replace(Style(replace="tracks"), (90, 150), True)                   # a colour goes with either kind of session
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    surf = Style(replace="background", backdrop=YuvFrames.empty(1, 90, 150))
    merge.check_replace(surf, (90, 150), "nv12")
    with pytest.raises(ValueError, match="surface=True"):                            # a surface backdrop in an RGB session
        merge.check_replace(surf, (90, 150), False)
    with pytest.raises(ValueError, match="surface=False"):                           # ... and the reverse
        merge.check_replace(Style(replace="background", backdrop=pic), (90, 150), True)
    with pytest.raises(ValueError, match="resize the picture"):
        merge.check_replace(surf, (92, 150), True)
    with pytest.raises(ValueError, match="session's format"):
        merge.check_replace(surf, (90, 150), "p010")
    with pytest.raises(ValueError, match="ONE surface"):
        Style(backdrop=YuvFrames.empty(2, 90, 150))


def test_matte_spec_validation():
    from mdqe_cvpr2023_amd.render import Matte
    m = Matte()
    assert (m.classes, m.gain) == (None, 1.0) and m.takes() is None and m.takes(torch.zeros(3, 2)) is None
    for bad in (0, -1.0, 64.5, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match=r"gain must be a number in \(0, 64\]"):
            Matte(gain=bad)
    for bad in ("person", [1.5], [-1], [True], 3):
        with pytest.raises(ValueError, match="classes must be None or a collection of ints"):
            Matte(classes=bad)
    m = Matte(classes=[7, 1, 1], gain=64)
    assert m.classes == (1, 7) and m == Matte(classes=(1, 7), gain=64)
    cls = torch.tensor([[0.1, 0.9], [0.8, 0.2], [0.3, 0.7], [0.5, 0.5]])
    assert m.takes(cls).tolist() == [0, 1, 0, 1, 0] + [0] * 251 and m.takes(cls).dtype == torch.uint8
    assert not m.takes(torch.zeros(0, 2)).any()
    with pytest.raises(ValueError, match="class rows"):
        m.takes()
    with pytest.raises(dataclasses.FrozenInstanceError):
        m.gain = 2.0


def test_matte_output_is_a_form_of_its_own():
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.online import Window
    from mdqe_cvpr2023_amd.render import Matte
    assert [f.name for f in dataclasses.fields(Forms)][-1] == "matte" and Forms().matte is False

    class M:
        matte_output = Matte()
    assert Forms.of_model(M()) == Forms(planes="dense", matte=True)
    assert Forms.of_emit("rle", matte=True) == Forms(planes="rle", matte=True) and Forms.of_emit("rle") == Forms(planes="rle")
    w = Window(frames=(0, 2), track_ids=[], cls_probs=torch.zeros(0, 2), matte=torch.zeros(2, 3, 4, dtype=torch.uint8))
    assert tuple(w.matte.shape) == (2, 3, 4) and Window(frames=(0, 2), track_ids=[], cls_probs=None).matte is None


def test_window_fields_and_the_default_forms_are_unchanged():
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.online import Window
    assert [f.name for f in dataclasses.fields(Window)] == ["frames", "track_ids", "cls_probs", "masks", "rles", "boxes", "areas"]

    class M:
        pass
    assert Forms.of_model(M()) == Forms(planes="dense")


# ---- the ABI and the wrappers ----------------------------------------------------------------------------------------------------------
def _lib_and_header():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib, _lib.load_library(), src


def test_abi_declares_and_exports_the_entries_and_they_refuse_bad_arguments():
    _lib, h, src = _lib_and_header()
    for name, n_args in (("mdqe_final_matte_u8", 16), ("mdqe_render_replace_u8", 20), ("mdqe_render_replace_yuv420sp", 30)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
        assert hasattr(h, name) and name in _lib.SIGNATURES
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == n_args
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # new entries only
    assert h.mdqe_version() >= 101
    EINVAL, ENULL = 1, 3

    def matte(n_sel=2, Fw=1, Hm=4, Wm=6, factor=4, h_=16, w=24, Ho=16, Wo=24, gain=1.0, f_off=0):
        return h.mdqe_final_matte_u8(None, n_sel, None, Fw, Hm, Wm, factor, h_, w, Ho, Wo, None, gain, None, f_off, None)
    for kw in ({"n_sel": 256}, {"n_sel": -1}, {"gain": 0.0}, {"gain": -1.0}, {"gain": 64.5}, {"gain": float("nan")}, {"gain": float("inf")},
               {"f_off": -1}, {"Ho": 0}, {"h_": 17}, {"Ho": 1 << 16, "Wo": 1 << 15}, {"factor": 0}):
        assert matte(**kw) == EINVAL, kw
        assert matte(**dict(kw, Fw=0)) == EINVAL, kw                                              # ... whatever Fw says
    assert matte(Fw=0) == 0 and matte(Fw=0, gain=64.0) == 0                                       # Fw = 0: OK, nothing launched
    assert matte() == ENULL and matte(n_sel=0) == ENULL                                           # (n_sel = 0 still writes zeros: it needs `out`)

    def rgb(F=1, Ho=8, Wo=8, a256=128, contour=1, picture=0, mode=0, f_off=0):
        return h.mdqe_render_replace_u8(None, 1, 0, 0, 0, None, F, Ho, Wo, None, None, a256, contour, None, None, picture, mode, None, f_off, None)
    for kw in ({"mode": 2}, {"mode": -1}, {"picture": 2}, {"contour": 4}, {"a256": 257}, {"F": -1}, {"f_off": -1}, {"Ho": 0}):
        assert rgb(**kw) == EINVAL, kw
        if "F" not in kw:
            assert rgb(**dict(kw, F=0)) == EINVAL, kw
    assert rgb(F=0) == 0 and rgb(F=0, mode=1, picture=1) == 0
    assert rgb() == ENULL


def test_the_wrappers_check_shapes_and_dtypes_before_devices():
    from mdqe_cvpr2023_amd import ops, render
    lab = torch.zeros(2, 6, 9, dtype=torch.uint8)
    out = torch.zeros(2, 6, 9, 3, dtype=torch.uint8)
    rgb, act = render.default_palette(), render.Style(replace="background").actions()
    col = torch.tensor([1, 2, 3], dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="mode must be"):
        ops.render_replace(lab, None, rgb, act, lab, col, out, mode=0)
    with pytest.raises(RuntimeError, match="labels must be contiguous uint8"):
        ops.render_replace(lab.float(), None, rgb, act, lab, col, out)
    with pytest.raises(RuntimeError, match="action must be contiguous uint8"):
        ops.render_replace(lab, None, rgb, act[:255], lab, col, out)
    for bad in (lab[:1], lab.float(), torch.zeros(2, 6, 8, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="matte must be contiguous uint8"):
            ops.render_replace(lab, None, rgb, act, bad, col, out)
    for bad in (col[:2], col.float(), torch.zeros(6, 9, 4, dtype=torch.uint8), torch.zeros(9, 6, 3, dtype=torch.uint8), (1, 2, 3)):
        with pytest.raises(RuntimeError, match="backdrop must be contiguous uint8"):
            ops.render_replace(lab, None, rgb, act, lab, bad, out)
    with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
        ops.render_replace(lab, None, rgb, act, lab, col, out[:1])
    with pytest.raises(RuntimeError, match="must be a CUDA tensor on out's device"):
        ops.render_replace(lab, None, rgb, act, lab, col, out)
    lg, idx = torch.zeros(2, 1, 4, 6), torch.arange(2, dtype=torch.int32)
    plane = torch.zeros(1, 16, 24, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="logits must be"):
        ops.final_matte(torch.zeros(256, 1, 4, 6), idx, 4, 16, 24, 16, 24, plane, 0)
    with pytest.raises(RuntimeError, match="inst_idx must be int32"):
        ops.final_matte(lg, idx.long(), 4, 16, 24, 16, 24, plane, 0)
    with pytest.raises(RuntimeError, match="gain must be a finite number"):
        ops.final_matte(lg, idx, 4, 16, 24, 16, 24, plane, 0, None, 0.0)
    with pytest.raises(RuntimeError, match="take must be contiguous uint8"):
        ops.final_matte(lg, idx, 4, 16, 24, 16, 24, plane, 0, torch.zeros(256))
    with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
        ops.final_matte(lg, idx, 4, 16, 24, 16, 24, plane, 1)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.final_matte(lg, idx, 4, 16, 24, 16, 24, plane, 0)


# ---- surfaces --------------------------------------------------------------------------------------------------------------------------
def test_backdrop_yuv_of_a_grey_is_exactly_neutral():
    from mdqe_cvpr2023_amd import render
    for fmt, mid in (("nv12", 128), ("p010", 512)):
        for matrix in ("bt601", "bt709"):
            for full in (False, True):
                for g in (0, 1, 77, 128, 254, 255):
                    b = render.backdrop_yuv((g, g, g), fmt, matrix, full, "rgb")
                    assert b.dtype == torch.uint16 and tuple(b.shape) == (3,) and b.view(torch.int16).tolist()[1:] == [mid, mid], (fmt, matrix, full, g)
    pal = torch.zeros(256, 3, dtype=torch.uint8)
    pal[0] = torch.tensor([10, 200, 30], dtype=torch.uint8)
    for order in ("rgb", "bgr"):
        want = render.palette_yuv(pal, "p010", "bt601", True, order)[0].view(torch.int16).tolist()
        assert render.backdrop_yuv((10, 200, 30), "p010", "bt601", True, order).view(torch.int16).tolist() == want
    with pytest.raises(ValueError, match="three ints"):
        render.backdrop_yuv((1, 2))
    st = render.Style(replace="tracks", backdrop=(5, 5, 5))
    assert st.backdrop_yuv_on("cpu", "nv12", "bt709", False, "rgb") is st.backdrop_yuv_on("cpu", "nv12", "bt709", False, "rgb")


def _surfaces(rng, n, H, W, fmt, pitch_align):
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    s = YuvFrames.empty(n, H, W, fmt=fmt, pitch_align=pitch_align)
    cw = 2 * ((W + 1) // 2)
    if fmt == "nv12":
        s.y[:, :, :W] = torch.from_numpy(rng.integers(0, 256, size=(n, H, W)).astype(np.uint8))
        s.uv[:, :, :cw] = torch.from_numpy(rng.integers(0, 256, size=(n, (H + 1) // 2, cw)).astype(np.uint8))
    else:                                                             # 10-bit values with low bits set: what a copied word must keep
        for t, shape in ((s.y, (n, H, W)), (s.uv, (n, (H + 1) // 2, cw))):
            words = (rng.integers(0, 1024, size=shape) << 6 | rng.integers(0, 64, size=shape)).astype(np.uint16)
            t[:, :, :shape[2]] = torch.from_numpy(words.view(np.int16))
    return s


def _stored(t, fmt, cols):
    a = t[:, :, :cols].numpy()
    return a.view(np.uint16) if fmt == "p010" else a


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(5, 7), (6, 8)])
def test_host_path_of_render_replace_yuv_against_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops, render
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    rng = np.random.default_rng(H * 10 + W)
    F, cw = 2, 2 * ((W + 1) // 2)
    src = _surfaces(rng, F, H, W, fmt, 64)                            # padded pitch
    back = _surfaces(rng, 1, H, W, fmt, 32)
    assert src.y.shape[2] > W
    lab = rng.integers(0, 5, size=(F, H, W)).astype(np.uint8)
    mat = REF.ramp_matte(F, H, W, seed=W)
    mat[1, :2, :2] = 255
    lab[1, :2, :2] = 0                                                # a whole block kept at full weight
    pal = torch.from_numpy(rng.integers(0, 1024 if fmt == "p010" else 256, size=(256, 3)).astype(np.uint16).view(np.int16)).view(torch.uint16)
    pal_np = pal.view(torch.int16).numpy().astype(np.int64) & 0xFFFF
    act = np.array([0, 1, 4, 1, 2] + [0] * 251, dtype=np.uint8)
    colour = render.backdrop_yuv((200, 30, 90), fmt)
    ys, cs = _stored(src.y, fmt, W), _stored(src.uv, fmt, cw)
    k = 0
    for mode in (0, 1):
        for b_dev, b_ref in ((colour, tuple(colour.view(torch.int16).tolist())), (back, (_stored(back.y, fmt, W)[0], _stored(back.uv, fmt, cw)[0]))):
            for contour, a256 in ((0, 128), (2, 77)):
                wy, wc = REF.replace_yuv(ys, cs, lab, pal_np, act, mat, b_ref, fmt, a256, contour, mode)
                py, pc = REF.replace_yuv_pixelwise(ys, cs, lab, pal_np, act, mat, b_ref, fmt, a256, contour, mode)
                assert np.array_equal(wy, py) and np.array_equal(wc, pc)                       # the two forms of the reference
                out = YuvFrames.empty(F + 1, H, W, fmt=fmt, pitch_align=48)
                out.y.fill_(0x55); out.uv.fill_(0x55)
                got = ops.render_replace_yuv(torch.from_numpy(lab), src, pal, torch.from_numpy(act), torch.from_numpy(mat), b_dev, out, 1,
                                             a256, contour, ops.REPLACE_MODES[mode])
                assert got is out
                assert np.array_equal(_stored(out.y[1:], fmt, W), wy) and np.array_equal(_stored(out.uv[1:], fmt, cw), wc), (mode, k)
                assert bool((out.y[0] == 0x55).all()) and bool((out.y[1:, :, W:] == 0x55).all())   # the guard surface and the padding
                if k % 3 == 0:                                        # in place: the same samples
                    own = src.clone()
                    ops.render_replace_yuv(torch.from_numpy(lab), own, pal, torch.from_numpy(act), torch.from_numpy(mat), b_dev, own, 0,
                                           a256, contour, ops.REPLACE_MODES[mode])
                    assert np.array_equal(_stored(own.y, fmt, W), wy) and np.array_equal(_stored(own.uv, fmt, cw), wc)
                if fmt == "p010":                                     # copied words keep their low bits, rewritten ones lose them
                    wt = 255 - mat.astype(np.int64) if mode else mat.astype(np.int64)
                    kept = (act[lab] != 1) & (wt == 255)
                    assert kept.any() and np.array_equal(wy[kept], ys[kept]) and (wy[~kept] & 0x3F == 0).all()
                    assert (wc[1, 0, :2] == cs[1, 0, :2]).all() or mode == 1
                k += 1
    assert k == 8
    # shapes and dtypes are refused before devices
    with pytest.raises(RuntimeError, match="matte must be contiguous uint8"):
        ops.render_replace_yuv(torch.from_numpy(lab), src, pal, torch.from_numpy(act), torch.from_numpy(mat[:1]), colour)
    with pytest.raises(RuntimeError, match="backdrop"):
        ops.render_replace_yuv(torch.from_numpy(lab), src, pal, torch.from_numpy(act), torch.from_numpy(mat), _surfaces(rng, 1, H + 1, W, fmt, 2))
    with pytest.raises(RuntimeError, match="backdrop"):
        ops.render_replace_yuv(torch.from_numpy(lab), src, pal, torch.from_numpy(act), torch.from_numpy(mat), torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="mode"):
        ops.render_replace_yuv(torch.from_numpy(lab), src, pal, torch.from_numpy(act), torch.from_numpy(mat), colour, mode=1)
