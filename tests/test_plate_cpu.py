"""Object removal, the host side: the numpy forms of the background plate's rule (tests/_plate_ref.py) against each other and against known
answers; the input generators' own guarantees; render.Style's plate fields and every refusal; merge.check_replace on plate_init; the ABI
entries' refusals, called through the library; the ops wrappers' argument checks; and the launches merge.overlay_frames makes, with the
ops replaced by recorders.  Integers only: every comparison is exact.  No GPU."""
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

import _plate_ref as REF  # noqa: E402

ENTRIES = {"mdqe_plate_update_u8": 12, "mdqe_plate_update_yuv420sp": 15, "mdqe_plate_picture_u8": 7, "mdqe_plate_picture_yuv420sp": 12}


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 3), (7, 40), (19, 70)])
def test_the_two_reference_forms_agree(size):
    h, w = size
    rng = np.random.default_rng(h * 100 + w)
    for reach in (0, 1, 2, 5, 9, 32):
        for p in (0.0, 0.01, 0.1, 0.5, 1.0):
            n = (rng.random((h, w)) < p).astype(np.int64) * rng.integers(1, 9, size=(h, w))
            a, b = REF.sources(n, reach), REF.sources_pixelwise(n, reach)
            assert np.array_equal(a, b), (size, reach, p)
            seen = n > 0
            assert np.array_equal(a[seen], np.argwhere(seen))         # a seen cell shows itself
            if reach == 0:
                assert (a[~seen] == -1).all()


def test_known_answers():
    # the update: the first observation sets P, then a rounded cumulative mean, then an exponential one; floordiv, not truncation
    P, n = REF.fresh(1, 1, 1)
    seq, want = [10, 11, 11, 0, 255], []
    for s in seq:
        P, n = REF.update(P, n, np.full((1, 1, 1, 1), s), np.ones((1, 1, 1), bool), 3)
        want.append((int(P[0, 0, 0]), int(n[0, 0])))
    # n' = 1: 2560; n' = 2: d = 256, (256 + 1) // 2 = 128 -> 2688; n' = 3: d = 128, (128 + 1) // 3 = 43 -> 2731;
    # n' = 3: d = -2731, (-2731 + 1) // 3 = -910 (truncation: -910 too; next) -> 1821; d = 65280 - 1821 = 63459, (63459 + 1) // 3 = 21153 -> 22974
    assert want == [(2560, 1), (2688, 2), (2731, 3), (1821, 3), (22974, 3)]
    P, n = REF.update(np.full((1, 1, 1), 1000), np.full((1, 1), 3), np.full((1, 1, 1, 1), 0), np.ones((1, 1, 1), bool), 3)
    assert int(P[0, 0, 0]) == 1000 + (-999 // 3) == 667               # (-1000 + 1) / 3 = -333 exactly; truncation would agree here ...
    P, n = REF.update(np.full((1, 1, 1), 1001), np.full((1, 1), 3), np.full((1, 1, 1, 1), 0), np.ones((1, 1, 1), bool), 3)
    assert int(P[0, 0, 0]) == 1001 - 334 == 667                       # ... and not here: floor(-1000 / 3) = -334, truncation gives -333
    # a background that does not change is reproduced exactly, whatever N; a blocked frame changes nothing
    for N in (1, 2, 64, 256):
        P, n = REF.fresh(2, 2, 3)
        s = np.broadcast_to(np.array([7, 0, 255]), (9, 2, 2, 3))
        obs = np.ones((9, 2, 2), bool)
        obs[3:5, 0, 0] = False
        P, n = REF.update(P, n, s, obs, N)
        assert (P == 256 * s[0]).all() and int(n[0, 0]) == min(7, N) and int(n[1, 1]) == min(9, N)
    # a chroma pair sees its in-picture pixels only
    block = np.zeros((1, 3, 5), dtype=np.uint8)
    block[0, 2, 4], block[0, 0, 1] = 1, 9
    assert REF.observed_chroma(block)[0].tolist() == [[False, True, True], [True, True, False]]
    # the picture: the nearest seen cell, of equally near ones the smallest Y', then the smallest X'; the disc is Euclidean
    n = np.zeros((9, 9), dtype=np.int64)
    n[4, 1], n[4, 7], n[1, 4], n[7, 4] = 1, 1, 1, 1
    for fn in (REF.sources, REF.sources_pixelwise):
        src = fn(n, 3)
        assert src[4, 4].tolist() == [1, 4]                          # four at distance 3: the smallest Y'
        n2 = n.copy()
        n2[1, 4] = 0
        assert fn(n2, 3)[4, 4].tolist() == [4, 1]                     # (4, 1), (4, 7), (7, 4): Y' = 4 twice, the smaller X'
        assert fn(n, 2)[4, 4].tolist() == [-1, -1]                    # beyond reach
        far = np.zeros((9, 9), dtype=np.int64)
        far[0, 0] = 1
        assert fn(far, 5)[3, 4].tolist() == [0, 0] and fn(far, 5)[4, 4].tolist() == [-1, -1]      # 9 + 16 = 25 <= 25 < 32
    P = np.arange(81 * 2).reshape(9, 9, 2) * 100
    pic = REF.picture(P, n, 3, (5, 6))
    assert pic[4, 4].tolist() == ((P[1, 4] + 128) >> 8).tolist() and pic[0, 0].tolist() == [5, 6] and pic[4, 1].tolist() == ((P[4, 1] + 128) >> 8).tolist()
    assert REF.from_picture(np.full((2, 2, 3), 9))[0].tolist() == np.full((2, 2, 3), 2304).tolist()
    st = REF.to_state(*REF.from_picture(np.full((2, 3, 2), 9)))
    assert st.dtype == np.int32 and st.shape == (2, 3, 4) and st[0, 0].tolist() == [2304, 2304, 1, 0]
    assert REF.to_state(*REF.from_picture(np.full((2, 3, 1), 9)))[1, 2].tolist() == [2304, 1]


def test_generated_inputs_can_go_wrong():
    """The generators assert their own guarantees (REF.check_update_case, REF.picture_cases); here they run for every shape the GPU tests use,
    and the guarantees are shown to have teeth: truncation instead of floor, and a forgotten saturation, change the result."""
    for h, w in ((19, 70), (37, 150)):
        for N in (1, 2, 3, 64):
            for C, top in ((3, 255), (1, 1023), (2, 255)):
                s, block = REF.update_case(h * w + N, 5, h, w, C, top, N)
                obs = block == 0
                P, n = REF.update(*REF.fresh(h, w, C), s, obs, N)
                if N > 1:                                             # truncation towards zero differs somewhere
                    Q, m = REF.fresh(h, w, C)
                    for f in range(5):
                        n1 = np.minimum(m + 1, N)
                        num = 256 * s[f] - Q + (n1 >> 1)[..., None]
                        Q = np.where(obs[f][..., None], Q + (np.sign(num) * (np.abs(num) // n1[..., None])), Q)
                        m = np.where(obs[f], n1, m)
                    assert not np.array_equal(P, Q)
                if N < 5:                                             # a count that does not saturate differs somewhere
                    assert not np.array_equal(P, REF.update(*REF.fresh(h, w, C), s, obs, 256)[0])
        for C, top, (ph, pw) in ((3, 255, (h, w)), (1, 1023, (h, w)), (2, 255, ((h + 1) // 2, (w + 1) // 2))):
            cases = REF.picture_cases(h + w, ph, pw, C, top)
            assert set(cases) == {"seen everywhere", "holes", "random", "sparse", "nothing seen"}
            P, n = cases["holes"]
            assert not np.array_equal(REF.picture(P, n, 1, (1,) * C), REF.picture(P, n, 32, (1,) * C))
    blk = REF.moving_square(5, 19, 70)
    assert (blk != 0).sum(axis=(1, 2)).tolist() == [36] * 5 and (blk == 0).any(0).all() and not (blk == 0).all(0).all()


# ---- render.Style --------------------------------------------------------------------------------------------------------------------
def test_style_plate_fields_and_refusals():
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style
    st = Style(replace="tracks", backdrop="plate")
    assert st.plate and (st.plate_frames, st.plate_margin, st.plate_reach, st.plate_fill, st.plate_init) == (64, 4, 16, (128, 128, 128), None)
    assert not Style().plate and not Style(replace="tracks").plate and not Style(replace="tracks", backdrop=(1, 2, 3)).plate
    assert Style().plate_frames == 64 and Style() == Style(plate_frames=64, plate_margin=4, plate_reach=16, plate_fill=(128, 128, 128))
    for what in ("background", None):
        with pytest.raises(ValueError, match="(?s)backdrop='plate'.*replace='tracks'"):
            Style(replace=what, backdrop="plate")
    with pytest.raises(ValueError, match="backdrop must be three ints"):
        Style(replace="tracks", backdrop="scene")
    for k, lo, hi in (("plate_frames", 1, 256), ("plate_margin", 0, 32), ("plate_reach", 0, 32)):
        for bad in (lo - 1, hi + 1, 4.0, True, None, "4"):
            with pytest.raises(ValueError, match="%s is .* an int in %d..%d" % (k, lo, hi)):
                Style(replace="tracks", backdrop="plate", **{k: bad})
        for ok in (lo, hi):
            assert getattr(Style(replace="tracks", backdrop="plate", **{k: ok}), k) == ok
    for bad in ((1, 2), (1, 2, 256), (1, 2, -1), (1.0, 2, 3), (True, 2, 3), "abc", 7, None, torch.zeros(3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="plate_fill must be three ints 0..255"):
            Style(replace="tracks", backdrop="plate", plate_fill=bad)
    assert Style(replace="tracks", backdrop="plate", plate_fill=[0, 255, 9]).plate_fill == (0, 255, 9)
    with pytest.raises(ValueError, match="(?s)grow.*matte_gain"):       # the margin of the other redactions stays refused with replace
        Style(replace="tracks", backdrop="plate", grow=2)
    # plate_init
    pic = torch.zeros(6, 8, 3, dtype=torch.uint8)
    assert Style(replace="tracks", backdrop="plate", plate_init=pic).plate_init is pic
    surf = YuvFrames.empty(1, 6, 8, fmt="nv12")
    assert Style(replace="tracks", backdrop="plate", plate_init=surf).plate_init is surf
    with pytest.raises(ValueError, match="(?s)plate_init.*backdrop='plate'"):
        Style(replace="tracks", plate_init=pic)
    for bad in (pic.float(), pic[0], torch.zeros(6, 8, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="plate_init: a backdrop picture must be a uint8 tensor .Ho, Wo, 3."):
            Style(replace="tracks", backdrop="plate", plate_init=bad)
    with pytest.raises(ValueError, match="plate_init: a backdrop surface must be a YuvFrames of ONE surface"):
        Style(replace="tracks", backdrop="plate", plate_init=YuvFrames.empty(2, 6, 8, fmt="nv12"))
    for bad in ((1, 2, 3), "shot.png", 5):
        with pytest.raises(ValueError, match="plate_init must be None, a uint8 tensor"):
            Style(replace="tracks", backdrop="plate", plate_init=bad)
    # the device tables, cached per device
    st = Style(replace="tracks", backdrop="plate", plate_fill=(1, 2, 3), plate_init=pic)
    assert st.plate_fill_on("cpu") is st.plate_fill_on("cpu") and st.plate_fill_on("cpu").tolist() == [1, 2, 3]
    assert st.plate_fill_on("cpu").dtype == torch.uint8 and st.plate_init_on("cpu") is st.plate_init_on("cpu")
    from mdqe_cvpr2023_amd.render import backdrop_yuv
    for kind in (("nv12", "bt601", True, "bgr"), ("p010", "bt709", False, "rgb")):
        f = st.plate_fill_yuv_on("cpu", *kind)
        assert f is st.plate_fill_yuv_on("cpu", *kind) and torch.equal(f, backdrop_yuv((1, 2, 3), *kind))
    # the matte's tables are those of replace="tracks" on a colour
    ref = Style(replace="tracks")
    assert torch.equal(st.actions(), ref.actions()) and torch.equal(st.takes(), ref.takes())


def test_check_replace_checks_plate_init_as_a_backdrop_picture():
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style
    mk = lambda init=None: Style(replace="tracks", backdrop="plate", plate_init=init)      # noqa: E731
    for surface in (False, True, "nv12", "p010"):
        merge.check_replace(mk(), (6, 8), surface)
    pic = torch.zeros(6, 8, 3, dtype=torch.uint8)
    merge.check_replace(mk(pic), (6, 8), False)
    with pytest.raises(ValueError, match="(?s)plate_init picture is 6 x 8 but the output is 6 x 10; resize"):
        merge.check_replace(mk(pic), (6, 10), False)
    with pytest.raises(ValueError, match="(?s)plate_init is an RGB picture but the session paints decoder surfaces.*YuvFrames"):
        merge.check_replace(mk(pic), (6, 8), True)
    surf = YuvFrames.empty(1, 6, 8, fmt="nv12")
    merge.check_replace(mk(surf), (6, 8), True)
    merge.check_replace(mk(surf), (6, 8), "nv12")
    with pytest.raises(ValueError, match="(?s)plate_init is a YuvFrames surface but the session paints RGB pictures.*surface=True"):
        merge.check_replace(mk(surf), (6, 8), False)
    with pytest.raises(ValueError, match="(?s)plate_init surface is 6 x 8 nv12 but the output is 8 x 8"):
        merge.check_replace(mk(surf), (8, 8), True)
    with pytest.raises(ValueError, match="(?s)plate_init surface is 6 x 8 nv12 but the output is 6 x 8 p010.*convert"):
        merge.check_replace(mk(surf), (6, 8), "p010")


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def _library():
    from mdqe_cvpr2023_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load_library()


def test_abi_declares_and_exports_the_four_entries():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    h = _library()
    for name, argc in ENTRIES.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
        assert hasattr(h, name) and name in _lib.SIGNATURES
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == argc, name
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # new entries only
    assert os.path.exists(os.path.join(ROOT, "mdqe_cvpr2023_amd", "csrc", "plate.hip"))


def test_entries_refuse_bad_arguments_before_any_pointer_is_looked_at():
    h = _library()
    EINVAL, M = 1, 1 << 24
    A = {"frames": 1 * M, "block": 2 * M, "plate": 3 * M, "fill": 4 * M, "out": 5 * M, "y": 6 * M, "uv": 7 * M, "plate_c": 8 * M, "out_uv": 9 * M}

    def upd(F=2, Ho=8, Wo=8, N=64, h0=8, w0=8, stride=None, is_u8=1, **p):
        p = dict({k: A[k] for k in ("frames", "block", "plate")}, **p)
        return h.mdqe_plate_update_u8(p["frames"], is_u8, 3 * h0 * w0 if stride is None else stride, h0, w0, p["block"], F, Ho, Wo, N, p["plate"], None)

    def pic(Ho=8, Wo=8, reach=4, **p):
        p = dict({k: A[k] for k in ("plate", "fill", "out")}, **p)
        return h.mdqe_plate_picture_u8(p["plate"], Ho, Wo, reach, p["fill"], p["out"], None)

    def updy(F=2, H=7, W=9, fmt=0, N=64, yp=16, ys=256, cp=16, cs=256, **p):
        p = dict({k: A[k] for k in ("y", "uv", "block", "plate", "plate_c")}, **p)
        return h.mdqe_plate_update_yuv420sp(p["y"], yp, ys, p["uv"], cp, cs, F, H, W, fmt, p["block"], N, p["plate"], p["plate_c"], None)

    def picy(H=7, W=9, fmt=0, reach=4, yp=16, cp=16, **p):
        p = dict({k: A[k] for k in ("plate", "plate_c", "fill", "out", "out_uv")}, **p)
        return h.mdqe_plate_picture_yuv420sp(p["plate"], p["plate_c"], H, W, fmt, reach, p["fill"], p["out"], yp, p["out_uv"], cp, None)
    # sizes and ranges: EINVAL with every pointer null, i.e. before any pointer is looked at
    null3 = {"frames": None, "block": None, "plate": None}
    for kw in ({"N": 0}, {"N": 257}, {"F": -1}, {"Ho": -1}, {"Wo": -1}, {"h0": 0}, {"w0": 0}, {"stride": 191}, {"Ho": 1 << 15, "Wo": 1 << 15},
               {"F": 1 << 12, "Ho": 1 << 10, "Wo": 1 << 10}):
        assert upd(**dict(kw, **null3)) == EINVAL, kw
    assert upd(F=0, **null3) == 0 and upd(Ho=0, **null3) == 0 and upd(Wo=0, **null3) == 0        # OK, nothing launched
    for kw in ({"reach": -1}, {"reach": 33}, {"Ho": -1}, {"Wo": -1}, {"Ho": 1 << 15, "Wo": 1 << 15}):
        assert pic(plate=None, fill=None, out=None, **kw) == EINVAL, kw
    assert pic(Ho=0, plate=None, fill=None, out=None) == 0 and pic(Wo=0, plate=None, fill=None, out=None) == 0
    nully = {"y": None, "uv": None, "block": None, "plate": None, "plate_c": None}
    for kw in ({"N": 0}, {"N": 257}, {"F": -1}, {"H": 0}, {"W": 0}, {"fmt": 2}, {"fmt": -1}, {"yp": 8}, {"cp": 9}, {"ys": -1}, {"cs": -1},
               {"fmt": 1, "yp": 19, "cp": 20}, {"fmt": 1, "yp": 20, "cp": 20, "ys": 255}, {"fmt": 1, "yp": 16, "cp": 20}):
        assert updy(**dict(kw, **nully)) == EINVAL, kw
    assert updy(F=0, **nully) == 0
    nullp = {"plate": None, "plate_c": None, "fill": None, "out": None, "out_uv": None}
    for kw in ({"reach": -1}, {"reach": 33}, {"H": 0}, {"W": 0}, {"fmt": 2}, {"yp": 8}, {"cp": 9}, {"fmt": 1, "yp": 19, "cp": 20}):
        assert picy(**dict(kw, **nullp)) == EINVAL, kw
    # with something to do: a missing pointer, a misaligned state, odd P010 planes, and any overlap of the state with an input or output
    for fn, keys in ((upd, ("frames", "block", "plate")), (pic, ("plate", "fill", "out")), (updy, ("y", "uv", "block", "plate", "plate_c")),
                     (picy, ("plate", "plate_c", "fill", "out", "out_uv"))):
        for missing in keys:
            assert fn(**{missing: None}) == EINVAL, (fn.__name__, missing)
        for k in [k for k in keys if k.startswith("plate")]:
            assert fn(**{k: A[k] + 4}) == EINVAL, (fn.__name__, k)
    assert updy(fmt=1, yp=20, cp=20, y=A["y"] + 1) == EINVAL and picy(fmt=1, yp=20, cp=20, out_uv=A["out_uv"] + 1) == EINVAL
    assert picy(fill=A["fill"] + 1) == EINVAL
    st = 8 * 8 * 16
    for kw in ({"frames": A["plate"]}, {"frames": A["plate"] + st - 1}, {"frames": A["plate"] - 2 * 192 + 1}, {"block": A["plate"] + st - 1},
               {"block": A["plate"] - 127}, {"plate": A["block"] + 112}):
        assert upd(**kw) == EINVAL, kw
    for kw in ({"out": A["plate"]}, {"out": A["plate"] + st - 1}, {"out": A["plate"] - 191}, {"fill": A["plate"] + 16}, {"fill": A["out"] + 191},
               {"plate": A["out"] + 176}):
        assert pic(**kw) == EINVAL, kw
    for kw in ({"y": A["plate"]}, {"uv": A["plate"] + 7 * 9 * 8 - 1}, {"block": A["plate_c"] + 4 * 5 * 16 - 1}, {"y": A["plate_c"] - 256 - 6 * 16 - 8},
               {"plate_c": A["plate"] + 496}, {"plate": A["uv"] + 304}):
        assert updy(**kw) == EINVAL, kw
    for kw in ({"out": A["plate"]}, {"out_uv": A["plate_c"] + 4 * 5 * 16 - 1}, {"out": A["plate_c"] - 6 * 16 - 8}, {"out_uv": A["out"] + 6 * 16 + 8},
               {"fill": A["plate_c"] + 2}, {"fill": A["out"] + 4}):
        assert picy(**kw) == EINVAL, kw


def test_wrapper_argument_checks():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    for name in ("plate_update", "plate_update_yuv", "plate_picture", "plate_picture_yuv"):
        assert callable(getattr(ops, name))
    plate = torch.zeros(6, 9, 4, dtype=torch.int32)
    frames = torch.zeros(2, 3, 5, 7, dtype=torch.uint8)
    block = torch.zeros(2, 6, 9, dtype=torch.uint8)
    fill = torch.zeros(3, dtype=torch.uint8)
    for bad in (plate.float(), plate[..., :3], torch.zeros(6, 9, 8, dtype=torch.int32)[..., ::2], plate[0], None, plate.numpy()):
        with pytest.raises(RuntimeError, match="plate_update: plate must be contiguous int32 .Ho, Wo, 4."):
            ops.plate_update(bad, frames, block)
        with pytest.raises(RuntimeError, match="plate_picture: plate must be contiguous int32 .Ho, Wo, 4."):
            ops.plate_picture(bad, fill)
    for bad in (frames.to(torch.int16), frames[0], frames[:, :2], None):
        with pytest.raises(RuntimeError, match="plate_update: frames must be uint8 or float32 .F, 3, h0, w0."):
            ops.plate_update(plate, bad, block)
    with pytest.raises(RuntimeError, match="plate_update: every frame must be contiguous"):
        ops.plate_update(plate, torch.zeros(2, 3, 5, 14, dtype=torch.uint8)[..., ::2], block)
    for bad in (block[:1], block.float(), torch.zeros(2, 6, 18, dtype=torch.uint8)[..., ::2], torch.zeros(2, 6, 8, dtype=torch.uint8), None):
        with pytest.raises(RuntimeError, match="plate_update: block must be contiguous uint8 .F = 2, 6, 9."):
            ops.plate_update(plate, frames, bad)
    for bad in (0, 257, 64.0, True, None):
        with pytest.raises(RuntimeError, match="plate_update: n_max must be an int in 1..256"):
            ops.plate_update(plate, frames, block, bad)
    for bad in (fill.float(), fill[:2], torch.zeros(6, dtype=torch.uint8)[::2], (1, 2, 3), None):
        with pytest.raises(RuntimeError, match="plate_picture: fill must be contiguous uint8 .3."):
            ops.plate_picture(plate, bad)
    for bad in (-1, 33, 4.0, True, None):
        with pytest.raises(RuntimeError, match="plate_picture: reach must be an int in 0..32"):
            ops.plate_picture(plate, fill, bad)
    for bad in (torch.zeros(6, 9, 4, dtype=torch.uint8), torch.zeros(6, 9, 3), torch.zeros(6, 9, 6, dtype=torch.uint8)[..., ::2], "x"):
        with pytest.raises(RuntimeError, match="plate_picture: out must be contiguous uint8"):
            ops.plate_picture(plate, fill, 4, bad)
    # shapes and dtypes first, devices after: a host without a GPU gets as far as the device check
    with pytest.raises(RuntimeError, match="plate_update: plate must be a CUDA tensor"):
        ops.plate_update(plate, frames, block)
    with pytest.raises(RuntimeError, match="plate_picture: plate must be a CUDA tensor"):
        ops.plate_picture(plate, fill, 4, torch.zeros(6, 9, 3, dtype=torch.uint8))
    # surfaces
    yuv = YuvFrames.empty(2, 7, 9, fmt="nv12")
    py, pc = torch.zeros(7, 9, 2, dtype=torch.int32), torch.zeros(4, 5, 4, dtype=torch.int32)
    blk = torch.zeros(2, 7, 9, dtype=torch.uint8)
    fy = torch.zeros(3, dtype=torch.int32).to(torch.uint16)
    with pytest.raises(RuntimeError, match="plate_update_yuv: yuv must be a preprocess.YuvFrames"):
        ops.plate_update_yuv(py, pc, torch.zeros(2, 3, 7, 9, dtype=torch.uint8), blk)
    for bad in (py.float(), torch.zeros(7, 9, 4, dtype=torch.int32), None):
        with pytest.raises(RuntimeError, match="plate_update_yuv: plate_y must be contiguous int32 .7, 9, 2."):
            ops.plate_update_yuv(bad, pc, yuv, blk)
        with pytest.raises(RuntimeError, match="plate_picture_yuv: plate_y must be contiguous int32 .7, 9, 2."):
            ops.plate_picture_yuv(bad, pc, fy, yuv[:1])
    for bad in (pc.float(), torch.zeros(3, 4, 4, dtype=torch.int32), torch.zeros(4, 5, 2, dtype=torch.int32), None):
        with pytest.raises(RuntimeError, match="plate_update_yuv: plate_c must be contiguous int32 .4, 5, 4."):
            ops.plate_update_yuv(py, bad, yuv, blk)
    with pytest.raises(RuntimeError, match="plate_update_yuv: block must be contiguous uint8 .F = 2, 7, 9."):
        ops.plate_update_yuv(py, pc, yuv, blk[:1])
    with pytest.raises(RuntimeError, match="plate_update_yuv: n_max must be an int in 1..256"):
        ops.plate_update_yuv(py, pc, yuv, blk, 0)
    for bad in (yuv, torch.zeros(7, 9, dtype=torch.uint8), None):
        with pytest.raises(RuntimeError, match="plate_picture_yuv: out must be a preprocess.YuvFrames of ONE surface"):
            ops.plate_picture_yuv(py, pc, fy, bad)
    for bad in (fy.view(torch.int16).to(torch.int32), fill, None):
        with pytest.raises(RuntimeError, match="plate_picture_yuv: fill_yuv must be contiguous uint16 .3."):
            ops.plate_picture_yuv(py, pc, bad, yuv[:1])
    with pytest.raises(RuntimeError, match="plate_picture_yuv: reach must be an int in 0..32"):
        ops.plate_picture_yuv(py, pc, fy, yuv[:1], 33)
    with pytest.raises(RuntimeError, match="plate_update_yuv: plate_y must be a CUDA tensor"):
        ops.plate_update_yuv(py, pc, yuv, blk)
    with pytest.raises(RuntimeError, match="plate_picture_yuv: plate_y must be a CUDA tensor"):
        ops.plate_picture_yuv(py, pc, fy, yuv[:1])


# ---- merge.overlay_frames: which launches a style makes ---------------------------------------------------------------------------------
class _Store:
    """A FrameStore's `pieces` for frames [10, 15): two pieces of 3 and 2 frames."""
    def __init__(self, make):
        self.make = make

    def pieces(self, f0, f1, stream=None):
        assert (f0, f1) == (10, 15)
        return [(self.make(3), 10), (self.make(2), 13)]


def _record(monkeypatch, style, surface, plate="make", n=2, windows=1):
    """The (name, args) of every ops call merge.overlay_frames makes for `windows` windows of 5 frames of 6 x 8 and n tracks, with every
    ops call replaced by a recorder."""
    from mdqe_cvpr2023_amd import merge, ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    calls = []
    sfx = "_yuv" if surface else ""
    for name in ("render_overlay", "render_replace", "plate_update", "plate_picture"):
        for s in ("", "_yuv"):
            monkeypatch.setattr(ops, name + s, (lambda k: lambda *a, **kw: (calls.append((k, a, kw)), a[3] if k.startswith("plate_picture") else None)[1])(name + s))

    def grow_labels(labels, table, radius, out=None):
        calls.append(("grow_labels", (labels, table, radius, out), {}))
        return out
    monkeypatch.setattr(ops, "grow_labels", grow_labels)
    monkeypatch.setattr(merge, "label_maps", lambda *a: None)
    monkeypatch.setattr(merge, "replace_matte", lambda m, *a: torch.zeros(5, 6, 8, dtype=torch.uint8))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    m = torch.zeros(n, 5, 3, 4)
    labels = torch.zeros(7, 6, 8, dtype=torch.uint8)
    kind = dict(fmt="nv12", matrix="bt601", full_range=True, order="bgr")
    if surface:
        out = YuvFrames.empty(6, 6, 8, **kind)
        store = _Store(lambda k: YuvFrames.empty(k, 6, 8, **kind))
    else:
        out = torch.zeros(6, 6, 8, 3, dtype=torch.uint8)
        store = _Store(lambda k: torch.zeros(k, 3, 6, 8, dtype=torch.uint8))
    if plate == "make":
        forms = merge.Forms.of_emit("overlay", surface=surface)
        plate = merge.plate_of(forms, style, (6, 8), torch.device("cpu"), out)
    kw = {} if plate is None else {"plate": plate}
    for _ in range(windows):
        merge.overlay_frames(m, 8, (6, 8), (6, 8), False, labels, 1, store, 10, style, torch.zeros(n, 2), out, 1, **kw)
    return calls, labels, plate, sfx


@pytest.mark.parametrize("surface", [False, True])
def test_overlay_frames_teaches_the_plate_and_hands_the_painters_its_picture(monkeypatch, surface):
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.render import Style
    # any other backdrop: no Plate, exactly the former calls
    for st in (Style(), Style(replace="tracks"), Style(replace="background", backdrop=(1, 2, 3))):
        calls, _, plate, sfx = _record(monkeypatch, st, surface)
        assert plate is None and [c[0] for c in calls] == [("render_replace" if st.replace else "render_overlay") + sfx] * 2
    # the plate, margin 4: one grow launch, an update per piece in order, one picture, then the painters with that picture as `back`
    st = Style(replace="tracks", backdrop="plate", plate_frames=9, plate_reach=7, plate_fill=(1, 2, 3))
    for n in (2, 0):                                                  # (a window without tracks still teaches the plate)
        calls, labels, plate, sfx = _record(monkeypatch, st, surface, n=n, windows=3)
        assert isinstance(plate, merge.Plate) and (plate.kind is None) == (not surface)
        one = ["grow_labels", "plate_update" + sfx, "plate_update" + sfx, "plate_picture" + sfx, "render_replace" + sfx, "render_replace" + sfx]
        assert [c[0] for c in calls] == one * 3
        lab, table, radius, scratch = calls[0][1]
        assert lab.data_ptr() == labels[1:6].data_ptr() and tuple(lab.shape) == (5, 6, 8) and radius == 4 and table.tolist() == [1] * 256
        assert scratch.data_ptr() == plate.scratch.data_ptr() and tuple(scratch.shape) == (5, 6, 8)
        for w in range(3):
            (_, u0, _), (_, u1, _), (_, p, _), (_, r0, _), (_, r1, _) = calls[6 * w + 1:6 * w + 6]
            states = (plate.state, plate.state_c) if surface else (plate.state,)
            for u, (d, k) in ((u0, (0, 3)), (u1, (3, 2))):
                assert all(a is b for a, b in zip(u, states)) and len(u[len(states)]) == k and u[-1] == 9
                assert u[-2].data_ptr() == plate.scratch[d:d + k].data_ptr() and len(u[-2]) == k
            assert all(a is b for a, b in zip(p, states)) and p[len(states)] is plate.fill
            assert (p[-2] is plate.back and p[-1] == 7) if surface else (p[-1] is plate.back and p[-2] == 7)
            for r in (r0, r1):
                assert r[5] is plate.back and r[-1] == "tracks"          # the painters' backdrop
        assert calls[6][1][3].data_ptr() == scratch.data_ptr()            # the same scratch, state and backdrop in every window
    # margin 0: the label map itself is the block, no grow launch, no scratch
    st0 = Style(replace="tracks", backdrop="plate", plate_margin=0)
    calls, labels, plate, sfx = _record(monkeypatch, st0, surface)
    assert [c[0] for c in calls] == ["plate_update" + sfx] * 2 + ["plate_picture" + sfx] + ["render_replace" + sfx] * 2
    assert calls[0][1][-2].data_ptr() == labels[1:4].data_ptr() and calls[1][1][-2].data_ptr() == labels[4:6].data_ptr() and plate.scratch is None
    # the state: fresh zeros of the rule's shapes
    if surface:
        assert tuple(plate.state.shape) == (6, 8, 2) and tuple(plate.state_c.shape) == (3, 4, 4) and plate.back.meta() == (6, 8, "nv12", "bt601", True, "bgr")
        assert not plate.state.any() and not plate.state_c.any() and plate.fill.dtype in (torch.uint16, torch.int16)
    else:
        assert tuple(plate.state.shape) == (6, 8, 4) and plate.state.dtype == torch.int32 and not plate.state.any()
        assert tuple(plate.back.shape) == (6, 8, 3) and plate.fill.tolist() == [128, 128, 128]
    # a plate style without the video's Plate is an error, not a fall-back
    with pytest.raises(RuntimeError, match="needs the video's Plate"):
        _record(monkeypatch, st, surface, plate=None)


def test_plate_init_starts_the_state_and_two_videos_share_no_state():
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style
    pic = torch.arange(6 * 8 * 3, dtype=torch.uint8).view(6, 8, 3)
    st = Style(replace="tracks", backdrop="plate", plate_init=pic)
    a, b = merge.Plate(st, (6, 8), torch.device("cpu")), merge.Plate(st, (6, 8), torch.device("cpu"))
    assert a.state.data_ptr() != b.state.data_ptr() and a.back.data_ptr() != b.back.data_ptr()      # the state is the video's, not the style's
    want = REF.to_state(*REF.from_picture(pic.numpy()))
    assert np.array_equal(a.state.numpy(), want) and np.array_equal(b.state.numpy(), want)
    for fmt in ("nv12", "p010"):
        s = YuvFrames.empty(1, 5, 7, fmt=fmt)
        ys = np.arange(35).reshape(5, 7) * 3
        cs = np.arange(24).reshape(3, 8) * 5
        if fmt == "p010":
            s.y[0].copy_(torch.from_numpy(((ys * 9) << 6 | 0x2A).astype(np.uint16).view(np.int16)).view(s.y.dtype))
            s.uv[0].copy_(torch.from_numpy(((cs * 8) << 6 | 0x15).astype(np.uint16).view(np.int16)).view(s.uv.dtype))
            ys, cs = ys * 9, cs * 8
        else:
            s.y[0].copy_(torch.from_numpy(ys.astype(np.uint8)))
            s.uv[0].copy_(torch.from_numpy(cs.astype(np.uint8)))
        p = merge.Plate(Style(replace="tracks", backdrop="plate", plate_init=s), (5, 7), torch.device("cpu"), s.meta())
        assert np.array_equal(p.state.numpy(), REF.to_state(*REF.from_picture(ys[..., None])))
        assert np.array_equal(p.state_c.numpy(), REF.to_state(*REF.from_picture(cs.reshape(3, 4, 2))))
