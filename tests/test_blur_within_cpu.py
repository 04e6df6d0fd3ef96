"""The edge-stopping blur without a GPU: the oracle (tests/_blur_within_ref.py: its loop form against its vectorised form), what the rule
of include/mdqe_hip.h promises (a constant member region keeps its value, a blurred pixel does not depend on any non-member's source --
where the plain blur's does --, the all-member case is within 1 of the plain blur, the 32-bit bound at 255 and the wide one at 1023),
render.Style's `blur_edge`, the two entries in the header and in the library, the `edge` keyword of the wrappers, the painter
dispatch, and the host path of ops.render_blur_yuv(edge="stop") against the oracle.  Integers only: every comparison is exact."""
import dataclasses
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

import _blur_ref as BREF  # noqa: E402
import _blur_within_ref as REF  # noqa: E402
import _overlay_ref as OREF  # noqa: E402
import _overlay_yuv_ref as OYREF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402
from test_blur_cpu import _raw, _record, _rgb_case, _taps, _typed  # noqa: E402

TABLES = REF.action_tables()


def _blob_labels(F, H, W):
    """Label 9 on an irregular region that touches a border, label 4 on a block, background elsewhere."""
    lab = np.zeros((F, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(F):
        lab[f][(yy - H // 2) ** 2 * 4 + (xx - W // 3 - f) ** 2 < (H * H) // 2 + 3] = 9
        lab[f, :2, W - 4:] = 9
        lab[f, H - 3:, :3] = 4
    return lab


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def test_the_loop_reference_equals_the_vectorised_one():
    rng = np.random.default_rng(7)
    lab, fr, pal = _rgb_case(5, 2, 9, 13, 9, 13)
    act = np.array([0, 1, 3], dtype=np.uint8)[rng.integers(0, 3, size=256)]
    assert all((act[lab] == k).any() for k in (0, 1, 3))
    for radius in (0, 1, 3):
        taps = _taps(radius)
        a = REF.paint(lab, fr, pal, act, 128, 1, taps)
        b = REF.paint(lab, fr, pal, act, 128, 1, taps, within_fn=REF.within_loops)
        assert np.array_equal(a, b), radius
        if radius == 0:                                               # the identity on the blurred pixels
            assert np.array_equal(a[act[lab] == 3], np.moveaxis(fr, 1, -1)[act[lab] == 3])
    assert not np.array_equal(a, BREF.paint(lab, fr, pal, act, 128, 1, taps))     # another picture than the plain blur's
    for fmt, top in (("nv12", 256), ("p010", 1024)):
        ys, cs = YREF.make_content(11, 2, 7, 9, fmt)
        labs = OYREF.make_labels(4, 2, 7, 9)
        pal = np.random.default_rng(2).integers(0, top, size=(256, 3))
        a = REF.paint_yuv(ys, cs, labs, pal, act, fmt, 77, 2, _taps(3), _taps(2))
        b = REF.paint_yuv(ys, cs, labs, pal, act, fmt, 77, 2, _taps(3), _taps(2), within_fn=REF.within_loops)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), fmt


@pytest.mark.parametrize("radius", [0, 2, 32])
def test_reference_under_the_plain_table_is_the_plain_overlay(radius):
    lab, fr, pal = _rgb_case(3, 2, 13, 21, 9, 30)
    assert np.array_equal(REF.paint(lab, fr, pal, TABLES["plain"], 77, 2, _taps(radius)), OREF.paint(lab, fr, pal, 77, 2))


def test_a_constant_member_region_keeps_its_value_whatever_lies_outside():
    F, H, W = 2, 20, 31
    lab = _blob_labels(F, H, W)
    act = np.zeros(256, dtype=np.uint8)
    act[9], act[4] = 3, 1
    member = lab == 9
    rng = np.random.default_rng(1)
    pal = rng.integers(0, 256, size=(256, 3)).astype(np.uint8)
    for radius, v in ((1, (0, 255, 7)), (5, (200, 1, 254)), (17, (255, 255, 255)), (32, (13, 128, 0))):
        fr = rng.integers(0, 256, size=(F, 3, H, W)).astype(np.uint8)
        for c in range(3):
            fr[:, c][member] = v[c]
        out = REF.paint(lab, fr, pal, act, 128, 1, _taps(radius))
        assert (out[member] == np.array(v, dtype=np.uint8)).all(), radius
        plain = BREF.paint(lab, fr, pal, act, 128, 1, _taps(radius))
        assert not (plain[member] == np.array(v, dtype=np.uint8)).all(), radius      # the plain blur takes the surroundings in
        assert np.array_equal(out[~member], plain[~member])


@pytest.mark.parametrize("table", ["background", "mix"])
def test_a_blurred_pixel_does_not_depend_on_any_non_member_where_the_plain_blurs_does(table):
    lab, fr, pal = _rgb_case(9, 2, 23, 37, 23, 37)
    act = TABLES[table]
    member = act[lab] == 3
    assert member.any() and (~member).any()
    other = fr.copy()
    noise = np.random.default_rng(2).integers(0, 256, size=fr.shape).astype(np.uint8)
    for c in range(3):
        other[:, c][~member] = noise[:, c][~member]
    assert np.array_equal(other[:, 0][member], fr[:, 0][member]) and not np.array_equal(other, fr)
    for radius in (1, 5, 17):
        taps = _taps(radius)
        a, b = REF.paint(lab, fr, pal, act, 128, 1, taps), REF.paint(lab, other, pal, act, 128, 1, taps)
        assert np.array_equal(a[member], b[member]), radius
        pa, pb = BREF.paint(lab, fr, pal, act, 128, 1, taps), BREF.paint(lab, other, pal, act, 128, 1, taps)
        assert not np.array_equal(pa[member], pb[member]), radius    # the same input through the plain blur does change
    # surfaces: luma among the member pixels, chroma among the member pairs
    for fmt, top in (("nv12", 256), ("p010", 1024)):
        F, H, W = 2, 11, 17
        ys, cs = YREF.make_content(3, F, H, W, fmt)
        labs = OYREF.make_labels(5, F, H, W)
        m = act[labs] == 3
        full = np.zeros((F, 12, 18), dtype=bool)
        full[:, :H, :W] = m
        pair = full[:, 0::2, 0::2] | full[:, 0::2, 1::2] | full[:, 1::2, 0::2] | full[:, 1::2, 1::2]
        assert m.any() and (~m).any() and (~pair).any()
        rng = np.random.default_rng(4)
        ys2, cs2 = ys.copy(), cs.copy()
        ys2[~m] = (rng.integers(0, top, size=ys.shape) << (6 if fmt == "p010" else 0)).astype(ys.dtype)[~m]
        pm = np.repeat(pair, 2, axis=2)
        cs2[~pm] = (rng.integers(0, top, size=cs.shape) << (6 if fmt == "p010" else 0)).astype(cs.dtype)[~pm]
        palette = rng.integers(0, top, size=(256, 3))
        a = REF.paint_yuv(ys, cs, labs, palette, act, fmt, 128, 1, _taps(5), _taps(3))
        b = REF.paint_yuv(ys2, cs2, labs, palette, act, fmt, 128, 1, _taps(5), _taps(3))
        assert np.array_equal(a[0][m], b[0][m]), fmt
        assert np.array_equal(a[1][pm], b[1][pm]) and not np.array_equal(a[1], b[1]), fmt      # (a member pair's own U, V did not change)
        pa = BREF.paint_yuv(ys, cs, labs, palette, act, fmt, 128, 1, _taps(5), _taps(3))
        pb = BREF.paint_yuv(ys2, cs2, labs, palette, act, fmt, 128, 1, _taps(5), _taps(3))
        assert not np.array_equal(pa[0][m], pb[0][m]) and not np.array_equal(pa[1][pm], pb[1][pm]), fmt


@pytest.mark.parametrize("radius", [1, 5, 17, 32])
def test_where_every_pixel_is_a_member_the_value_is_within_1_of_the_plain_blur(radius):
    rng = np.random.default_rng(radius)
    v = rng.integers(0, 256, size=(2, 19, 27, 3)).astype(np.int64)
    v[1, :, :13] = 255                                                # a hard step: the largest row-rounding errors
    v[1, :, 13:] = 0
    got, plain = REF.within(v, np.ones(v.shape[:3], dtype=bool), _taps(radius)), BREF.blur(v, _taps(radius))
    assert np.abs(got - plain).max() <= 1
    v10 = rng.integers(0, 1024, size=(1, 9, 40)).astype(np.int64)
    assert np.abs(REF.within(v10, np.ones(v10.shape, dtype=bool), _taps(radius)) - BREF.blur(v10, _taps(radius))).max() <= 1


def test_the_bounds_all_255_and_all_1023_at_radius_32():
    lab = OYREF.make_labels(1, 1, 9, 13)
    pal = np.zeros((256, 3), dtype=np.uint8)
    fr = np.full((1, 3, 9, 13), 255, dtype=np.uint8)
    assert (REF.paint(lab, fr, pal, TABLES["all"], 128, 1, _taps(32)) == 255).all()
    w, R = BREF._taps(_taps(32))
    ones = np.ones((1, 9, 13), dtype=np.int64)
    assert (REF._sums(ones, w, R) == 2 ** 24).all() and int((REF._sums(255 * ones, w, R) + 2 ** 23).max()) == 4286578688 < 2 ** 32
    assert int(REF._sums(1023 * ones, w, R).max()) > 2 ** 32                          # 10-bit values need the wide sum
    for fmt, top in (("nv12", 255), ("p010", 1023)):
        sh = 6 if fmt == "p010" else 0
        dt = np.uint16 if fmt == "p010" else np.uint8
        ys, cs = np.full((1, 9, 13), top << sh, dtype=dt), np.full((1, 5, 14), top << sh, dtype=dt)
        gy, gc = REF.paint_yuv(ys, cs, lab, np.zeros((256, 3), dtype=np.int64), TABLES["all"], fmt, 128, 1, _taps(32), _taps(16))
        assert (gy == top << sh).all() and (gc == top << sh).all(), fmt


# ---- the style -----------------------------------------------------------------------------------------------------------------------
def test_style_blur_edge_field_order_defaults_and_refusals():
    from mdqe_cvpr2023_amd.render import Style
    names = [f.name for f in dataclasses.fields(Style)]
    assert names[:19] == ["alpha", "contour", "palette", "mosaic", "cell", "classes", "blur", "blur_radius", "box", "caption", "class_names",
                          "text_scale", "min_area", "trail", "trail_width", "replace", "backdrop", "matte_gain", "grow"]
    assert names[19] == "blur_edge"
    assert Style().blur_edge == "bleed" and Style(blur="tracks").blur_edge == "bleed" and Style() == Style(blur_edge="bleed")
    for blur in ("tracks", "background"):
        st = Style(blur=blur, blur_edge="stop", grow=4)
        assert st.blur_edge == "stop" and st.actions().tolist() == Style(blur=blur).actions().tolist()
    assert Style(blur="tracks", classes=[0], blur_edge="stop", grow=8).classes == (0,)
    for bad in ("Stop", "", None, 1, True, "edge"):
        with pytest.raises(ValueError, match="blur_edge must be 'bleed' or 'stop'"):
            Style(blur="tracks", blur_edge=bad)
    for kw in ({}, {"mosaic": "tracks"}, {"replace": "background"}):
        with pytest.raises(ValueError, match="(?s)blur_edge='stop'.*add blur='tracks' or blur='background'"):
            Style(blur_edge="stop", **kw)
    doc = Style.__doc__
    assert '"bleed"' in doc and '"stop"' in doc


# ---- the entries and the wrappers ----------------------------------------------------------------------------------------------------
def test_abi_declares_both_entries_and_the_library_exports_and_checks_them():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)                                    # new entries only
    for name, plain in (("mdqe_render_blur_within_u8", "mdqe_render_blur_u8"), ("mdqe_render_blur_within_yuv420sp", "mdqe_render_blur_yuv420sp")):
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
        assert proto, name + " is not declared in mdqe_hip.h"
        want = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % plain, src, flags=re.S).group(1)
        assert re.sub(r"\s+", " ", proto.group(1)) == re.sub(r"\s+", " ", want)                    # the plain entry's argument list
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[plain]
    if not os.path.exists(_lib.LIB_PATH):
        return
    h = _lib.load_library()
    assert h.mdqe_abi_version() == 6
    assert hasattr(h, "mdqe_render_blur_within_u8") and hasattr(h, "mdqe_render_blur_within_yuv420sp")
    EINVAL, ENULL = 1, 3

    def rgb(F=1, Ho=8, Wo=8, a256=128, contour=1, radius=8, f_off=0):
        return h.mdqe_render_blur_within_u8(None, 1, 0, 0, 0, None, F, Ho, Wo, None, None, a256, contour, None, radius, None, f_off, None)

    def yuv(F=1, H=32, W=64, fmt=0, a256=128, contour=1, radius=8, radius_c=4, f_off=0, ptrs=None):
        q = dict({"y": None, "uv": None, "labels": None, "pal": None, "act": None, "taps": None, "taps_c": None, "oy": None, "ouv": None},
                 **(ptrs or {}))
        return h.mdqe_render_blur_within_yuv420sp(q["y"], 64, 64 * 48, q["uv"], 64, 64 * 48, F, H, W, fmt, q["labels"], q["pal"], q["act"],
                                                  a256, contour, q["taps"], radius, q["taps_c"], radius_c, q["oy"], 64, 64 * 48, q["ouv"],
                                                  64, 64 * 48, f_off, None)
    for call in (rgb, yuv):
        for kw in ({"radius": -1}, {"radius": 33}, {"contour": 4}, {"a256": 257}, {"F": -1}, {"f_off": -1}):
            assert call(**kw) == EINVAL and call(**dict(kw, F=kw.get("F", 0))) == EINVAL, (call.__name__, kw)
        assert call(F=0, radius=32) == 0 and call() == ENULL                                       # F = 0: OK, nothing launched
    assert yuv(radius_c=17) == EINVAL and yuv(fmt=2) == EINVAL
    # never dereferenced (the refusals come before the launch): in place and any other overlap of an output plane
    ptrs = {"y": 1 << 20, "uv": 2 << 20, "labels": 3 << 20, "pal": 4 << 20, "act": 7 << 20, "taps": 8 << 20, "taps_c": 9 << 20,
            "oy": 5 << 20, "ouv": 6 << 20}
    for kw in ({"oy": ptrs["y"]}, {"ouv": ptrs["uv"]}, {"oy": ptrs["y"] + 64}, {"ouv": ptrs["y"]}, {"oy": ptrs["labels"] + 5},
               {"taps": ptrs["oy"] + 100}, {"taps": ptrs["taps"] + 1}):
        assert yuv(ptrs=dict(ptrs, **kw)) == EINVAL, kw


def test_the_edge_keyword_of_the_wrappers():
    import inspect
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import blur_taps
    for fn in (ops.render_blur, ops.render_blur_yuv):
        par = list(inspect.signature(fn).parameters.values())
        assert par[-1].name == "edge" and par[-1].default == "bleed"
    lab = torch.zeros(1, 4, 6, dtype=torch.uint8)
    act, taps = torch.from_numpy(TABLES["all"]), blur_taps(2)
    src = YuvFrames.empty(1, 4, 6, fmt="nv12")
    pal = torch.zeros(256, 3, dtype=torch.int16)
    for bad in ("Stop", None, 1, ""):
        with pytest.raises(RuntimeError, match="render_blur: edge must be 'bleed' or 'stop'"):
            ops.render_blur(lab, None, torch.zeros(256, 3, dtype=torch.uint8), act, taps, torch.zeros(1, 4, 6, 3, dtype=torch.uint8), edge=bad)
        with pytest.raises(RuntimeError, match="render_blur_yuv: edge must be 'bleed' or 'stop'"):
            ops.render_blur_yuv(lab, src, pal, act, taps, taps, edge=bad)
    with pytest.raises(RuntimeError, match="taps must be contiguous uint16"):                       # the same argument checks
        ops.render_blur_yuv(lab, src, pal, act, taps.to(torch.int32), taps, edge="stop")


@pytest.mark.parametrize("surface", [False, True])
def test_overlay_frames_passes_the_edge_only_for_stop(monkeypatch, surface):
    from mdqe_cvpr2023_amd.render import Style
    sfx = "_yuv" if surface else ""
    for st in (Style(blur="background", blur_edge="stop", alpha=0, contour=0), Style(blur="tracks", classes=[1], blur_edge="stop")):
        calls, _, out = _record(monkeypatch, st, surface)
        assert [c[0] for c in calls] == ["render_blur" + sfx] * 2 and all(c[2] == {"edge": "stop"} for c in calls)
        same, _, _ = _record(monkeypatch, dataclasses.replace(st, blur_edge="bleed"), surface)
        assert all(not c[2] for c in same)                            # "bleed": exactly the former calls
        for (_, a, _), (_, b, _) in zip(calls, same):
            assert len(a) == len(b) and a[-3:] == b[-3:] and a[3].tolist() == b[3].tolist()


# ---- the host path of ops.render_blur_yuv(edge="stop") ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(5, 7), (34, 70)])
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
            got = ops.render_blur_yuv(torch.from_numpy(lab), src, pal, torch.from_numpy(act), taps, taps_c, a256=a256, contour=contour, edge="stop")
            assert (len(got), got.meta()) == (F, src.meta()) and tuple(got.y.shape) == (F, H, W)
            assert np.array_equal(_raw(got.y, fmt), wy) and np.array_equal(_raw(got.uv, fmt), wc), (radius, name)
            if name == "plain":                                       # ... the plain overlay's host path
                ref = ops.render_overlay_yuv(torch.from_numpy(lab), src, pal, a256=a256, contour=contour)
                assert np.array_equal(_raw(ref.y, fmt), wy) and np.array_equal(_raw(ref.uv, fmt), wc)
            elif radius:                                              # ... and another picture than "bleed"'s
                bleed = ops.render_blur_yuv(torch.from_numpy(lab), src, pal, torch.from_numpy(act), taps, taps_c, a256=a256, contour=contour)
                assert name == "all" or H * W < 40 or not np.array_equal(_raw(bleed.y, fmt), wy), (radius, name)
            k += 1
    assert np.array_equal(flat, before)
    with pytest.raises(RuntimeError, match="render_blur_yuv: out must not share memory"):          # not in place, as "bleed"
        ops.render_blur_yuv(torch.from_numpy(lab), src, pal, torch.from_numpy(TABLES["all"]), taps, taps_c, src, edge="stop")
