"""Track paths without a GPU: the properties of the rule as tests/_paths_ref.py states it (a lone point draws a disc, a width-1 line is
connected and does not depend on its direction, gaps are bridged, points outside the picture are ignored, the centroid's rounding), the
style's two fields, the header and the library's exports, the wrappers' argument checks on the host, the point table's bookkeeping and
the refusals of the layers above."""
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

import _paths_ref as REF  # noqa: E402

PAL = np.arange(256 * 3, dtype=np.int64).reshape(256, 3) % 251 + 1    # (no row is black)


def _mask(Ho, Wo, A, B, width):
    m = np.zeros((Ho, Wo), dtype=bool)
    ys, xs, part = REF.stroke_mask(Ho, Wo, A, B, width)
    m[ys, xs] = part
    return m


# ---- the reference's own properties ----------------------------------------------------------------------------------------------------
def test_a_lone_point_draws_a_disc():
    yy, xx = np.mgrid[:21, :21]
    for width, count in ((1, 1), (2, 5), (3, 9), (4, 13), (5, 21)):  # pixels with 4 * (dx^2 + dy^2) <= width^2
        m = _mask(21, 21, (10, 10), (10, 10), width)
        assert np.array_equal(m, 4 * ((xx - 10) ** 2 + (yy - 10) ** 2) <= width * width) and int(m.sum()) == count, width
    pts = np.full((1, 4, 2), -1, dtype=np.int32)
    pts[0, 2] = (10, 10)
    pic = REF.trails_rgb(np.zeros((1, 21, 21, 3), dtype=np.uint8), pts, 1, PAL, 1, 0, 2, 2, 3)
    assert np.array_equal(pic[0].any(-1), _mask(21, 21, (10, 10), (10, 10), 3)) and (pic[0][10, 10] == PAL[1]).all()


def _connected8(m):
    """Whether the set pixels of m form one 8-connected component."""
    todo, seen = [tuple(np.argwhere(m)[0])], set()
    while todo:
        y, x = todo.pop()
        if (y, x) in seen:
            continue
        seen.add((y, x))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = y + dy, x + dx
                if 0 <= yy < m.shape[0] and 0 <= xx < m.shape[1] and m[yy, xx] and (yy, xx) not in seen:
                    todo.append((yy, xx))
    return len(seen) == int(m.sum())


def test_a_width_1_line_is_connected_covers_every_column_or_row_and_is_symmetric():
    rng = np.random.default_rng(1)
    ends = [((0, 0), (39, 39)), ((0, 39), (39, 0)), ((0, 7), (39, 7)), ((5, 0), (5, 39)), ((0, 0), (39, 1)), ((3, 38), (4, 0)), ((17, 17), (18, 18))]
    ends += [(tuple(int(v) for v in rng.integers(0, 40, 2)), tuple(int(v) for v in rng.integers(0, 40, 2))) for _ in range(150)]
    for A, B in ends:
        m = _mask(40, 40, A, B, 1)
        assert np.array_equal(m, _mask(40, 40, B, A, 1)), (A, B)      # swapping the ends changes nothing
        assert m[A[1], A[0]] and m[B[1], B[0]] and _connected8(m), (A, B)
        if abs(B[0] - A[0]) >= abs(B[1] - A[1]):                      # at least one pixel per column; per row on steep lines
            assert m.any(0)[min(A[0], B[0]):max(A[0], B[0]) + 1].all(), (A, B)
        else:
            assert m.any(1)[min(A[1], B[1]):max(A[1], B[1]) + 1].all(), (A, B)
    for A, B in ends[:20]:                                            # wider lines contain the narrower ones
        for w in (2, 3, 4, 5):
            assert not (_mask(40, 40, A, B, w - 1) & ~_mask(40, 40, A, B, w)).any(), (A, B, w)


def test_gaps_are_bridged_and_points_outside_the_picture_or_before_column_0_are_ignored():
    Ho, Wo = 20, 30
    pts = np.full((2, 8, 2), -1, dtype=np.int64)
    pts[0, 1], pts[0, 5] = (2, 3), (25, 15)                           # columns 2..4 absent: one line from column 1 to column 5
    pts[0, 3] = (Wo, 5)                                               # x == Wo: absent
    pts[0, 4] = (7, -2 ** 31)                                         # negative, huge: absent
    black = np.zeros((1, Ho, Wo, 3), dtype=np.uint8)
    got = REF.trails_rgb(black, pts, 1, PAL, 1, 0, 5, 4, 1)[0].any(-1)
    assert np.array_equal(got, _mask(Ho, Wo, (2, 3), (25, 15), 1))
    assert REF.strokes_of(REF.present_points(pts[0], 1, 5, Ho, Wo)) == [((2, 3), (2, 3)), ((25, 15), (25, 15)), ((2, 3), (25, 15))]
    # a trail of 3 no longer reaches column 1: the lone point's disc
    assert np.array_equal(REF.trails_rgb(black, pts, 1, PAL, 1, 0, 5, 3, 1)[0].any(-1), _mask(Ho, Wo, (25, 15), (25, 15), 1))
    # columns below 0 are absent (p_off + f - trail < 0), and nothing present means nothing written
    assert np.array_equal(REF.trails_rgb(black, pts, 1, PAL, 1, 0, 1, 64, 1)[0].any(-1), _mask(Ho, Wo, (2, 3), (2, 3), 1))
    noise = np.random.default_rng(2).integers(0, 256, size=(2, Ho, Wo, 3)).astype(np.uint8)
    assert np.array_equal(REF.trails_rgb(noise, pts, 2, PAL, 1, 1, 0, 64, 5), noise)
    # the lower label lies over the higher one where they cross; frames outside the call keep their bytes
    pts[1, 1], pts[1, 5] = (2, 15), (25, 3)
    pic = REF.trails_rgb(noise, pts, 2, PAL, 1, 1, 5, 4, 2)
    a, b = _mask(Ho, Wo, (2, 3), (25, 15), 2), _mask(Ho, Wo, (2, 15), (25, 3), 2)
    assert (a & b).any() and (pic[1][a] == PAL[1]).all() and (pic[1][b & ~a] == PAL[2]).all()
    assert np.array_equal(pic[1][~(a | b)], noise[1][~(a | b)]) and np.array_equal(pic[0], noise[0])


def test_centroid_rounding_on_hand_made_maps():
    lab = np.zeros((2, 4, 6), dtype=np.uint8)
    lab[0, 0, 0:2] = 1                                                # x = 0, 1: SX = 1, m = 2 -> (1 + 1) / 2 = 1 (a half rounds up)
    lab[0, 1:4, 3] = 2                                                # y = 1, 2, 3: SY = 6, m = 3 -> 2
    lab[0, 3, 4:6] = 3                                                # x = 4, 5, y = 3
    lab[1, 0, 0], lab[1, 0, 1], lab[1, 0, 2] = 1, 1, 1
    lab[1, 2, 0] = 1                                                  # x = 0, 1, 2, 0: SX = 3, m = 4 -> (3 + 2) / 4 = 1; SY = 2 -> (2 + 2) / 4 = 1
    lab[1, 3, 5] = 9                                                  # a label above n: counted nowhere
    mom, pts = REF.centroids(lab, 4)
    assert mom[:, 0].tolist() == [[2, 1, 0], [3, 9, 6], [2, 9, 6], [0, 0, 0]] and mom[:, 1].tolist() == [[4, 3, 2], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    assert pts[:, 0].tolist() == [[1, 0], [3, 2], [5, 3], [-1, -1]] and pts[:, 1].tolist() == [[1, 1], [-1, -1], [-1, -1], [-1, -1]]
    _, pts3 = REF.centroids(lab, 4, min_area=3)                       # present: m >= max(1, min_area)
    assert pts3[:, 0].tolist() == [[-1, -1], [3, 2], [-1, -1], [-1, -1]] and pts3[:, 1].tolist() == [[1, 1], [-1, -1], [-1, -1], [-1, -1]]
    assert mom.dtype == np.int64 and pts.dtype == np.int32 and REF.centroids(lab, 0)[0].shape == (0, 2, 3)


def test_surface_form_keeps_what_it_does_not_hit_and_averages_chroma_blocks():
    H, W = 5, 7                                                       # odd both ways: blocks of 1 and 2 pixels on the edges
    rng = np.random.default_rng(3)
    for fmt, top in (("nv12", 256), ("p010", 65536)):
        dt = np.uint8 if fmt == "nv12" else np.uint16
        y, uv = rng.integers(0, top, size=(1, H + 1, W + 3)).astype(dt), rng.integers(0, top, size=(1, 4, 10)).astype(dt)
        pal = rng.integers(0, 256 if fmt == "nv12" else 1024, size=(256, 3)).astype(np.int64)
        pts = np.array([[[6, 4]]], dtype=np.int32)                    # the last pixel: a chroma block of ONE pixel
        oy, ouv = REF.trails_yuv(y, uv, fmt, H, W, pts, 1, pal, 1, 0, 0, 1, 1)
        sh = 0 if fmt == "nv12" else 6
        assert oy[0, 4, 6] == pal[1, 0] << sh and ouv[0, 2, 6] == pal[1, 1] << sh and ouv[0, 2, 7] == pal[1, 2] << sh
        oy[0, 4, 6], ouv[0, 2, 6], ouv[0, 2, 7] = y[0, 4, 6], uv[0, 2, 6], uv[0, 2, 7]
        assert np.array_equal(oy, y) and np.array_equal(ouv, uv)     # every other sample, the padding and P010's low bits kept
        pts = np.array([[[2, 2]]], dtype=np.int32)                    # one pixel of a full block: (hit + 3 stored + 2) >> 2
        oy, ouv = REF.trails_yuv(y, uv, fmt, H, W, pts, 1, pal, 1, 0, 0, 1, 1)
        assert ouv[0, 1, 2] == ((int(pal[1, 1]) + 3 * (int(uv[0, 1, 2]) >> sh) + 2) >> 2) << sh


# ---- the style -------------------------------------------------------------------------------------------------------------------------
def test_style_validates_trail_and_trail_width():
    from mdqe_cvpr2023_amd.render import Style
    st = Style()
    assert (st.trail, st.trail_width, st.trails, st.annotates) == (0, 2, False, False)
    assert Style(trail=64, trail_width=5).trails and Style(trail=1, trail_width=1).trails and not Style(trail=0, trail_width=5).trails
    assert not Style(trail=3).annotates and not Style(box=1).trails
    for bad in (-1, 65, 1.0, True, None, "3"):
        with pytest.raises(ValueError, match=r"overlay style: trail must be an int in 0\.\.64"):
            Style(trail=bad)
    for bad in (0, 6, 2.0, True, None):
        with pytest.raises(ValueError, match=r"overlay style: trail_width must be an int in 1\.\.5"):
            Style(trail_width=bad)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_the_three_entries():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    for name, n_args in (("mdqe_label_centroids_u8", 11), ("mdqe_render_trails_u8", 13), ("mdqe_render_trails_yuv420sp", 19)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
        assert hasattr(h, name) and name in _lib.SIGNATURES
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == n_args
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # new entries only
    EINVAL, ENULL = 1, 3                                              # (the refusals need no device: they come before any pointer is looked at)
    assert h.mdqe_label_centroids_u8(None, 1, 8, 8, 256, 0, None, None, 64, 0, None) == EINVAL
    assert h.mdqe_label_centroids_u8(None, 1, 8, 8, 2, 0, None, None, 1, 0, None) == EINVAL
    assert h.mdqe_label_centroids_u8(None, 1, 8, 8, 2, 0, None, None, 2, 0, None) == ENULL
    assert h.mdqe_label_centroids_u8(None, 0, 8, 8, 2, 0, None, None, 2, 0, None) == 0
    assert h.mdqe_render_trails_u8(None, 1, 8, 8, 0, None, 64, 0, 1, 0, 2, None, None) == EINVAL
    assert h.mdqe_render_trails_u8(None, 1, 8, 8, 0, None, 64, 0, 1, 4, 6, None, None) == EINVAL
    assert h.mdqe_render_trails_u8(None, 1, 8, 8, 0, None, 64, 0, 1, 4, 2, None, None) == ENULL
    assert h.mdqe_render_trails_yuv420sp(None, 8, 64, None, 8, 32, 1, 8, 8, 2, 0, None, 64, 0, 1, 4, 2, None, None) == EINVAL
    assert h.mdqe_render_trails_yuv420sp(None, 8, 64, None, 8, 32, 1, 8, 8, 0, 0, None, 64, 0, 0, 4, 2, None, None) == 0


# ---- the wrappers' refusals ------------------------------------------------------------------------------------------------------------
def test_wrapper_argument_checks():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    lab = torch.zeros(2, 6, 9, dtype=torch.uint8)
    for bad in (lab.float(), lab[:, :, :8], torch.zeros(2, 6, 9, 1, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="label_centroids: labels must be contiguous uint8"):
            ops.label_centroids(bad, 3)
    with pytest.raises(RuntimeError, match=r"Ho, Wo must be in 1\.\.16384"):
        ops.label_centroids(torch.zeros(1, 1, 16385, dtype=torch.uint8), 3)
    for n in (-1, 256, 3.0, True):
        with pytest.raises(RuntimeError, match="n must be an int in 0..255"):
            ops.label_centroids(lab, n)
    for kw, what in (({"min_area": -1}, "min_area"), ({"min_area": 1.5}, "min_area"), ({"p_off": -1}, "p_off"), ({"p_off": True}, "p_off")):
        with pytest.raises(RuntimeError, match="%s must be an int" % what):
            ops.label_centroids(lab, 3, **kw)
    for mom in (torch.zeros(3, 2, 3), torch.zeros(3, 2, 3, dtype=torch.int32), torch.zeros(2, 2, 3, dtype=torch.int64),
                torch.zeros(3, 2, 6, dtype=torch.int64)[..., ::2], torch.zeros(2, 3, 3, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="mom must be contiguous int64"):
            ops.label_centroids(lab, 3, mom=mom)
    for pts in (torch.zeros(3, 2, 2), torch.zeros(2, 2, 2, dtype=torch.int32), torch.zeros(3, 1, 2, dtype=torch.int32),
                torch.zeros(3, 2, 3, dtype=torch.int32), torch.zeros(3, 2, 4, dtype=torch.int32)[..., ::2], torch.zeros(3, 2, 2, dtype=torch.int64)):
        with pytest.raises(RuntimeError, match="pts must be int32"):
            ops.label_centroids(lab, 3, pts=pts)
    with pytest.raises(RuntimeError, match="pts must be int32"):         # p_off moves the columns past the table's end
        ops.label_centroids(lab, 3, pts=torch.zeros(3, 2, 2, dtype=torch.int32), p_off=1)
    # shapes and dtypes first, devices after (a host without a GPU gets as far as the device check)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor on the labels' device"):
        ops.label_centroids(lab, 3, mom=torch.zeros(3, 2, 3, dtype=torch.int64), pts=torch.zeros(3, 5, 2, dtype=torch.int32), p_off=3)

    pic = torch.zeros(2, 6, 9, 3, dtype=torch.uint8)
    pts = torch.zeros(3, 7, 2, dtype=torch.int32)
    pal = torch.zeros(256, 3, dtype=torch.uint8)
    for n in (-1, 256, 3.0, True):
        with pytest.raises(RuntimeError, match="n must be an int in 0..255"):
            ops.render_trails(pic, pts, n, pal, 2)
    for kw, what in (({"trail": 0}, "trail"), ({"trail": 65}, "trail"), ({"width": 0}, "width"), ({"width": 6}, "width"), ({"width": 2.0}, "width"),
                     ({"f_off": -1}, "f_off"), ({"p_off": -1}, "p_off"), ({"trail": True}, "trail")):
        with pytest.raises(RuntimeError, match="%s must be an int" % what):
            ops.render_trails(pic, pts, 3, pal, 2, **kw)
    with pytest.raises(RuntimeError, match="F must be an int"):
        ops.render_trails(pic, pts, 3, pal, -1)
    for bad in (pts.float(), pts[:2], pts[:, :, :1], torch.zeros(3, 7, 4, dtype=torch.int32)[..., ::2]):
        with pytest.raises(RuntimeError, match="pts must be int32"):
            ops.render_trails(pic, bad, 3, pal, 2)
    with pytest.raises(RuntimeError, match="pts must be int32"):         # p_off + F columns are needed
        ops.render_trails(pic, pts, 3, pal, 2, p_off=6)
    for bad in (pal.to(torch.int16), pal[:255], torch.zeros(256, 6, dtype=torch.uint8)[:, ::2]):
        with pytest.raises(RuntimeError, match="palette must be contiguous uint8"):
            ops.render_trails(pic, pts, 3, bad, 2)
    for bad in (pic.float(), pic[..., :2], torch.zeros(2, 6, 18, 3, dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(RuntimeError, match="pic must be contiguous uint8"):
            ops.render_trails(bad, pts, 3, pal, 2)
    with pytest.raises(RuntimeError, match="must hold frames f_off"):
        ops.render_trails(pic, pts, 3, pal, 2, f_off=1)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor on pic's device"):
        ops.render_trails(pic, pts, 3, pal, 2)
    pal_y = torch.zeros(256, 3, dtype=torch.uint16)
    with pytest.raises(RuntimeError, match="yuv must be a preprocess.YuvFrames"):
        ops.render_trails_yuv(pic, pts, 3, pal_y, 2)
    with pytest.raises(RuntimeError, match="palette must be contiguous uint16"):
        ops.render_trails_yuv(YuvFrames.empty(2, 6, 9), pts, 3, pal, 2)
    with pytest.raises(RuntimeError, match="the call needs f_off"):
        ops.render_trails_yuv(YuvFrames.empty(2, 6, 9), pts, 3, pal_y, 2, f_off=1)
    with pytest.raises(RuntimeError, match="must be on a HIP device"):
        ops.render_trails_yuv(YuvFrames.empty(2, 6, 9), pts, 3, pal_y, 2)


# ---- the point table's bookkeeping, on the host ------------------------------------------------------------------------------------------
def test_path_table_moves_its_history_blanks_new_rows_and_stitches(monkeypatch):
    from mdqe_cvpr2023_amd import merge, ops
    calls = []

    def centroids(labels, n, min_area, mom, pts, p_off):              # a stand-in kernel: frame f of row k is at (100 * k + frame id, min_area)
        calls.append((tuple(labels.shape), n, min_area, p_off))
        for f in range(labels.shape[0]):
            for k in range(n):
                pts[k, p_off + f] = torch.tensor([100 * k + int(labels[f, 0, 0]), min_area], dtype=torch.int32)
        mom.fill_(7)
    monkeypatch.setattr(ops, "label_centroids", centroids)
    t = merge.PathTable(3, 5, "cpu", keep=True)
    frame = 0
    seen = []
    for n, nf in ((2, 4), (3, 2), (3, 5), (0, 1), (4, 2)):            # rows appear over the windows; a window shorter than the trail; one without tracks
        cen, mom = t.begin(n, nf)
        assert tuple(cen.shape) == (n, nf, 2) and tuple(mom.shape) == (n, nf, 3) and tuple(t.pts.shape[::2]) == (255, 2) and t.pts.shape[1] >= 3 + nf
        lab = torch.arange(frame, frame + nf, dtype=torch.uint8).view(nf, 1, 1).expand(nf, 2, 2).contiguous()
        t.run(torch.cat([torch.zeros(1, 2, 2, dtype=torch.uint8), lab]), 1)
        t.keep(frame)
        seen.append((frame, n, nf))
        # the window's columns, and in front of them the three frames before it -- absent for a row the earlier windows did not hold
        for k in range(4):
            first = min([f0 for f0, rows, _ in seen if rows > k] or [10 ** 6])
            want = [[100 * k + f, 5] if f >= first and f >= 0 and k < n_at(seen, f) else [-1, -1] for f in range(frame - 3, frame + nf)]
            assert t.pts[k, :3 + nf].tolist() == want, (n, nf, k)
        frame += nf
    assert calls == [((4, 2, 2), 2, 5, 3), ((2, 2, 2), 3, 5, 3), ((5, 2, 2), 3, 5, 3), ((2, 2, 2), 4, 5, 3)]          # (no rows: no call)
    res = merge.path_result([2, 0, 2], 14, [(f, nf, n, c, m) for f, nf, n, c, m in t.windows])
    assert tuple(res["pred_centroids"].shape) == (3, 14, 2) and res["pred_centroids"].dtype == torch.int32
    assert tuple(res["pred_moments"].shape) == (3, 14, 3) and res["pred_moments"].dtype == torch.int64
    assert res["pred_centroids"][1, :, 0].tolist() == list(range(11)) + [-1, 12, 13]                 # row 0: every frame but the empty window's
    assert res["pred_centroids"][0, :, 0].tolist() == [-1] * 4 + [200 + f for f in range(4, 11)] + [-1, 212, 213]    # row 2 appears at frame 4
    assert torch.equal(res["pred_centroids"][0], res["pred_centroids"][2])
    assert res["pred_moments"][0, :, 0].tolist() == [0] * 4 + [7] * 7 + [0, 7, 7]
    empty = merge.path_result([], 14, t.windows)
    assert tuple(empty["pred_centroids"].shape) == (0, 14, 2) and tuple(empty["pred_moments"].shape) == (0, 14, 3)
    # which videos get a table
    from mdqe_cvpr2023_amd.render import Style
    F = merge.Forms
    assert merge.path_table(F(overlay=True, labels=True), Style(), "cpu") is None and merge.path_table(F(planes="dense"), Style(trail=4), "cpu") is None
    t = merge.path_table(F(overlay=True, labels=True), Style(trail=4, min_area=9), "cpu")
    assert (t.trail, t.min_area, t.windows) == (4, 9, None)
    t = merge.path_table(F(planes="dense", paths=True), Style(trail=4, min_area=9), "cpu", keep=True)
    assert (t.trail, t.min_area, t.windows) == (0, 0, [])


def n_at(seen, f):
    """The rows of the window that holds frame f."""
    at = 0
    for f0, n, nf in seen:
        if f0 <= f < f0 + nf:
            return n
    return at


# ---- the session's and the model's refusals, on stand-ins ------------------------------------------------------------------------------
def _standin(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)

    def check():
        from mdqe_cvpr2023_amd.meta_arch import MDQE
        MDQE.check_label_capacity(types.SimpleNamespace(cfg=cfg))
    return types.SimpleNamespace(cfg=cfg, device=torch.device("cuda", 0), check_label_capacity=check)


def test_online_session_takes_paths_beside_every_emit_and_refuses_what_it_cannot_do():
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.online import Window
    for emit in ("masks", "rle", "labels", "overlay"):
        ov = MDQE.online_video(_standin(), emit=emit, paths=True)
        assert ov.paths is True and ov.frames_held == 0
        f = Forms.of_emit(emit, paths=True)
        assert f.paths and f == dataclasses.replace(Forms.of_emit(emit), paths=True)
    assert MDQE.online_video(_standin(), emit="masks").paths is False and not Forms.of_emit("masks").paths
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="paths must be a bool"):
            MDQE.online_video(_standin(), emit="masks", paths=bad)
    with pytest.raises(ValueError, match="COCO image config.*video config"):
        MDQE.online_video(_standin(is_coco=True), emit="masks", paths=True)
    with pytest.raises(ValueError, match="n_max_inst.*exceeds 255"):    # more tracks than the label map has rows for
        MDQE.online_video(_standin(n_max_inst=256), emit="masks", paths=True)
    assert [f.name for f in dataclasses.fields(Window)] == ["frames", "track_ids", "cls_probs", "masks", "rles", "boxes", "areas"]
    w = Window(frames=(0, 2), track_ids=[0], cls_probs=torch.zeros(1, 2), centroids="c", moments="m")
    assert (w.centroids, w.moments, w.crops, w.labels) == ("c", "m", None, None)
    w = Window(frames=(0, 2), track_ids=[0], cls_probs=torch.zeros(1, 2))
    assert w.centroids is None and w.moments is None


def test_model_path_output_round_trips_resolves_into_the_forms_and_is_refused_where_it_cannot_run():
    from mdqe_cvpr2023_amd import sharding
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    m = MDQE(PRESETS["R50_ovis_360"], seed=1)
    assert m.path_output is False and not Forms.of_model(m).paths and Forms.of_model(m) == Forms(planes="dense")
    m.path_output = True
    for attrs, planes, labels in (({}, "dense", False), ({"rle_output": True}, "rle", False), ({"label_output": True}, "dense", True),
                                  ({"label_output": "only"}, None, True)):
        for k, v in attrs.items():
            setattr(m, k, v)
        f = Forms.of_model(m)
        assert f.paths and f.planes == planes and f.labels == labels and not f.overlay and not f.crops
        assert not Forms.of_model(m, emit_masks=False).paths
        for k in attrs:
            setattr(m, k, False)
    assert m._frame_source(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), None) is None    # (the paths need no frames)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="path_output must be False or True"):
            m.path_output = bad
    m.path_output = False
    assert Forms.of_model(m) == Forms(planes="dense")
    with pytest.raises(ValueError, match="n_max_inst.*exceeds 255"):
        MDQE(dataclasses.replace(PRESETS["R50_ovis_360"], n_max_inst=256), seed=1).path_output = True
    # a COCO image config
    coco = types.SimpleNamespace(cfg=dataclasses.replace(m.cfg, is_coco=True), engine=None, device=torch.device("cpu"), path_output=True)
    with pytest.raises(ValueError, match="COCO image branch has no paths.*video config"):
        MDQE.inference_image(coco, [{"image": torch.zeros(3, 3, 8, 8)}])
    # the sharded driver
    geo = types.SimpleNamespace(Hp=8, Wp=8, N=4)
    model = types.SimpleNamespace(cfg=m.cfg, device=torch.device("cpu"), engine=types.SimpleNamespace(geometry=lambda h, w: geo), path_output=True)
    with pytest.raises(ValueError, match="path_output is not offered by the sharded driver.*one device"):
        sharding.run_round_robin(model, {0: torch.zeros(4, 3, 8, 8)}, [(0, 0, 4)], 0, 1, None, (8, 8))
