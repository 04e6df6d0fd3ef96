"""Track outlines on the device: mdqe_label_polygons_u8 (ops.label_polygons, csrc/polygons.hip) against the sequential tracer of
tests/_polygon_ref.py -- xy, all five ring columns and the totals, exactly; the caps and their guard bands; the rounds of the ranking
on a ring of thousands of corners; the moments of ops.label_centroids as an independent count; and the layers above the kernel:
forward() with model.polygon_output on both mask paths, online_video(polygons=...).  Integers only: every comparison is exact.

The mark kernel's tile is TILE_W x TILE_H = 64 x 16 lattice vertices, and a picture of H x W pixels has (H + 1) x (W + 1) of them:
15 x 63 pixels fill one tile exactly, 16 x 64 cross it by one vertex each way, 14 x 62 are one short of it."""
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

import _polygon_ref as REF  # noqa: E402

TILE_W, TILE_H = 64, 16
GUARD = 0x5A5A5A5A


def _run(lab, n, min_area=0, cap_vertices=None, cap_rings=None):
    """ops.label_polygons on a numpy map -> (xy [V, 2], rings [R, 5], totals) on the host, cut to the totals where they fit the caps."""
    from mdqe_cvpr2023_amd import ops
    dev = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint8)).cuda()
    F, H, W = dev.shape
    if cap_vertices == "all":                                         # what no map can exceed: noise has far more corners than masks
        cap_vertices, cap_rings = 4 * F * (H + 1) * (W + 1) + 1, F * H * W + 1
    xy, rings, totals = ops.label_polygons(dev, n, min_area, cap_vertices, cap_rings)
    assert xy.dtype == rings.dtype == totals.dtype == torch.int32 and xy.is_cuda and rings.is_cuda and totals.is_cuda
    V, R = totals.cpu().tolist()
    return xy.cpu().numpy()[:V], rings.cpu().numpy()[:R], (V, R)


def _check(lab, n, min_area=0, cap_vertices="all", cap_rings=None):
    lab = np.asarray(lab, dtype=np.uint8)
    if lab.ndim == 2:
        lab = lab[None]
    want_xy, want_rings = REF.trace(lab, n, min_area)
    xy, rings, (V, R) = _run(lab, n, min_area, cap_vertices, cap_rings)
    assert (V, R) == (len(want_xy), len(want_rings)), (lab.shape, n, min_area, V, R)
    assert np.array_equal(rings, want_rings), (lab.shape, n, min_area)
    assert np.array_equal(xy, want_xy), (lab.shape, n, min_area)
    return want_xy, want_rings


def _nested(size, depth, label=1):
    lab = np.zeros((size, size), dtype=np.uint8)
    for d in range(depth):
        lab[2 * d:size - 2 * d, 2 * d:size - 2 * d] = label if d % 2 == 0 else 0
    return lab


def _comb(size):
    """A staircase outline: a spine down column 0 with a tooth on every third row, each tooth with one-pixel steps above it on the odd
    columns and below it on the even ones -- a single 4-connected region whose outer ring turns at nearly every lattice vertex."""
    lab = np.zeros((size, size), dtype=np.uint8)
    lab[:, 0] = 1
    lab[1::3, :] = 1
    lab[0::3, 1::2] = 1
    lab[2::3, 2::2] = 1
    return lab


HAND = {
    "pixel": (np.array([[1]]), 1),
    "ring": (np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]]), 1),
    "diagonal_one_label": (np.array([[1, 0], [0, 1]]), 1),
    "diagonal_two_labels": (np.array([[1, 0], [0, 2]]), 2),
    # a hole that touches the outside diagonally: the ring around the hole's corner visits a vertex twice
    "pinch": (np.array([[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 1]]), 1),
}


def test_hand_written_cases():
    xy, rings = _check(*HAND["pixel"])
    assert xy.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]] and rings.tolist() == [[0, 0, 0, 4, 0]]
    xy, rings = _check(*HAND["ring"])
    assert rings.tolist() == [[0, 0, 0, 4, 0], [0, 0, 4, 4, 1]] and xy[4].tolist() == [1, 1] and xy[5].tolist() == [1, 2]
    xy, rings = _check(*HAND["diagonal_one_label"])
    assert rings[:, [0, 3, 4]].tolist() == [[0, 4, 0], [0, 4, 0]] and [1, 1] in xy[:4].tolist() and [1, 1] in xy[4:].tolist()
    xy, rings = _check(*HAND["diagonal_two_labels"])
    assert rings[:, [0, 3, 4]].tolist() == [[0, 4, 0], [1, 4, 0]]
    xy, rings = _check(*HAND["pinch"])
    assert len(rings) == 1 and xy.tolist().count([1, 1]) == 2         # one ring: the "hole" opens to the outside through the pinch


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1)])
def test_smallest_maps(shape):
    _check(np.ones(shape), 1)
    _check(np.zeros(shape), 1)
    lab = np.arange(shape[0] * shape[1]).reshape(shape) % 3
    _check(lab, 2)
    _check(lab, 1)


def test_one_label_fills_the_picture():
    xy, rings = _check(np.full((2, 9, 13), 3), 3, cap_vertices=None)      # (the default caps)
    assert xy.tolist() == [[0, 0], [13, 0], [13, 9], [0, 9]] * 2 and rings[:, 1].tolist() == [0, 1]


def test_checkerboards_the_most_corners_per_pixel():
    yy, xx = np.mgrid[:8, :8]
    for phase in (0, 1):
        xy, rings = _check(((yy + xx + phase) % 2), 1)
        assert len(rings) == 32 and len(xy) == 128
    four = 1 + (yy % 2) * 2 + (xx % 2)                                # every inner vertex meets 4 labels
    xy, rings = _check(four, 4)
    assert len(rings) == 64
    _check(four, 3)


def test_nested_rings_to_depth_three():
    lab = _nested(15, 3)
    xy, rings = _check(lab, 1, cap_vertices=None)
    assert rings[:, 4].tolist().count(1) == 1 and len(rings) == 3
    lab2 = lab.copy()
    lab2[lab == 0] = 2                                                # the gaps are a second label: its rings nest between
    _check(lab2, 2)


@pytest.mark.parametrize("H,W", [(TILE_H - 2, TILE_W - 2), (TILE_H - 1, TILE_W - 1), (TILE_H, TILE_W), (2 * TILE_H, 2 * TILE_W + 1)])
def test_sizes_around_the_tile(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    lab = rng.integers(0, 4, size=(2, H, W)) * (rng.random((2, H, W)) < 0.7)
    lab[0, -1, :] = 1                                                 # runs along the last row and column, across the tile's edge
    lab[0, :, -1] = 1
    _check(lab, 3)
    _check(np.ones((1, H, W)), 1)


def test_a_straight_run_longer_than_a_tile():
    lab = np.zeros((3, 200), dtype=np.uint8)
    lab[1, 3:199] = 1
    xy, rings = _check(lab, 1, cap_vertices=None)
    assert xy.tolist() == [[3, 1], [199, 1], [199, 2], [3, 2]]
    _check(np.ones((3, 200)), 1)
    _check(np.ones((200, 3)), 1)


def test_frames_with_different_content_and_an_empty_one():
    rng = np.random.default_rng(5)
    lab = rng.integers(0, 3, size=(3, 11, 17))
    lab[1] = 0
    xy, rings = _check(lab, 2)
    assert set(rings[:, 1].tolist()) == {0, 2}


def test_labels_above_n_are_not_regions():
    rng = np.random.default_rng(6)
    lab = rng.integers(0, 6, size=(2, 12, 19))
    for n in (5, 3, 1):
        xy, rings = _check(lab, n)
        assert int(rings[:, 0].max()) == n - 1
    lab[lab == 2] = 255
    _check(lab, 4)
    _check(lab, 255)


def test_nothing_to_trace():
    from mdqe_cvpr2023_amd import ops
    xy, rings, totals = _run(np.ones((2, 5, 6)), 0)
    assert totals == (0, 0)
    t = ops.label_polygons(torch.zeros((0, 5, 6), dtype=torch.uint8, device="cuda"), 3)[2]
    assert t.cpu().tolist() == [0, 0]
    assert _run(np.zeros((2, 5, 6)), 3)[2] == (0, 0)


def test_min_area_at_the_size_and_one_above():
    lab = np.zeros((2, 9, 9), dtype=np.uint8)
    lab[0, 1:4, 1:5] = 1                                              # 12 pixels
    lab[0, 6:8, 6:8] = 2                                              # 4
    lab[1, 1:3, 1:3] = 1                                              # 4: the same label, another frame
    lab[1, 5:8, 2:6] = 2                                              # 12
    for min_area, want in ((0, 4), (1, 4), (4, 4), (5, 2), (12, 2), (13, 0)):
        xy, rings = _check(lab, 2, min_area)
        assert len(rings) == want, min_area


@pytest.mark.parametrize("seed", range(20))
def test_random_maps(seed):
    rng = np.random.default_rng(seed)
    dens = (0.3, 0.5, 0.8)[seed % 3]
    lab = rng.integers(1, 7, size=(2, 37, 53)) * (rng.random((2, 37, 53)) < dens)
    if seed % 2:                                                      # blobs beside the noise: long runs, holes
        for _ in range(6):
            y0, x0 = int(rng.integers(0, 30)), int(rng.integers(0, 45))
            lab[int(rng.integers(0, 2)), y0:y0 + int(rng.integers(2, 20)), x0:x0 + int(rng.integers(2, 25))] = int(rng.integers(1, 6))
    _check(lab, 5, min_area=(0, 3)[seed % 4 == 3])


def _direct(lab, n, cap_vertices, cap_rings, pad=64):
    """The C entry with buffers of this test's own: `pad` guard rows behind xy and rings."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    dev = torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint8)).cuda()
    F, Ho, Wo = dev.shape
    xy = torch.full((cap_vertices + pad, 2), GUARD, dtype=torch.int32, device="cuda")
    rings = torch.full((cap_rings + pad, 5), GUARD, dtype=torch.int32, device="cuda")
    totals = torch.full((2 + pad,), GUARD, dtype=torch.int32, device="cuda")
    need = lib.mdqe_label_polygons_workspace(F, Ho, Wo, cap_vertices)
    ws = ops._workspace(need, dev.device)
    check(lib.mdqe_label_polygons_u8(ptr(dev), F, Ho, Wo, n, 0, cap_vertices, cap_rings, ptr(xy), ptr(rings), ptr(totals), ptr(ws), ws.numel(),
                                     cur_stream(dev.device)), "label_polygons")
    return xy.cpu().numpy(), rings.cpu().numpy(), totals.cpu().numpy()


def test_caps_one_below_the_counts_keep_the_totals_true_and_the_guards_whole():
    rng = np.random.default_rng(11)
    lab = rng.integers(0, 4, size=(2, 21, 30)) * (rng.random((2, 21, 30)) < 0.6)
    want_xy, want_rings = REF.trace(lab, 3)
    V, R = len(want_xy), len(want_rings)
    assert V > 200 and R > 40
    for cv, cr, fits in ((V, R, True), (V - 1, R, False), (V, R - 1, False), (V - 1, R - 1, False), (4, 1, False), (1, 1, False)):
        xy, rings, totals = _direct(lab, 3, cv, cr)
        assert totals[:2].tolist() == [V, R], (cv, cr)
        assert (totals[2:] == GUARD).all() and (xy[cv:] == GUARD).all() and (rings[cr:] == GUARD).all(), (cv, cr)
        if fits:
            assert np.array_equal(xy[:V], want_xy) and np.array_equal(rings[:R], want_rings)
    # ops.label_polygons reports the same totals through its own buffers
    assert _run(lab, 3, cap_vertices=V - 1)[2] == (V, R) and _run(lab, 3, cap_rings=R - 1)[2] == (V, R)


def test_a_workspace_that_is_too_small_is_refused():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import cur_stream, lib, ptr
    dev = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    need = lib.mdqe_label_polygons_workspace(1, 8, 8, 64)
    assert need > 0 and lib.mdqe_label_polygons_workspace(1, 8, 8, 0) == -1
    ws = ops._workspace(need, dev.device)
    out = torch.zeros((64, 5), dtype=torch.int32, device="cuda")
    args = (ptr(dev), 1, 8, 8, 1, 0, 64, 12, ptr(out), ptr(out), ptr(out), ptr(ws))
    assert lib.mdqe_label_polygons_u8(*args, need - 1, cur_stream(dev.device)) == 1      # MDQE_EINVAL
    assert lib.mdqe_label_polygons_u8(*args, need, cur_stream(dev.device)) == 0


def test_one_ring_of_thousands_of_corners_and_identical_bytes_twice():
    lab = _comb(70)
    want_xy, want_rings = REF.trace(lab[None], 1)
    assert int(want_rings[:, 3].max()) > 4096                        # one ring: the ranking has to double past 2^12
    a = _run(lab[None], 1, cap_vertices="all")
    assert np.array_equal(a[0], want_xy) and np.array_equal(a[1], want_rings)
    b = _run(lab[None], 1, cap_vertices="all")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_area_sums_are_twice_the_moments_of_label_centroids():
    from mdqe_cvpr2023_amd import ops
    rng = np.random.default_rng(21)
    lab = (rng.integers(1, 6, size=(3, 40, 61)) * (rng.random((3, 40, 61)) < 0.7)).astype(np.uint8)
    lab[1, 5:30, 10:50] = 2
    n = 5
    xy, rings, _ = _run(lab, n, cap_vertices="all")
    mom = ops.label_centroids(torch.from_numpy(lab).cuda(), n, pts=False)[0].cpu().numpy()
    a2 = np.zeros((n, 3), dtype=np.int64)
    for k, f, first, cnt, hole in rings.tolist():
        part = REF.area2(xy[first:first + cnt])
        assert (part < 0) == bool(hole)
        a2[k, f] += part
    assert np.array_equal(a2, 2 * mom[:, :, 0]) and int(mom[:, :, 0].min()) > 0


# ---- the model -----------------------------------------------------------------------------------------------------------------------
from test_overlay_gpu import L, PLANS, _forward, _model, _online, _same  # noqa: E402


def _expected(label_map, inst, spec, out_size):
    """The reference on the run's own label map, after rle.labels_keep: rows renumbered to the outputs, `every` applied."""
    from mdqe_cvpr2023_amd import rle
    from mdqe_cvpr2023_amd.polygons import TrackPolygons, select_rings
    kept = rle.labels_keep(label_map.numpy(), inst)
    xy, rings = REF.trace(kept, int(kept.max()), spec.min_area)
    xy, rings = select_rings(xy, rings, rings[:, 1] % spec.every == 0)
    rings[:, 0] = [inst.index(k) for k in rings[:, 0].tolist()]
    return TrackPolygons(xy, rings, out_size)


@pytest.fixture(scope="module")
def video():
    """The fixture of test_paths_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5 frames, many tracks -- the plain
    run every case here compares with and the reference's polygons of its label map, once."""
    from bench import synth_video
    from mdqe_cvpr2023_amd.polygons import Polygons
    _, model = _model(n_frames_window_test=6, apply_cls_thres=1e-6)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    base = _forward(model, frames, label_output=True)
    inst = base["pred_track_ids"]
    want = {every: _expected(base["pred_label_map"], inst, Polygons(every=every), (90, 150)) for every in (1, 2)}
    print("tracks:", len(set(inst)), "rings:", len(want[1]), "vertices:", len(want[1].xy), "holes:", int(want[1].rings[:, 4].sum()))
    assert len(want[1]) > 20 and len(set(want[1].rings[:, 1].tolist())) == L
    return model, frames, base, want


def _with_polygons(model, frames, spec, **attrs):
    model.polygon_output = spec
    try:
        return _forward(model, frames, **attrs)
    finally:
        model.polygon_output = None


class _Calls:
    """Every ops function a run calls, by name and in order."""

    def __init__(self, monkeypatch):
        import types
        from mdqe_cvpr2023_amd import ops
        self.names = []
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and not name.startswith("_") and fn.__module__ == ops.__name__:
                monkeypatch.setattr(ops, name, self._counted(name, fn))

    def _counted(self, name, fn):
        def call(*a, **kw):
            self.names.append(name)
            return fn(*a, **kw)
        return call

    def take(self):
        names, self.names = self.names, []
        return names


def test_polygon_output_on_both_mask_paths_and_nothing_else_changes(video, monkeypatch):
    from mdqe_cvpr2023_amd.polygons import Polygons, TrackPolygons
    model, frames, base, want = video
    calls = _Calls(monkeypatch)
    got = {}
    for early in (True, False):
        plain = _forward(model, frames, label_output=True, early_masks=early)
        parent = calls.take()
        assert "label_polygons" not in parent and _same(plain, base)  # the defaults: exactly the launches of before
        got[early] = _with_polygons(model, frames, Polygons(), label_output=True, early_masks=early)
        ours = calls.take()
        assert [c for c in ours if c != "label_polygons"] == parent   # the same calls in the same order, and between them ...
        assert 3 <= ours.count("label_polygons") <= 6                 # ... one per window, and one more where its caps overflowed
        assert set(got[early]) == set(base) | {"pred_polygons"}
        assert isinstance(got[early]["pred_polygons"], TrackPolygons) and got[early]["pred_polygons"] == want[1], early
        for k in base:                                                # every other key keeps its bits
            assert _same(got[early][k], base[k]), (early, k)
    assert got[True]["pred_polygons"] == got[False]["pred_polygons"]  # both mask paths agree
    # without the label map the outlines are the same and the map stays a scratch; every / min_area reach the kernel and the filter
    alone = _with_polygons(model, frames, Polygons(every=2))
    assert alone["pred_polygons"] == want[2] and "pred_label_map" not in alone and alone["pred_track_ids"] == base["pred_track_ids"]
    assert "pred_polygons" not in _forward(model, frames)
    tp = got[True]["pred_polygons"]
    lab = base["pred_label_map"].numpy()
    for k, t in enumerate(base["pred_track_ids"]):
        if base["pred_track_ids"].index(t) == k:
            for f in (0, 7, L - 1):
                assert np.array_equal(tp.rasterize(k, f), lab[f] == t + 1)   # the round trip


def test_online_windows_with_polygons_concatenate_to_the_offline_run(video):
    from mdqe_cvpr2023_amd.polygons import Polygons, TrackPolygons
    model, frames, base, want = video
    spec = Polygons(every=2)
    for sizes in (PLANS[0], PLANS[2]):
        ov, wins, _ = _online(model, frames, sizes, emit="rle", polygons=spec, keep=True)
        assert [w.frames for w in wins] == [(0, 6), (6, 12), (12, 17)]
        for w in wins:
            assert isinstance(w.polygons, TrackPolygons) and w.polygons.size == (90, 150)
            fs = set(w.polygons.rings[:, 1].tolist())
            assert fs and fs <= set(range(w.frames[0] + w.frames[0] % 2, w.frames[1], 2))
            assert int(w.polygons.rings[:, 0].max()) < len(w.track_ids)
        res = ov.result()
        inst = res["pred_track_ids"]
        assert inst == base["pred_track_ids"] and res["pred_polygons"] == want[2], sizes
        table = {}
        for j, t in enumerate(inst):
            table.setdefault(t, j)
        assert TrackPolygons.concat([w.polygons.renumbered(table) for w in wins]) == want[2]
    ov, wins, _ = _online(model, frames, PLANS[0], emit="rle", polygons=spec)
    assert "pred_polygons" not in ov.result() and wins[0].polygons is not None
    ov, wins, _ = _online(model, frames, PLANS[0], emit="rle")
    assert all(w.polygons is None for w in wins)


def test_an_overlay_session_with_polygons_keeps_the_overlays_bytes(video):
    from mdqe_cvpr2023_amd.polygons import Polygons
    model, frames, base, want = video
    _, plain, _ = _online(model, frames, PLANS[2], emit="overlay")
    ov, wins, _ = _online(model, frames, PLANS[2], emit="overlay", polygons=Polygons(), keep=True)
    assert torch.equal(torch.cat([w.overlay for w in wins]), torch.cat([w.overlay for w in plain]))
    assert torch.equal(torch.cat([w.labels for w in wins]), base["pred_label_map"])
    assert ov.result()["pred_polygons"] == want[1]
