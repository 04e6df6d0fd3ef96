"""Track outlines without a GPU: the sequential tracer of tests/_polygon_ref.py against hand-written rings and the rule's invariants on
seeded random maps; polygons.polygons_from_labels against it, ring for ring; polygons.TrackPolygons and polygons.Polygons; how the
option resolves into merge.Forms; ops.label_polygons' argument errors; the header; and the refusals on stand-in models."""
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

import _polygon_ref as REF  # noqa: E402


def _maps():
    """200 seeded random maps of at most 13 x 15 with 1..3 labels at densities 0.3 / 0.5 / 0.8, traced once."""
    if not _maps.cache:
        for seed in range(200):
            rng = np.random.default_rng(seed)
            H, W, nl = int(rng.integers(1, 14)), int(rng.integers(1, 16)), int(rng.integers(1, 4))
            lab = (rng.integers(1, nl + 1, size=(1, H, W)) * (rng.random((1, H, W)) < (0.3, 0.5, 0.8)[seed % 3])).astype(np.uint8)
            _maps.cache.append((lab, nl, REF.trace(lab, nl)))
    return _maps.cache


_maps.cache = []


# ---- the reference against hand-written expectations ----------------------------------------------------------------------------------
def test_reference_single_pixel():
    xy, rings = REF.trace(np.array([[[1]]], dtype=np.uint8), 1)
    assert xy.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]] and rings.tolist() == [[0, 0, 0, 4, 0]]


def test_reference_block_with_its_centre_cleared():
    lab = np.ones((1, 3, 3), dtype=np.uint8)
    lab[0, 1, 1] = 0
    xy, rings = REF.trace(lab, 1)
    assert rings.tolist() == [[0, 0, 0, 4, 0], [0, 0, 4, 4, 1]]
    assert xy[:4].tolist() == [[0, 0], [3, 0], [3, 3], [0, 3]]
    assert xy[4:].tolist() == [[1, 1], [1, 2], [2, 2], [2, 1]]        # the hole starts at (1, 1) heading S
    assert REF.area2(xy[:4]) == 18 and REF.area2(xy[4:]) == -2


def test_reference_diagonal_pixels_of_one_and_of_two_labels():
    one = np.array([[[1, 0], [0, 1]]], dtype=np.uint8)
    xy, rings = REF.trace(one, 1)
    assert rings.tolist() == [[0, 0, 0, 4, 0], [0, 0, 4, 4, 0]]       # regions are 4-connected: two rings that share the vertex (1, 1)
    assert xy.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1], [1, 1], [2, 1], [2, 2], [1, 2]]
    two = np.array([[[1, 0], [0, 2]]], dtype=np.uint8)
    xy2, rings2 = REF.trace(two, 2)
    assert np.array_equal(xy2, xy) and rings2.tolist() == [[0, 0, 0, 4, 0], [1, 0, 4, 4, 0]]
    assert REF.trace(two, 1)[1].tolist() == [[0, 0, 0, 4, 0]]         # a label above n is not a region


def test_reference_pinch_visits_a_vertex_twice():
    lab = np.array([[[0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 1]]], dtype=np.uint8)
    xy, rings = REF.trace(lab, 1)
    assert rings.tolist() == [[0, 0, 0, 10, 0]] and xy.tolist().count([1, 1]) == 2
    assert REF.area2(xy) == 2 * int(lab.sum())


# ---- the invariants ---------------------------------------------------------------------------------------------------------------------
def test_invariants_on_random_maps():
    from mdqe_cvpr2023_amd.polygons import TrackPolygons
    n_rings = n_holes = 0
    for lab, nl, (xy, rings) in _maps():
        tp = TrackPolygons(xy, rings, lab.shape[1:])
        for k, f, first, cnt, hole in rings.tolist():
            assert cnt % 2 == 0 and cnt >= 4
            assert (REF.area2(xy[first:first + cnt]) < 0) == bool(hole)
            n_rings += 1
            n_holes += hole
        for k in range(nl):
            region = lab[0] == k + 1
            assert tp.area2(k, 0) == 2 * int(region.sum())
            assert np.array_equal(tp.rasterize(k, 0), region)
    assert n_rings > 2000 and n_holes > 10


def test_polygons_from_labels_is_the_reference_ring_for_ring():
    from mdqe_cvpr2023_amd.polygons import polygons_from_labels
    for lab, nl, (xy, rings) in _maps():
        got = polygons_from_labels(lab, nl)
        assert np.array_equal(got.xy, xy) and np.array_equal(got.rings, rings) and got.size == tuple(lab.shape[1:])
        assert got.xy.dtype == np.int32 and got.rings.dtype == np.int32
    # several frames, a tensor, labels above n, min_area
    rng = np.random.default_rng(7)
    lab = (rng.integers(1, 6, size=(3, 12, 14)) * (rng.random((3, 12, 14)) < 0.6)).astype(np.uint8)
    lab[1] = 0
    for n, min_area in ((5, 0), (3, 0), (5, 4), (0, 0)):
        xy, rings = REF.trace(lab, n, min_area)
        got = polygons_from_labels(torch.from_numpy(lab), n, min_area)
        assert np.array_equal(got.xy, xy) and np.array_equal(got.rings, rings), (n, min_area)
    with pytest.raises(ValueError, match=r"\[F, H, W\]"):
        polygons_from_labels(lab[0], 3)


# ---- TrackPolygons ----------------------------------------------------------------------------------------------------------------------
def _two_frames():
    from mdqe_cvpr2023_amd.polygons import polygons_from_labels
    lab = np.zeros((2, 5, 6), dtype=np.uint8)
    lab[0, 0:3, 0:3] = 1
    lab[0, 1, 1] = 0                                                  # a hole
    lab[0, 4, 4:6] = 2
    lab[1, 2:4, 1:5] = 2
    return lab, polygons_from_labels(lab, 2)


def test_track_polygons_accessors():
    from mdqe_cvpr2023_amd.polygons import TrackPolygons
    lab, tp = _two_frames()
    assert len(tp) == 4 and tp.size == (5, 6) and "4 rings" in repr(tp)
    of = tp.of(0, 0)
    assert [h for _, h in of] == [False, True] and of[0][0].tolist() == [[0, 0], [3, 0], [3, 3], [0, 3]]
    assert tp.of(0, 1) == [] and tp.of(7, 0) == []
    assert tp.has_holes(0, 0) and not tp.has_holes(1, 0) and not tp.has_holes(0, 1)
    assert tp.to_coco(0, 0) == [[0.0, 0.0, 3.0, 0.0, 3.0, 3.0, 0.0, 3.0]]      # the hole is dropped
    assert tp.to_coco(1, 1) == [[1.0, 2.0, 5.0, 2.0, 5.0, 4.0, 1.0, 4.0]] and tp.to_coco(0, 1) == []
    assert tp.area2(0, 0) == 16 and tp.area2(1, 0) == 4 and tp.area2(1, 1) == 16 and tp.area2(0, 1) == 0
    for k in range(2):
        for f in range(2):
            assert np.array_equal(tp.rasterize(k, f), lab[f] == k + 1)
    assert tp == TrackPolygons(tp.xy.copy(), tp.rings.copy(), (5, 6)) and tp != TrackPolygons(tp.xy, tp.rings, (5, 7))


def test_track_polygons_concat_and_renumbering():
    from mdqe_cvpr2023_amd.polygons import TrackPolygons, polygons_from_labels
    lab, tp = _two_frames()
    a, b = polygons_from_labels(lab[:1], 2), polygons_from_labels(lab[1:], 2).renumbered(f0=1)
    assert TrackPolygons.concat([a, b]) == tp
    assert TrackPolygons.concat([tp]) == tp and len(TrackPolygons.concat([], size=(5, 6))) == 0
    with pytest.raises(ValueError, match="no parts and no size"):
        TrackPolygons.concat([])
    with pytest.raises(ValueError, match="different sizes"):
        TrackPolygons.concat([tp, TrackPolygons(tp.xy, tp.rings, (9, 9))])
    # rows renumbered to the outputs: row 1 -> output 0, row 0 dropped
    sel = tp.renumbered({1: 0})
    assert sel.rings[:, 0].tolist() == [0, 0] and sel.rings[:, 1].tolist() == [0, 1] and sel.rings[:, 2].tolist() == [0, 4] and len(sel.xy) == 8
    assert np.array_equal(sel.rasterize(0, 1), lab[1] == 2)
    assert tp.renumbered([None, 3]).rings[:, 0].tolist() == [3, 3]


def test_polygon_result_maps_rows_to_the_first_output_and_drops_the_rest():
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.polygons import polygons_from_labels
    lab, tp = _two_frames()
    parts = [polygons_from_labels(lab[:1], 2), polygons_from_labels(lab[1:], 2).renumbered(f0=1)]
    res = merge.polygon_result([1, 1], (5, 6), parts)["pred_polygons"]
    assert res == tp.renumbered({1: 0})
    res = merge.polygon_result([4, 0, 1], (5, 6), parts)["pred_polygons"]
    assert res == tp.renumbered({0: 1, 1: 2})
    assert len(merge.polygon_result([], (5, 6), parts)["pred_polygons"]) == 0
    assert merge.polygon_result([0], (5, 6), [])["pred_polygons"].size == (5, 6)


# ---- the request ------------------------------------------------------------------------------------------------------------------------
def test_polygons_validation():
    from mdqe_cvpr2023_amd.polygons import Polygons
    p = Polygons()
    assert (p.min_area, p.every, p.classes) == (0, 1, None)
    assert Polygons(classes=[3, 1, 3]).classes == (1, 3) and Polygons(min_area=7, every=2).every == 2
    for bad in (-1, 1.5, True, "3", 2 ** 31):
        with pytest.raises(ValueError, match="min_area"):
            Polygons(min_area=bad)
    for bad in (0, -2, 1.0, True, None):
        with pytest.raises(ValueError, match="every"):
            Polygons(every=bad)
    for bad in (3, "12", [1, -1], [True], [1.0]):
        with pytest.raises(ValueError, match="classes"):
            Polygons(classes=bad)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.every = 3


def test_every_and_classes_filter_the_ring_records():
    from mdqe_cvpr2023_amd.polygons import Polygons, select_rings
    rings = np.array([[0, 0, 0, 4, 0], [1, 0, 4, 6, 0], [0, 1, 10, 4, 1], [2, 2, 14, 4, 0], [1, 3, 18, 4, 0]], dtype=np.int32)
    xy = np.arange(44, dtype=np.int32).reshape(22, 2)
    cls = torch.tensor([[0.1, 0.9, 0.2], [0.8, 0.8, 0.1], [0.0, 0.1, 0.7]])   # first maxima: 1, 0, 2
    assert Polygons().keep(rings, 0, cls, 3).tolist() == [True] * 5
    assert Polygons(every=2).keep(rings, 0, cls, 3).tolist() == [True, True, False, True, False]
    assert Polygons(every=2).keep(rings, 5, cls, 3).tolist() == [False, False, True, False, True]     # the window starts at video frame 5
    assert Polygons(classes=[0, 2]).keep(rings, 0, cls, 3).tolist() == [False, True, False, True, True]
    assert Polygons(classes=[1], every=3).keep(rings, 0, cls, 3).tolist() == [True, False, False, False, False]
    assert Polygons(classes=[5]).rows(cls, 3).tolist() == [False] * 3 and Polygons().rows(None, 2).tolist() == [True, True]
    with pytest.raises(ValueError, match="class rows"):
        Polygons(classes=[1]).rows(None, 2)
    sx, sr = select_rings(xy, rings, Polygons(classes=[0, 2]).keep(rings, 0, cls, 3))
    assert sr.tolist() == [[1, 0, 0, 6, 0], [2, 2, 6, 4, 0], [1, 3, 10, 4, 0]]
    assert sx.tolist() == xy[4:10].tolist() + xy[14:22].tolist()
    ex, er = select_rings(xy, rings, np.zeros(5, dtype=bool))
    assert ex.shape == (0, 2) and er.shape == (0, 5) and ex.dtype == er.dtype == np.int32


# ---- the forms --------------------------------------------------------------------------------------------------------------------------
def test_forms_resolution():
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.polygons import Polygons
    assert Forms().polygons is False and Forms(planes="dense") == Forms(planes="dense", polygons=False)
    for emit in ("masks", "rle", "labels", "overlay"):
        f = Forms.of_emit(emit, polygons=True)
        assert f.polygons and f == dataclasses.replace(Forms.of_emit(emit), polygons=True)
        assert not Forms.of_emit(emit).polygons
    bare = types.SimpleNamespace()
    assert Forms.of_model(bare) == Forms(planes="dense")              # a stand-in without the flag: the defaults, unchanged
    m = types.SimpleNamespace(polygon_output=Polygons(every=2))
    assert Forms.of_model(m) == Forms(planes="dense", polygons=True) and Forms.of_model(m, emit_masks=False) == Forms()
    m.label_output = "only"
    assert Forms.of_model(m) == Forms(planes=None, labels=True, polygons=True)
    m.polygon_output = None
    assert not Forms.of_model(m).polygons


# ---- the op's argument checks ---------------------------------------------------------------------------------------------------------
def test_label_polygons_argument_errors_on_the_host():
    from mdqe_cvpr2023_amd import ops
    lab = torch.zeros((2, 4, 5), dtype=torch.uint8)
    for bad in (lab.float(), lab[0], lab.transpose(1, 2), "x"):
        with pytest.raises(RuntimeError, match="labels must be contiguous uint8"):
            ops.label_polygons(bad, 1)
    with pytest.raises(RuntimeError, match="Ho, Wo must be in 1..16384"):
        ops.label_polygons(torch.zeros((1, 0, 5), dtype=torch.uint8), 1)
    for bad in (-1, 256, 1.0, True):
        with pytest.raises(RuntimeError, match="n must be an int in 0..255"):
            ops.label_polygons(lab, bad)
    for bad in (-1, 2 ** 31, 0.5, False):
        with pytest.raises(RuntimeError, match="min_area must be an int"):
            ops.label_polygons(lab, 1, bad)
    for bad in (0, 2 ** 26 + 1, 1.0, True):
        with pytest.raises(RuntimeError, match="cap_vertices must be an int in 1.."):
            ops.label_polygons(lab, 1, 0, bad)
    for bad in (0, 2 ** 24 + 1, 2.0, True):
        with pytest.raises(RuntimeError, match="cap_rings must be an int in 1.."):
            ops.label_polygons(lab, 1, 0, 16, bad)
    with pytest.raises(RuntimeError, match="labels must be a CUDA tensor"):   # the devices come after everything a host can check
        ops.label_polygons(lab, 1)


# ---- the header and the binding -------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_abi_stays_6():
    from mdqe_cvpr2023_amd import _lib
    text = open(os.path.join(ROOT, "include", "mdqe_hip.h")).read()
    assert re.search(r"#define MDQE_ABI_VERSION 6\b", text) and _lib.ABI_VERSION == 6
    decl = re.search(r"int mdqe_label_polygons_u8\(([^;]*)\);", text)
    assert decl is not None
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["labels", "F", "Ho", "Wo", "n", "min_area", "cap_vertices", "cap_rings", "xy", "rings",
                                                         "totals", "workspace", "workspace_bytes", "stream"]
    assert len(_lib.SIGNATURES["mdqe_label_polygons_u8"]) == len(args)
    assert re.search(r"long mdqe_label_polygons_workspace\(int F, int Ho, int Wo, int cap_vertices\);", text)
    for word in ("right turn before straight on before the left", "E < S < W < N", "heading out is S"):
        assert word in text, word                                     # the rule is in the comment
    lib = os.path.join(ROOT, "mdqe_cvpr2023_amd", "csrc", "libmdqe_hip.so")
    if os.path.exists(lib):
        assert _lib.load_library().mdqe_abi_version() == 6


# ---- the refusals, on stand-ins -------------------------------------------------------------------------------------------------------
def _standin(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)

    def check():
        from mdqe_cvpr2023_amd.meta_arch import MDQE
        MDQE.check_label_capacity(types.SimpleNamespace(cfg=cfg))
    return types.SimpleNamespace(cfg=cfg, device=torch.device("cuda", 0), check_label_capacity=check)


def test_online_session_takes_polygons_beside_every_emit_and_refuses_what_it_cannot_do():
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.online import Window
    from mdqe_cvpr2023_amd.polygons import Polygons
    spec = Polygons(every=2)
    for emit in ("masks", "rle", "labels", "overlay"):
        ov = MDQE.online_video(_standin(), emit=emit, polygons=spec)
        assert ov.polygons is spec and ov.frames_held == 0
    assert MDQE.online_video(_standin(), emit="masks").polygons is None
    for bad in (True, "yes", 3):
        with pytest.raises(ValueError, match="polygons must be a polygons.Polygons"):
            MDQE.online_video(_standin(), emit="masks", polygons=bad)
    with pytest.raises(ValueError, match="COCO image config.*video config"):
        MDQE.online_video(_standin(is_coco=True), emit="masks", polygons=spec)
    with pytest.raises(ValueError, match="n_max_inst.*exceeds 255"):    # more tracks than the label map has rows for
        MDQE.online_video(_standin(n_max_inst=256), emit="masks", polygons=spec)
    assert [f.name for f in dataclasses.fields(Window)] == ["frames", "track_ids", "cls_probs", "masks", "rles", "boxes", "areas"]
    w = Window(frames=(0, 2), track_ids=[0], cls_probs=torch.zeros(1, 2), polygons="p")
    assert w.polygons == "p" and w.centroids is None
    assert Window(frames=(0, 2), track_ids=[0], cls_probs=torch.zeros(1, 2)).polygons is None


def test_model_polygon_output_round_trips_and_is_refused_where_it_cannot_run():
    from mdqe_cvpr2023_amd import sharding
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.polygons import Polygons
    m = MDQE(PRESETS["R50_ovis_360"], seed=1)
    assert m.polygon_output is None and Forms.of_model(m) == Forms(planes="dense")
    spec = Polygons(min_area=4)
    m.polygon_output = spec
    assert m.polygon_output is spec and Forms.of_model(m) == Forms(planes="dense", polygons=True)
    assert m._frame_source(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), None) is None    # (the outlines need no frames)
    for bad in (True, 1, "yes"):
        with pytest.raises(ValueError, match="polygon_output must be None or a polygons.Polygons"):
            m.polygon_output = bad
    m.polygon_output = None
    assert Forms.of_model(m) == Forms(planes="dense")
    with pytest.raises(ValueError, match="n_max_inst.*exceeds 255"):
        MDQE(dataclasses.replace(PRESETS["R50_ovis_360"], n_max_inst=256), seed=1).polygon_output = spec
    # a COCO image config
    coco = types.SimpleNamespace(cfg=dataclasses.replace(m.cfg, is_coco=True), engine=None, device=torch.device("cpu"), polygon_output=spec)
    with pytest.raises(ValueError, match="COCO image branch has no polygons.*video config"):
        MDQE.inference_image(coco, [{"image": torch.zeros(3, 3, 8, 8)}])
    # the sharded driver
    geo = types.SimpleNamespace(Hp=8, Wp=8, N=4)
    model = types.SimpleNamespace(cfg=m.cfg, device=torch.device("cpu"), engine=types.SimpleNamespace(geometry=lambda h, w: geo), polygon_output=spec)
    with pytest.raises(ValueError, match="polygon_output is not offered by the sharded driver.*one device"):
        sharding.run_round_robin(model, {0: torch.zeros(4, 3, 8, 8)}, [(0, 0, 4)], 0, 1, None, (8, 8))
