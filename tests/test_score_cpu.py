"""Scoring against ground truth, the host side: GroundTruth's packed form (dense and RLE input, more than 32 tracks, a result as a pseudo
ground truth), YTVISScorer against the naive scorer of tests/_score_ref.py on seeded random integer tables and on hand-derived anchors,
the refusals that need no launch (the binding's argument checks, the entry point's size checks, the sharded driver, the image branch),
and the ABI entry.  No GPU."""
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

import _score_ref as REF  # noqa: E402


# ---- GroundTruth ---------------------------------------------------------------------------------------------------------------------
def _tracks(G, L, H, W, seed):
    """Overlapping random rectangles per (track, frame); track 1 is absent on frames 1..2, track 0 is all-set on frame 0."""
    rng = np.random.default_rng(seed)
    m = np.zeros((G, L, H, W), dtype=np.uint8)
    for g in range(G):
        for f in range(L):
            y0, x0 = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 1))
            m[g, f, y0:y0 + int(rng.integers(1, H)), x0:x0 + int(rng.integers(1, W))] = 1
    if G > 1:
        m[1, 1:3] = 0
    if G:
        m[0, 0] = 1
    return m


def _unpack(gt):
    words = [w.view(torch.int32).numpy().view(np.uint32) for w in gt.words]
    return np.stack([(words[g // 32] >> np.uint32(g % 32)) & np.uint32(1) for g in range(gt.G)]).astype(np.uint8) if gt.G else None


@pytest.mark.parametrize("G", [1, 5, 32, 40])
def test_ground_truth_from_rles_equals_ground_truth_from_masks(G):
    from mdqe_cvpr2023_amd import rle as R
    from mdqe_cvpr2023_amd.vis_score import GroundTruth
    L, H, W = 4, 9, 13
    m = _tracks(G, L, H, W, seed=G)
    rles = [[R.encode_dense(m[g, f]) if m[g, f].any() else None for f in range(L)] for g in range(G)]
    if G > 2:                                                           # the uncompressed form (a list of run lengths) is accepted too
        c, _ = R.strings_to_counts([rles[2][0]["counts"]])
        rles[2][0] = {"size": [H, W], "counts": c.tolist()}
    cats = list(range(1, G + 1))
    a = GroundTruth(masks=torch.from_numpy(m), category_ids=cats)
    b = GroundTruth(rles=rles, size=(H, W), category_ids=cats)
    assert a.G == b.G == G and a.length == b.length == L and a.size == b.size == (H, W)
    assert len(a.words) == len(b.words) == -(-G // 32) == (2 if G == 40 else 1)
    for x, y in zip(a.words, b.words):
        assert x.dtype == y.dtype == torch.uint32 and tuple(x.shape) == (L, H, W)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert np.array_equal(_unpack(a), m) and np.array_equal(_unpack(b), m)          # bit 31 and the second group included
    want = m.reshape(G, L, -1).sum(2)
    assert a.gt_area.dtype == torch.int64 and np.array_equal(a.gt_area.numpy(), want) and torch.equal(a.gt_area, b.gt_area)
    assert np.array_equal(a.areas, want) and a.iscrowd == [0] * G and a.ids == cats
    on = a.on("cpu")
    assert len(on) == len(a.words) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(on, a.words))
    # the annotation's areas are kept beside the masks' own counts
    ann = [[7 if v else None for v in row] for row in want]
    c = GroundTruth(masks=m, category_ids=cats, areas=ann, iscrowd=[1] + [0] * (G - 1))
    assert np.array_equal(c.areas, np.where(want > 0, 7, 0)) and np.array_equal(c.gt_area.numpy(), want) and c.iscrowd[0] == 1


def test_ground_truth_refuses_what_it_cannot_hold():
    from mdqe_cvpr2023_amd.vis_score import GroundTruth
    m = np.zeros((2, 3, 4, 5), dtype=np.uint8)
    for kw, what in (({}, "masks or rles"), ({"masks": m, "rles": [[None] * 3] * 2}, "masks or rles"), ({"masks": m[0]}, r"\[G, L, H, W\]"),
                     ({"masks": m, "size": (5, 4)}, "size"), ({"masks": m, "category_ids": [1]}, "category_ids"),
                     ({"rles": [[None] * 3, [None] * 2]}, "per frame"), ({"rles": [[None] * 3]}, "size")):
        kw.setdefault("category_ids", [1, 2] if "masks" in kw and kw["masks"] is m else [1] * len(kw.get("rles", [])))
        with pytest.raises(ValueError, match=what):
            GroundTruth(**kw)
    e = GroundTruth(rles=[], size=(4, 5))                                # a video without annotated objects
    assert e.G == 0 and e.words == [] and tuple(e.gt_area.shape) == (0, 0)


def test_decode_dense_inverts_encode_dense():
    from mdqe_cvpr2023_amd import rle as R
    rng = np.random.default_rng(0)
    for shape in ((1, 1), (7, 5), (16, 33)):
        for p in (0.0, 0.3, 1.0):
            m = (rng.random(shape) < p).astype(np.uint8)
            d = R.decode_dense(R.encode_dense(m))
            assert d.dtype == np.uint8 and np.array_equal(d, m)
    with pytest.raises(ValueError, match="runs cover"):
        R.decode_dense({"size": [2, 2], "counts": [1, 2]})


@pytest.mark.parametrize("form", ["pred_masks", "pred_rles"])
def test_from_result_round_trips(form):
    from mdqe_cvpr2023_amd import rle as R
    from mdqe_cvpr2023_amd.vis_score import GroundTruth
    m = _tracks(3, 4, 9, 13, seed=7)
    res = {"image_size": (9, 13), "pred_scores": [0.9, 0.2, 0.6], "pred_labels": [4, 1, 4]}
    if form == "pred_masks":
        res["pred_masks"] = [torch.from_numpy(x).bool() for x in m]
    else:
        res["pred_rles"] = [[R.encode_dense(fm) for fm in x] for x in m]
    gt = GroundTruth.from_result(res)
    assert gt.category_ids == [4, 1, 4] and np.array_equal(_unpack(gt), m) and gt.size == (9, 13) and gt.length == 4
    gt = GroundTruth.from_result(res, score_thr=0.5)
    assert gt.category_ids == [4, 4] and np.array_equal(_unpack(gt), m[[0, 2]])
    assert GroundTruth.from_result(res, score_thr=0.95).G == 0


# ---- YTVISScorer against the naive scorer --------------------------------------------------------------------------------------------
AREAS = [0, 0, 900, 5000, 128 ** 2 - 1, 128 ** 2, 128 ** 2 + 1, 30000, 256 ** 2, 256 ** 2 + 1, 90000]
SCORES = [0.9, 0.9, 0.75, 0.5, 0.5, 0.31, 0.05]


def _random_case(seed):
    """Integer tables only: 1-4 videos of 2-3 frames, 1-3 categories, 0-4 ground-truth tracks and 0-12 predictions a video, tied scores,
    crowd flags, per-frame areas on both sides of the 128^2 / 256^2 limits, overlaps anywhere from none to the whole smaller side."""
    rng = np.random.default_rng(seed)
    n_cat = int(rng.integers(1, 4))
    videos = {}
    for vid in range(int(rng.integers(1, 5))):
        L, G, n = int(rng.integers(2, 4)), int(rng.integers(0, 5)), int(rng.integers(0, 13))
        ga = rng.choice(AREAS, size=(G, L))
        pa = rng.choice(AREAS, size=(n, L))
        cap = np.minimum(pa.sum(1)[:, None], ga.sum(1)[None]) if n and G else np.zeros((n, G), dtype=np.int64)
        frac = rng.choice([0.0, 0.3, 0.55, 0.8, 0.97, 1.0], size=(n, G))
        ann = ga.copy()
        if G and seed % 3 == 0:                                          # an annotation whose areas differ from the masks' counts
            ann[0] = rng.choice(AREAS, size=L)
        videos["v%d" % vid if seed % 2 else vid] = {
            "scores": [float(s) for s in rng.choice(SCORES, size=n)], "labels": [int(c) for c in rng.integers(1, n_cat + 1, size=n)],
            "inter": np.floor(cap * frac).astype(np.int64), "pred_area": pa.astype(np.int64), "gt_area": ga.astype(np.int64),
            "gt_cats": [int(c) for c in rng.integers(1, n_cat + 1, size=G)], "crowd": [int(c) for c in rng.random(G) < 0.2], "gt_ann_area": ann}
    return videos, list(range(1, n_cat + 1))


def _score(videos, cats=None):
    from mdqe_cvpr2023_amd.vis_score import YTVISScorer
    sc = YTVISScorer(category_ids=cats)
    for vid, v in videos.items():
        sc.add_tables(vid, v["scores"], v["labels"], v["inter"], v["pred_area"], v["gt_area"], v["gt_cats"], v["crowd"], v["gt_ann_area"])
    return sc.evaluate()


@pytest.mark.parametrize("seed", range(50))
def test_scorer_equals_the_naive_scorer_on_random_tables(seed):
    from mdqe_cvpr2023_amd.vis_score import STAT_NAMES
    videos, cats = _random_case(seed)
    got = _score(videos, cats)
    stats, precision, recall = REF.evaluate(videos, cats)
    assert got["precision"].shape == precision.shape == (10, 101, len(cats), 4, 3) and got["recall"].shape == recall.shape
    assert np.array_equal(got["precision"], precision) and np.array_equal(got["recall"], recall)
    assert got["stats"].dtype == np.float64 and np.array_equal(got["stats"], stats), (got["stats"], stats)
    assert [got[n] for n in STAT_NAMES] == stats.tolist() and got["category_ids"] == cats
    # the default category axis (every category named) gives the same 12 numbers: a category nobody names is -1 and drops out
    assert np.array_equal(_score(videos)["stats"], stats)


def _one(scores, labels, inter, pa, ga, cats, **kw):
    return _score({0: dict({"scores": scores, "labels": labels, "inter": np.array(inter).reshape(len(scores), len(cats)),
                            "pred_area": np.array(pa).reshape(len(scores), np.array(ga).shape[1]), "gt_area": np.array(ga), "gt_cats": cats,
                            "crowd": [0] * len(cats), "gt_ann_area": np.array(ga)}, **kw)})


ONE = 1.0 / (1.0 + np.spacing(1))        # a precision of tp / (tp + 0 + eps) with tp = 1: 1 - 2^-52


def test_anchor_predictions_identical_to_the_ground_truth():
    """Two categories with one track each, over two frames; the predictions ARE the ground truth: inter = area, IoU 1 at every threshold.
    Category 1's track has per-frame areas (100, 0) -> avg_area 100 (the zero frame does not count): small.  Category 2's: (70000, 80000)
    -> 75000 > 256^2: large.  Each category has one true positive and nothing else: recall 1 at every threshold, precision
    1 / (1 + eps) = 1 - 2^-52 at every recall level (the reference's own guard against 0 / 0), so every AP is 1 to within the rounding
    of a mean of such values (asserted to 1e-12; the entries themselves are asserted exactly).  No medium track exists: -1."""
    out = _one([0.9, 0.8], [1, 2], [[100, 0], [0, 150000]], [[100, 0], [70000, 80000]], [[100, 0], [70000, 80000]], [1, 2])
    want = [ONE, ONE, ONE, ONE, -1, ONE, 1.0, 1.0, 1.0, 1.0, -1, 1.0]
    assert out["stats"].tolist() == pytest.approx(want, abs=1e-12) and abs(ONE - 1.0) < 3e-16
    assert [out["stats"][i] for i in (4, 10)] == [-1, -1] and out["stats"][6:10].tolist() == [1.0] * 4
    assert (out["precision"][:, :, 0, 2, :] == -1).all() and (out["precision"][:, :, 0, 1, :] == ONE).all()


def test_anchor_no_predictions():
    """One small ground-truth track, nothing predicted: every recall is 0 and the precision at every recall level is 0 (no detection
    reaches it); the medium and large classes hold no track: -1."""
    out = _one([], [], np.zeros((0, 1)), np.zeros((0, 2)), [[100, 120]], [3])
    assert out["stats"].tolist() == [0, 0, 0, 0, -1, -1, 0, 0, 0, 0, -1, -1]


def test_anchor_three_predictions_two_tracks_by_hand():
    """One category, one frame, two ground-truth tracks g1, g2 of 100 pixels each (small).  Three predictions, best score first:
        p1 (0.9): 78 pixels, all inside g1            -> IoU(p1, g1) = 78 / 100 = 0.78
        p2 (0.8): 50 pixels, 20 in g1 and 10 in g2    -> IoU 20 / 130 and 10 / 140: below every threshold, a false positive throughout
        p3 (0.7): 62 pixels, all inside g2            -> IoU(p3, g2) = 62 / 100 = 0.62
    Thresholds 0.50, 0.55, 0.60 (three): TP, FP, TP.  tp = 1, 1, 2; fp = 0, 1, 1; recall 0.5, 0.5, 1; precision 1, 1/2, 2/3, whose
    envelope is 1, 2/3, 2/3.  The 51 recall levels 0 .. 0.50 read 1 (eps aside), the 50 levels 0.51 .. 1 read 2/3: (51 + 100/3) / 101.
    Thresholds 0.65, 0.70, 0.75 (three): TP, FP, FP.  Recall stays 0.5: levels 0 .. 0.50 read 1, the rest nothing (0): 51 / 101.
    Thresholds 0.80 .. 0.95 (four): three false positives: 0.
    AP50 = (51 + 100/3) / 101 = 0.834983..., AP75 = 51 / 101 = 0.504950..., AP = (3 * AP50 + 3 * AP75) / 10.
    Recall at up to 100 (or 10) predictions: 1, 1, 1, 0.5, 0.5, 0.5, 0, 0, 0, 0 -> 0.45; with the best prediction only (p1): 0.5 at six
    thresholds -> 0.3.  Everything is small: APs = AP, ARs = AR100; no medium or large track: -1."""
    out = _one([0.9, 0.8, 0.7], [1, 1, 1], [[78, 0], [20, 10], [0, 62]], [[78], [50], [62]], [[100], [100]], [1, 1])
    ap50, ap75 = (51 + 100 / 3) / 101, 51 / 101
    ap = (3 * ap50 + 3 * ap75) / 10
    want = [ap, ap50, ap75, ap, -1, -1, 0.3, 0.45, 0.45, 0.45, -1, -1]
    assert ap50 != ap75 and out["stats"].tolist() == pytest.approx(want, abs=1e-12)
    assert [out["stats"][i] for i in (4, 5, 10, 11)] == [-1] * 4


def test_scorer_needs_pred_gt_and_takes_a_result():
    from mdqe_cvpr2023_amd.vis_score import GroundTruth, YTVISScorer, iou_table
    m = np.zeros((2, 1, 10, 10), dtype=np.uint8)
    m[0, 0, :, :5], m[1, 0, :, 5:] = 1, 1
    gt = GroundTruth(masks=m, category_ids=[1, 1])
    sc = YTVISScorer()
    with pytest.raises(ValueError, match="pred_gt"):
        sc.add(0, {"pred_scores": [], "pred_labels": []}, gt)
    inter, pa = np.array([[50, 0], [10, 40]]), np.array([[50], [50]])
    iou = iou_table(inter, pa, gt.gt_area.numpy())
    assert iou.dtype == np.float64 and iou.tolist() == [[1.0, 0.0], [10 / 90, 40 / 60]]
    assert iou_table(np.zeros((1, 1)), np.zeros((1, 3)), np.zeros((1, 3))).tolist() == [[0.0]]      # an empty union is 0, not NaN
    sc.add(0, {"pred_scores": [0.9, 0.8], "pred_labels": [1, 1], "pred_gt": {"inter": inter, "pred_area": pa, "gt_area": gt.gt_area}}, gt)
    with pytest.raises(ValueError, match="added already"):
        sc.add(0, {"pred_scores": [], "pred_labels": [], "pred_gt": {"inter": np.zeros((0, 2)), "pred_area": np.zeros((0, 1)), "gt_area": gt.gt_area}}, gt)
    out = sc.evaluate()
    assert out["AP50"] == pytest.approx(1.0, abs=1e-12) and out["AP75"] == pytest.approx(51 / 101, abs=1e-12) and out["AR1"] == 0.5


# ---- refusals that need no launch ----------------------------------------------------------------------------------------------------
def _gt(L=4, H=8, W=8):
    from mdqe_cvpr2023_amd.vis_score import GroundTruth
    return GroundTruth(masks=np.zeros((1, L, H, W), dtype=np.uint8), category_ids=[1])


def test_the_sharded_driver_and_the_image_branch_refuse_ground_truth():
    from mdqe_cvpr2023_amd import sharding
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    gt = _gt()
    fr = torch.zeros(4, 3, 8, 8)
    # (a stand-in model as far as the driver looks at it before it would build its merger)
    cfg = PRESETS["R50_ovis_360"]
    geo = types.SimpleNamespace(Hp=8, Wp=8, N=4)
    model = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"), engine=types.SimpleNamespace(geometry=lambda h, w: geo))
    with pytest.raises(ValueError, match="ground_truth is not offered by the sharded driver"):
        sharding.run_round_robin(model, {0: fr}, [(0, 0, 4)], 0, 1, None, (8, 8), ground_truth=gt)
    with pytest.raises(ValueError, match="ground_truth is not offered by the sharded driver"):
        next(sharding.run_round_robin_stream(model, [({0: fr}, [(0, 0, 4)])], 0, 1, None, (8, 8), ground_truth=gt))
    coco = types.SimpleNamespace(cfg=dataclasses.replace(PRESETS["R50_ovis_360"], is_coco=True), engine=None, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="image branch"):
        MDQE.inference_image(coco, [{"image": fr, "ground_truth": gt}])


def test_the_video_paths_refuse_a_ground_truth_that_does_not_fit():
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    gt = _gt(L=4, H=8, W=8)
    assert MDQE._ground_truth({"image": None}) is None
    assert MDQE._ground_truth({"ground_truth": gt}, (8, 8), 4) is gt
    with pytest.raises(ValueError, match="size"):
        MDQE._ground_truth({"ground_truth": gt}, (8, 9), 4)
    with pytest.raises(ValueError, match="frames"):
        MDQE._ground_truth({"ground_truth": gt}, (8, 8), 5)
    with pytest.raises(ValueError, match="GroundTruth"):
        MDQE._ground_truth({"ground_truth": np.zeros((1, 4, 8, 8))}, (8, 8), 4)
    model = types.SimpleNamespace(overlay_output=False, geometry_output=False, label_output=False)
    with pytest.raises(ValueError, match="frames"):
        merge.ClipMerger(model, (8, 8), (8, 8), (2, 2), n_frames=5, ground_truth=gt)
    # a model on the host: refused by name, before anything of the device is touched
    model.device = torch.device("cpu")
    with pytest.raises(ValueError, match="ground_truth: .*the model is on cpu"):
        merge.ClipMerger(model, (8, 8), (8, 8), (2, 2), n_frames=4, ground_truth=gt)
    with pytest.raises(ValueError, match="GroundTruth"):
        MDQE.online_video(types.SimpleNamespace(), ground_truth=np.zeros((1, 4, 8, 8)))


def test_the_binding_checks_its_arguments_before_any_launch():
    from mdqe_cvpr2023_amd import ops
    lg = torch.zeros(2, 3, 4, 6)
    idx = torch.zeros(2, dtype=torch.int32)
    bits = torch.zeros(4, 16, 24, dtype=torch.int32).view(torch.uint32)
    inter = torch.zeros(2, 8, dtype=torch.int64)

    def call(logits=lg, inst_idx=idx, gt_bits=bits, G=5, f_off=0, inter=inter, area=None):
        return ops.final_masks_overlap(logits, inst_idx, 4, 16, 24, 16, 24, gt_bits, G, f_off, inter, area)
    with pytest.raises(RuntimeError, match="gt_bits holds 4 frames, the window needs f_off \\+ Fw = 5"):
        call(f_off=2)
    with pytest.raises(RuntimeError, match="gt_bits holds 2 frames"):
        call(gt_bits=bits[:2])
    for kw, what in (({"logits": lg[0]}, "logits"), ({"inst_idx": idx.long()}, "inst_idx"), ({"gt_bits": bits.view(torch.int32)}, "gt_bits"),
                     ({"gt_bits": bits[:, :, :20]}, "gt_bits"), ({"f_off": -1}, "gt_bits"), ({"inter": inter.int()}, "inter"),
                     ({"inter": inter[:1]}, "inter"), ({"G": 9}, "inter"), ({"area": torch.zeros(5, dtype=torch.int32)}, "area"),
                     ({}, "gt_bits must be a CUDA tensor")):
        with pytest.raises(RuntimeError, match="final_masks_overlap: " + what):
            call(**kw)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)


def test_abi_declares_exports_and_binds_the_overlap_entry_point():
    from mdqe_cvpr2023_amd import _lib
    name = "mdqe_final_masks_overlap"
    src = _header()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
    assert hasattr(h, name) and name in _lib.SIGNATURES
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == 18
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # no existing entry changed
    fn = h.mdqe_final_masks_overlap

    def call(n_sel=1, Fw=1, Ho=4, Wo=4, G=5, f_off=0, stride=8):
        # NULL everywhere: the size checks come before any pointer is looked at, so a refusal launches nothing
        return fn(None, n_sel, None, Fw, 2, 2, 4, 4, 4, Ho, Wo, None, G, f_off, None, stride, None, None)
    assert call(G=0) == 1 and call(G=33) == 1 and call(G=5, stride=4) == 1 and call(f_off=-1) == 1          # MDQE_EINVAL
    assert call(Ho=0) == 1 and call(Ho=60000, Wo=60000) == 1
    assert call(G=32, stride=32) == 3 and call(G=1, stride=1) == 3                                            # sizes fine: MDQE_ENULL
    assert call(n_sel=0) == 0 and call(Fw=0) == 0                                                             # OK, nothing launched
    assert call(n_sel=0, G=33) == 1                                                                           # (sizes are checked first)
