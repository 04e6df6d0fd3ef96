"""Per-frame track boxes and areas, the host side: the ABI carries the two geometry entry points, the RLE / dense helpers agree with
the oracle's box rule (d2 BitMasks.get_bounding_boxes) and a plain pixel count, and the YTVIS annotation writer has the layout the
reference's loader reads (mdqe/data/datasets/ytvis.py:260-306).  All comparisons are exact."""
import dataclasses
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

NEW = ("mdqe_final_masks_u8_geom", "mdqe_final_masks_rle_geom")


def test_abi_declares_exports_and_binds_the_geometry_entry_points():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n + " is not declared in mdqe_hip.h"
        assert hasattr(h, n), n + " is not exported"
        assert n in _lib.SIGNATURES, n + " is not bound"
    assert len(_lib.SIGNATURES["mdqe_final_masks_u8_geom"]) == len(_lib.SIGNATURES["mdqe_final_masks_u8"]) + 1
    assert len(_lib.SIGNATURES["mdqe_final_masks_rle_geom"]) == len(_lib.SIGNATURES["mdqe_final_masks_rle"]) + 1
    assert h.mdqe_abi_version() == 6
    from mdqe_cvpr2023_amd import ops
    assert callable(ops.final_masks_geom) and callable(ops.final_masks_rle_geom)


def _cases():
    """Random blobs plus the corner cases, over ordinary sizes and height / width 1."""
    rng = np.random.default_rng(7)
    out = []
    for h, w in ((7, 9), (1, 13), (13, 1), (1, 1), (40, 33), (90, 150)):
        for t in range(6):
            m = np.zeros((h, w), bool)
            for _ in range(int(rng.integers(1, 4))):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
                m[y0:y0 + int(rng.integers(1, h + 1)), x0:x0 + int(rng.integers(1, w + 1))] = True
            if t >= 4:
                m = m & (rng.random((h, w)) > 0.4)                  # ragged: many short runs
            out.append(m)
        out.append(rng.random((h, w)) > 0.5)
        out.append(np.zeros((h, w), bool))                          # empty
        out.append(np.ones((h, w), bool))                           # full
        for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):   # one pixel in each corner
            m = np.zeros((h, w), bool)
            m[y, x] = True
            out.append(m)
        m = np.zeros((h, w), bool); m[h // 2, :] = True; out.append(m)   # a one-pixel-wide row
        m = np.zeros((h, w), bool); m[:, w // 2] = True; out.append(m)   # ... and column
    return out


def test_strings_to_counts_inverts_counts_to_strings():
    import rle_oracle as RO
    from mdqe_cvpr2023_amd import rle as R
    masks = _cases()
    ref = [RO.rle_counts(m) for m in masks]
    strings = [RO.rle_to_string(c) for c in ref]
    counts, lengths = R.strings_to_counts(strings)
    assert lengths.tolist() == [len(c) for c in ref]
    assert counts.tolist() == [v for c in ref for v in c]
    assert R.counts_to_strings(counts, lengths) == strings
    counts2, lengths2 = R.strings_to_counts([s.decode("ascii") for s in strings])     # str as the model hands them out
    assert counts2.tolist() == counts.tolist() and lengths2.tolist() == lengths.tolist()
    c0, l0 = R.strings_to_counts([])
    assert c0.shape == (0,) and l0.shape == (0,)


def test_area_bbox_geometry_against_the_oracle():
    import mdqe_oracle as O
    import rle_oracle as RO
    from mdqe_cvpr2023_amd import rle as R
    masks = _cases()
    rles = [RO.encode(m) for m in masks]
    areas, boxes = R.area(rles), R.to_bbox(rles)
    assert areas.dtype == np.int64 and boxes.shape == (len(masks), 4)
    n_empty = 0
    for i, m in enumerate(masks):
        t = torch.from_numpy(m)
        want = O.mask_bounding_boxes(t[None])[0]                    # [x0, y0, x1 + 1, y1 + 1], zeros when empty
        cnt = int(m.sum())
        xywh = [float(want[0]), float(want[1]), float(want[2] - want[0]), float(want[3] - want[1])]
        assert int(areas[i]) == cnt and boxes[i].tolist() == xywh, i
        assert R.area(rles[i]) == cnt and R.to_bbox(rles[i]).tolist() == xywh          # one dict -> scalar / [4]
        g = R.geometry_dense(t)
        assert g.dtype == torch.int32 and tuple(g.shape) == (5,)
        if cnt == 0:
            n_empty += 1
            assert g.tolist() == [0, m.shape[1], m.shape[0], -1, -1]                   # xmin > xmax, ymin > ymax
        bx, ar = R.geom_to_boxes(g)
        assert bx.dtype == torch.float32 and ar.dtype == torch.int64
        assert int(ar) == cnt and torch.equal(bx, want), (i, g, want)
    assert n_empty >= 6
    # batched, any leading shape
    same = [m for m in masks if m.shape == (40, 33)]
    st = torch.from_numpy(np.stack(same)).view(3, -1, 40, 33)
    g = R.geometry_dense(st)
    assert tuple(g.shape) == (3, st.shape[1], 5)
    bx, ar = R.geom_to_boxes(g.numpy())
    assert torch.equal(bx.view(-1, 4), O.mask_bounding_boxes(st.view(-1, 40, 33)))
    assert ar.view(-1).tolist() == [int(m.sum()) for m in same]


def _outputs(L=5, H=12, W=17):
    """Three tracks: one present on every frame, one empty on frames 0 and 3, one empty everywhere (and below the threshold)."""
    m = torch.zeros(3, L, H, W, dtype=torch.bool)
    for f in range(L):
        m[0, f, 2:5 + f, 3 + f:9 + f] = True
        if f not in (0, 3):
            m[1, f, H - 1, 0] = True
            m[1, f, f, W - 1] = True
    return {"image_size": (H, W), "pred_scores": [0.9, 0.4, 0.01], "pred_labels": [3, 0, 7], "pred_masks": [m[0], m[1], m[2]]}


def test_instances_to_ytvis_annotations():
    import rle_oracle as RO
    from mdqe_cvpr2023_amd import rle as R
    dense = _outputs()
    L, (H, W) = 5, dense["image_size"]
    inputs = [{"video_id": 42}]
    recs = R.instances_to_ytvis_annotations(inputs, dense)
    assert [r["id"] for r in recs] == [1, 2, 3]
    keys = {"id", "video_id", "category_id", "iscrowd", "score", "height", "width", "length", "segmentations", "bboxes", "areas"}
    for j, r in enumerate(recs):
        assert set(r) == keys
        assert (r["video_id"], r["iscrowd"], r["height"], r["width"], r["length"]) == (42, 0, H, W, L)
        assert r["category_id"] == dense["pred_labels"][j] and r["score"] == dense["pred_scores"][j]
        assert len(r["segmentations"]) == len(r["bboxes"]) == len(r["areas"]) == L
        for f in range(L):
            mk = dense["pred_masks"][j][f]
            if not bool(mk.any()):                                   # all three None together: the loader skips this frame (:283)
                assert r["segmentations"][f] is None and r["bboxes"][f] is None and r["areas"][f] is None
                continue
            seg = r["segmentations"][f]
            assert seg["size"] == [H, W] and isinstance(seg["counts"], str)
            assert np.array_equal(RO.rle_decode(RO.rle_from_string(seg["counts"].encode()), H, W), mk.numpy())
            ys, xs = np.nonzero(mk.numpy())
            assert r["bboxes"][f] == [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]
            assert r["areas"][f] == int(mk.sum()) and isinstance(r["areas"][f], int)
    assert [f for f in range(L) if recs[1]["areas"][f] is None] == [0, 3] and recs[2]["areas"] == [None] * L
    json.loads(json.dumps(recs))                                     # JSON-serialisable as it stands

    # the same records from RLE outputs, and from outputs that carry the device geometry (bboxes = XYWH of pred_boxes)
    rle_out = {k: v for k, v in dense.items() if k != "pred_masks"}
    rle_out["pred_rles"] = [[R.encode_dense(fm.numpy()) for fm in m] for m in dense["pred_masks"]]
    assert R.instances_to_ytvis_annotations(inputs, rle_out) == recs
    bx, ar = R.geom_to_boxes(R.geometry_dense(torch.stack(dense["pred_masks"])))
    for base in (dense, rle_out):
        with_geo = dict(base, pred_boxes=list(bx), pred_areas=list(ar))
        got = R.instances_to_ytvis_annotations(inputs, with_geo)
        assert got == recs
        for j, r in enumerate(got):
            for f in range(L):
                if r["bboxes"][f] is not None:
                    x0, y0, x1, y1 = bx[j, f].tolist()
                    assert r["bboxes"][f] == [x0, y0, x1 - x0, y1 - y0]

    # score_thr drops records, ids stay consecutive from first_id
    got = R.instances_to_ytvis_annotations(inputs, dense, score_thr=0.05, first_id=100)
    assert [r["id"] for r in got] == [100, 101] and [r["category_id"] for r in got] == [3, 0]
    got = R.instances_to_ytvis_annotations(inputs, dense, score_thr=0.5, first_id=7)
    assert [r["id"] for r in got] == [7] and got[0]["segmentations"] == recs[0]["segmentations"]
    # the result writer is as it was
    res = R.instances_to_coco_json_video(inputs, rle_out)
    assert set(res[0]) == {"video_id", "score", "category_id", "segmentations"}


def test_window_fields_and_model_flag_default_off():
    import inspect
    from mdqe_cvpr2023_amd import online
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    names = [f.name for f in dataclasses.fields(online.Window)]
    assert names[:5] == ["frames", "track_ids", "cls_probs", "masks", "rles"] and names[5:] == ["boxes", "areas"]
    w = online.Window(frames=(0, 1), track_ids=[], cls_probs=torch.zeros(0, 2))
    assert w.boxes is None and w.areas is None and w.masks is None and w.rles is None
    assert inspect.signature(MDQE.online_video).parameters["geometry"].default is False
    assert inspect.signature(online.OnlineVideo.__init__).parameters["geometry"].default is False
