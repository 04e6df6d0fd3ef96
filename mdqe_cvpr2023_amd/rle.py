"""COCO mask RLE for the result writer.

The reference turns every [L,H,W] boolean video mask into per-frame COCO RLEs on the host
(instances_to_coco_json_video, mdqe/data/ytvis_eval.py:288-324: pycocotools `encode` of a Fortran-ordered uint8 copy per
frame).  Here the run boundaries come straight from the device (ops.final_masks_rle: the dense mask is never written nor
copied) and only the LEB128-like string packing (cocoapi rleToString) runs on the host, vectorised over all runs of a
video.  `instances_to_coco_json_video` is the drop-in for the reference function: it takes the model output with
`pred_rles` (model.rle_output = True) or, as a fallback, dense `pred_masks`.

Geometry: the kernels that decide the final masks also count their pixels and keep their tight boxes (ops.final_masks_geom /
ops.final_masks_rle_geom -> int32 rows (area, xmin, ymin, xmax, ymax), inclusive, empty = (0, W, H, -1, -1)).  `geom_to_boxes` turns
those rows into the d2 / COCO forms; `area` / `to_bbox` (pycocotools `area` / `toBbox`, mdqe/data/pycocotools/mask.py:93-101) and
`geometry_dense` compute the same on the host from RLE dicts / dense masks -- for the paths without a device window and as the
independent check in the tests.  `instances_to_ytvis_annotations` writes predictions in the YTVIS ANNOTATION layout the reference's
loader reads (mdqe/data/datasets/ytvis.py:260-306).
"""
import numpy as np


def counts_to_strings(counts, lengths):
    """counts: int64 [sum(lengths)] run lengths of consecutive masks; lengths: runs per mask -> list of bytes (rleToString).
    Every run i > 2 of a mask is stored as the difference to run i-2; values are cut into 5-bit groups, bit 5 flags a
    continuation, a group sequence ends when the rest is all sign bits; each byte is offset by 48."""
    counts = np.asarray(counts, dtype=np.int64)
    lengths = np.asarray(lengths, dtype=np.int64)
    n = int(counts.shape[0])
    if n == 0:
        return [b"" for _ in lengths]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    idx_in_mask = np.arange(n, dtype=np.int64) - np.repeat(starts, lengths)
    x = counts.copy()
    d = np.zeros_like(counts)
    d[2:] = counts[:-2]
    x = np.where(idx_in_mask > 2, counts - d, counts)
    chars = np.zeros((n, 8), dtype=np.uint8)
    valid = np.zeros((n, 8), dtype=bool)
    alive = np.ones(n, dtype=bool)
    for r in range(8):                                   # 8 groups cover 40 bits
        c = x & 0x1f
        x = x >> 5                                        # arithmetic shift
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        ch = (c | (more.astype(np.int64) << 5)) + 48
        chars[:, r] = np.where(alive, ch, 0)
        valid[:, r] = alive
        alive = alive & more
        if not alive.any():
            break
    per_run = valid.sum(1)
    flat = chars[valid]                                   # row-major: groups of a run stay together, runs stay in order
    run_off = np.concatenate([[0], np.cumsum(per_run)])
    out = []
    buf = flat.tobytes()
    for s, l in zip(starts, lengths):
        out.append(buf[run_off[s]:run_off[s + l]])
    return out


def strings_to_counts(strings):
    """Inverse of counts_to_strings (cocoapi rleFrString), over all masks at once: list of bytes / str -> (counts int64
    [sum(lengths)], lengths int64 [n_masks])."""
    strings = [x.encode("ascii") if isinstance(x, str) else bytes(x) for x in strings]
    n_masks = len(strings)
    if n_masks == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    c = np.frombuffer(b"".join(strings), dtype=np.uint8).astype(np.int64) - 48
    nb = int(c.shape[0])
    if nb == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(n_masks, dtype=np.int64)
    last = (c & 0x20) == 0                                # the last 5-bit group of a run
    gstart = np.flatnonzero(np.concatenate([[True], last[:-1]]))          # first byte of every run
    run_of = np.cumsum(np.concatenate([[0], last[:-1].astype(np.int64)]))   # run index of every byte
    k = np.arange(nb, dtype=np.int64) - gstart[run_of]    # group index within its run
    x = np.zeros(int(gstart.shape[0]), dtype=np.int64)
    np.add.at(x, run_of, (c & 0x1f) << (5 * k))
    neg = last & ((c & 0x10) != 0)                        # sign bit of the top group: extend
    x[run_of[neg]] |= (np.int64(-1) << (5 * (k[neg] + 1)))
    byte_len = np.array([len(b) for b in strings], dtype=np.int64)
    byte_end = np.cumsum(byte_len)
    ends = np.concatenate([[0], np.cumsum(last.astype(np.int64))])        # runs completed before byte i
    lengths = ends[byte_end] - ends[byte_end - byte_len]
    # run i > 2 was stored as the difference to run i-2: undo with one cumulative sum per parity and mask
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    idx = np.arange(int(x.shape[0]), dtype=np.int64) - np.repeat(starts, lengths)
    counts = x.copy()
    for par in (0, 1):
        sel = np.flatnonzero((idx >= 1) & (idx % 2 == par))              # chains 1,3,5,.. and 2,4,6,.. (run 0 stands alone)
        if sel.size == 0:
            continue
        cs = np.cumsum(x[sel])
        mask_of = np.searchsorted(starts, sel, side="right") - 1
        first = np.concatenate([[True], mask_of[1:] != mask_of[:-1]])     # first element of this chain in its mask
        head = np.maximum.accumulate(np.where(first, np.arange(sel.size), 0))
        counts[sel] = cs - (cs - x[sel])[head]            # minus the sum of the chains of the masks before
    return counts, lengths


def _as_list(rle):
    return ([rle], True) if isinstance(rle, dict) else (list(rle), False)


def _runs(rles):
    """RLE dicts -> per ones-run (mask index, start, end) in column-major pixel indices, heights, widths."""
    counts, lengths = strings_to_counts([r["counts"] for r in rles])
    hs = np.array([int(r["size"][0]) for r in rles], dtype=np.int64)
    ws = np.array([int(r["size"][1]) for r in rles], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    mask_of = np.repeat(np.arange(len(rles), dtype=np.int64), lengths)
    idx = np.arange(int(counts.shape[0]), dtype=np.int64) - np.repeat(starts, lengths)
    end = np.cumsum(counts)
    end = end - np.repeat((end - counts)[starts[lengths > 0]], lengths[lengths > 0])   # per mask: position after each run
    ones = (idx % 2 == 1) & (counts > 0)
    return mask_of[ones], (end - counts)[ones], end[ones], hs, ws


def area(rle):
    """pycocotools `area`: number of set pixels of an RLE dict (int) or of each of a list of them (int64 array)."""
    rles, single = _as_list(rle)
    m, s, e, hs, ws = _runs(rles)
    out = np.zeros(len(rles), dtype=np.int64)
    np.add.at(out, m, e - s)
    return int(out[0]) if single else out


def to_bbox(rle):
    """pycocotools `toBbox`: [x, y, w, h] (float64) of the set pixels of an RLE dict ([4]) or of each of a list ([n, 4]); zeros
    for an empty mask."""
    rles, single = _as_list(rle)
    m, s, e, hs, ws = _runs(rles)
    n = len(rles)
    h = hs[m]
    xa, xb = s // h, (e - 1) // h                          # first / last column a run touches
    wrap = xa != xb                                        # a run that crosses a column boundary touches rows 0 and h-1
    ya = np.where(wrap, 0, s % h)
    yb = np.where(wrap, h - 1, (e - 1) % h)
    big = np.iinfo(np.int64).max
    x0 = np.full(n, big); y0 = np.full(n, big); x1 = np.full(n, -1, dtype=np.int64); y1 = np.full(n, -1, dtype=np.int64)
    np.minimum.at(x0, m, xa); np.minimum.at(y0, m, ya)
    np.maximum.at(x1, m, xb); np.maximum.at(y1, m, yb)
    has = x1 >= 0
    out = np.zeros((n, 4), dtype=np.float64)
    out[has] = np.stack([x0, y0, x1 - x0 + 1, y1 - y0 + 1], 1)[has]
    return out[0] if single else out


def geometry_dense(masks):
    """bool / 0-1 tensor (or array) [..., H, W] -> int32 tensor [..., 5]: (area, xmin, ymin, xmax, ymax) of the set pixels, inclusive;
    (0, W, H, -1, -1) for an empty mask -- the rows ops.final_masks_geom writes."""
    import torch
    m = torch.as_tensor(masks).to(torch.bool)
    H, W = int(m.shape[-2]), int(m.shape[-1])
    xa, ya = m.any(-2), m.any(-1)                          # [..., W], [..., H]
    ar_x, ar_y = torch.arange(W, device=m.device), torch.arange(H, device=m.device)
    neg = torch.tensor(-1, device=m.device)
    cnt = m.flatten(-2).sum(-1)
    x0 = torch.where(xa, ar_x, torch.tensor(W, device=m.device)).min(-1)[0]
    x1 = torch.where(xa, ar_x, neg).max(-1)[0]
    y0 = torch.where(ya, ar_y, torch.tensor(H, device=m.device)).min(-1)[0]
    y1 = torch.where(ya, ar_y, neg).max(-1)[0]
    return torch.stack([cnt, x0, y0, x1, y1], -1).to(torch.int32)


def geom_to_boxes(geom):
    """geom rows [..., 5] (tensor or array) -> (boxes float32 [..., 4] = [xmin, ymin, xmax + 1, ymax + 1], XYXY_ABS as d2's
    BitMasks.get_bounding_boxes, zeros for an empty mask; areas int64 [...]), on the host."""
    import torch
    g = torch.as_tensor(geom).cpu().to(torch.int64)
    has = g[..., 0] > 0
    b = torch.stack([g[..., 1], g[..., 2], g[..., 3] + 1, g[..., 4] + 1], -1)
    boxes = torch.where(has[..., None], b, torch.zeros_like(b)).to(torch.float32)
    return boxes, g[..., 0].clone()


def positions_to_counts(pos, n_pos, total):
    """pos [n_masks, cap] change positions (column-major pixel indices), n_pos [n_masks] -> (counts, lengths) of all masks."""
    pos = np.asarray(pos, dtype=np.int64)
    n_pos = np.asarray(n_pos, dtype=np.int64)
    n_masks, cap = pos.shape
    if (n_pos > cap).any():
        raise OverflowError("RLE position buffer too small")
    lengths = n_pos + 1
    col = np.arange(cap + 1, dtype=np.int64)[None]
    ext = np.concatenate([pos, np.zeros((n_masks, 1), dtype=np.int64)], 1)
    ext = np.where(col < n_pos[:, None], ext, total)              # the position after the last change is the mask's end
    prev = np.concatenate([np.zeros((n_masks, 1), dtype=np.int64), ext[:, :-1]], 1)
    runs = ext - prev
    keep = col <= n_pos[:, None]
    return runs[keep], lengths


def positions_to_rles(pos, n_pos, size, frames):
    """ops.final_masks_rle's pos [tracks * frames, cap], n_pos [tracks * frames] (on the host) of (H, W) masks -> per track, per frame
    {"size", "counts": str}."""
    H, W = int(size[0]), int(size[1])
    counts, lengths = positions_to_counts(pos, n_pos, H * W)
    strs = counts_to_strings(counts, lengths)
    return [[{"size": [H, W], "counts": s.decode("utf-8")} for s in strs[i:i + frames]] for i in range(0, len(strs), frames)]


def empty_rle(size):
    """The RLE dict of an all-zero (H, W) mask: one run of H * W zeros."""
    H, W = int(size[0]), int(size[1])
    return {"size": [H, W], "counts": counts_to_strings([H * W], [1])[0].decode("utf-8")}


def encode_dense(mask):
    """Host fallback: one [H,W] boolean mask (numpy / CPU tensor) -> {"size", "counts": str}, pycocotools-style."""
    m = np.asarray(mask).astype(np.uint8)
    v = m.flatten(order="F")
    change = np.flatnonzero(np.diff(np.concatenate([[0], v])) != 0)
    counts, lengths = positions_to_counts(change[None], [len(change)], v.shape[0])
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": counts_to_strings(counts, lengths)[0].decode("utf-8")}


def decode_dense(rle):
    """Inverse of `encode_dense` (pycocotools `decode`): {"size": [H, W], "counts": str / bytes or a list of run lengths (the
    uncompressed form)} -> uint8 [H, W]; runs alternate 0, 1, ... in column-major order."""
    H, W = int(rle["size"][0]), int(rle["size"][1])
    c = rle["counts"]
    counts = strings_to_counts([c])[0] if isinstance(c, (str, bytes)) else np.asarray(c, dtype=np.int64)
    if int(counts.sum()) != H * W or (counts < 0).any():
        raise ValueError("decode_dense: the runs cover %d pixels, the mask has %d" % (int(counts.sum()), H * W))
    v = np.repeat((np.arange(counts.shape[0]) % 2).astype(np.uint8), counts)
    return v.reshape((H, W), order="F")


# ---- label maps (model.label_output / online emit="labels"): uint8 [L, H, W], label t + 1 = track t, 0 = background ----------------------
def labels_to_masks(label_map, track_ids):
    """The exclusive region of each track of `track_ids` as a bool plane -> [len(track_ids), L, H, W] (tensor in, tensor out; else numpy)."""
    if hasattr(label_map, "dim"):
        import torch
        ids = torch.as_tensor(list(track_ids), dtype=torch.int64).view(-1, 1, 1, 1) + 1
        return label_map.unsqueeze(0) == ids.to(label_map.device)
    lm = np.asarray(label_map)
    return lm[None] == (np.asarray(list(track_ids), dtype=np.int64).reshape(-1, 1, 1, 1) + 1)


def labels_keep(label_map, track_ids):
    """The map with every label but those of `track_ids` set to 0 -- "only my selected tracks" (a map names every track of its window,
    also one that misses the video-level top-k).  One pass through a 256-entry look-up table; same type and shape as the input."""
    lut = np.zeros(256, dtype=np.uint8)
    for t in track_ids:
        if not 0 <= int(t) < 255:
            raise ValueError("labels_keep: track id %r is outside 0..254" % (t,))
        lut[int(t) + 1] = int(t) + 1
    if hasattr(label_map, "dim"):
        import torch
        return torch.from_numpy(lut).to(label_map.device)[label_map.long()]
    return lut[np.asarray(label_map)]


def labels_to_rles(label_map, track_id):
    """The exclusive region of one track as per-frame COCO RLE dicts (`encode_dense`) -> list of L {"size", "counts"}."""
    lm = label_map.cpu().numpy() if hasattr(label_map, "dim") else np.asarray(label_map)
    return [encode_dense(fm == int(track_id) + 1) for fm in lm]


def instances_to_coco_json_video(inputs, outputs):
    """Drop-in for mdqe/data/ytvis_eval.py:288-324: list of {"video_id", "score", "category_id", "segmentations"}."""
    assert len(inputs) == 1, "More than one inputs are loaded for inference!"
    video_id = inputs[0]["video_id"]
    res = []
    rles = outputs.get("pred_rles")
    for i, (s, l) in enumerate(zip(outputs["pred_scores"], outputs["pred_labels"])):
        segms = rles[i] if rles is not None else [encode_dense(m) for m in outputs["pred_masks"][i]]
        res.append({"video_id": video_id, "score": s, "category_id": l, "segmentations": segms})
    return res


def instances_to_ytvis_annotations(inputs, outputs, score_thr=0.0, first_id=1):
    """Predictions as YTVIS-format ANNOTATIONS (pseudo-labels): one record per output track with score >= score_thr, in the layout
    the reference's loader reads (mdqe/data/datasets/ytvis.py:260-306): id (first_id, first_id + 1, ...), video_id, category_id,
    iscrowd, score, height, width, length and per frame segmentations[f] (RLE dict), bboxes[f] ([x, y, w, h]), areas[f] (int) --
    all three None on a frame whose mask is empty, which is what makes the loader skip the instance on that frame (:283).
    Takes `pred_rles` or dense `pred_masks`; `pred_boxes` / `pred_areas` (model.geometry_output) are used when present, the host
    helpers above when not."""
    assert len(inputs) == 1, "More than one inputs are loaded for inference!"
    video_id = inputs[0]["video_id"]
    Ho, Wo = int(outputs["image_size"][0]), int(outputs["image_size"][1])
    rles, boxes, areas = outputs.get("pred_rles"), outputs.get("pred_boxes"), outputs.get("pred_areas")
    res = []
    for i, (s, l) in enumerate(zip(outputs["pred_scores"], outputs["pred_labels"])):
        if s < score_thr:
            continue
        segms = list(rles[i]) if rles is not None else [encode_dense(m) for m in outputs["pred_masks"][i]]
        if boxes is not None and areas is not None:
            b = np.asarray(boxes[i], dtype=np.float64)
            xywh = np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1) if len(segms) else np.zeros((0, 4))
            ar = np.asarray(areas[i], dtype=np.int64)
        else:
            xywh, ar = (to_bbox(segms), area(segms)) if len(segms) else (np.zeros((0, 4)), np.zeros(0, dtype=np.int64))
        has = ar > 0
        res.append({"id": first_id + len(res), "video_id": video_id, "category_id": int(l), "iscrowd": 0, "score": float(s),
                    "height": Ho, "width": Wo, "length": len(segms),
                    "segmentations": [sg if h else None for sg, h in zip(segms, has)],
                    "bboxes": [[float(v) for v in bb] if h else None for bb, h in zip(xywh, has)],
                    "areas": [int(a) if h else None for a, h in zip(ar, has)]})
    return res
