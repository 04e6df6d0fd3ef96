"""A deliberately naive YTVIS scorer for the tests: one (category, area range, detections cap, IoU threshold) at a time, plain Python
loops over plain lists, written separately from mdqe_cvpr2023_amd/vis_score.py (which works on whole [thresholds, detections] arrays).
What the two share is the evaluation's PARAMETERS (the threshold grids, the caps, the area ranges) and IEEE double arithmetic, so their
results are compared for equality.  The definition both restate: mdqe/data/pycocotools/ytvoseval.py (segm, default parameters).

A video is a dict of plain tables: "scores" [n], "labels" [n], "inter" [n][G], "pred_area" [n][L], "gt_area" [G][L] (the masks' pixel
counts), "gt_cats" [G], "crowd" [G], "gt_ann_area" [G][L] (the annotation's areas, what the size classes use)."""
import sys

import numpy as np

IOU_THRS = np.linspace(.5, 0.95, 10, endpoint=True).tolist()
REC_THRS = np.linspace(.0, 1.00, 101, endpoint=True).tolist()
CAPS = [1, 10, 100]
RANGES = [(0.0, 1e10), (0.0, 128.0 ** 2), (128.0 ** 2, 256.0 ** 2), (256.0 ** 2, 1e10)]
EPS = sys.float_info.epsilon                     # the spacing of doubles at 1


def mean_nonzero(row):
    vals = [int(a) for a in row if a]
    return sum(vals) / len(vals) if vals else 0


def video_iou(v, i, g):
    inter = int(v["inter"][i][g])
    union = sum(int(a) for a in v["pred_area"][i]) + sum(int(a) for a in v["gt_area"][g]) - inter
    return inter / union if union > 0 else 0.0


def match_one(v, cat, rng, cap, thr):
    """One video at one threshold -> (per kept detection (score, matched, ignored), ground-truth tracks that count) or None."""
    gts = [g for g in range(len(v["gt_cats"])) if v["gt_cats"][g] == cat]
    dts = [i for i in range(len(v["scores"])) if v["labels"][i] == cat]
    if not gts and not dts:
        return None
    lo, hi = rng
    ign = {g: bool(v["crowd"][g]) or not (lo <= mean_nonzero(v["gt_ann_area"][g]) <= hi) for g in gts}
    gts = [g for g in gts if not ign[g]] + [g for g in gts if ign[g]]
    dts = sorted(dts, key=lambda i: -v["scores"][i])[:min(cap, 100)]          # (sorted is stable)
    taken = set()
    out = []
    for i in dts:
        best, best_iou = None, min(thr, 1 - 1e-10)
        for g in gts:
            if g in taken and not v["crowd"][g]:
                continue
            if best is not None and not ign[best] and ign[g]:
                break
            iou = video_iou(v, i, g)
            if iou < best_iou:
                continue
            best, best_iou = g, iou
        if best is None:
            out.append((v["scores"][i], False, not (lo <= mean_nonzero(v["pred_area"][i]) <= hi)))
        else:
            taken.add(best)
            out.append((v["scores"][i], True, ign[best]))
    return out, sum(1 for g in gts if not ign[g])


def evaluate(videos, cats):
    """videos: {video_id: tables}; cats: the category axis -> (stats [12], precision [10, 101, K, 4, 3], recall [10, K, 4, 3])."""
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(cats), len(RANGES), len(CAPS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k, cat in enumerate(cats):
        for a, rng in enumerate(RANGES):
            for m, cap in enumerate(CAPS):
                for t, thr in enumerate(IOU_THRS):
                    per_video = [match_one(videos[vid], cat, rng, cap, thr) for vid in sorted(videos)]
                    per_video = [p for p in per_video if p is not None]
                    if not per_video:
                        continue
                    n_gt = sum(p[1] for p in per_video)
                    if n_gt == 0:
                        continue
                    dets = sorted([d for p in per_video for d in p[0]], key=lambda d: -d[0])
                    tp = fp = 0
                    rc, pr = [], []
                    for _, matched, ignored in dets:
                        if not ignored:
                            tp, fp = tp + (1 if matched else 0), fp + (0 if matched else 1)
                        rc.append(float(tp) / n_gt)
                        pr.append(float(tp) / (float(fp) + float(tp) + EPS))
                    recall[t, k, a, m] = rc[-1] if rc else 0
                    for i in range(len(pr) - 2, -1, -1):
                        pr[i] = max(pr[i], pr[i + 1])
                    for r, want in enumerate(REC_THRS):
                        at = next((i for i in range(len(rc)) if rc[i] >= want), None)
                        precision[t, r, k, a, m] = pr[at] if at is not None else 0.0

    def mean_of(x):
        x = x[x > -1]
        return -1 if x.size == 0 else np.mean(x)

    ap = lambda t, a, m: mean_of(precision[:, :, :, a:a + 1, m] if t is None else precision[t:t + 1, :, :, a:a + 1, m])   # noqa: E731
    ar = lambda a, m: mean_of(recall[:, :, a:a + 1, m])                                                                  # noqa: E731
    stats = np.array([ap(None, 0, 2), ap(0, 0, 2), ap(5, 0, 2), ap(None, 1, 2), ap(None, 2, 2), ap(None, 3, 2),
                      ar(0, 0), ar(0, 1), ar(0, 2), ar(1, 2), ar(2, 2), ar(3, 2)], dtype=np.float64)
    return stats, precision, recall
