"""Scoring a video's tracks against ground truth: video IoU and the YTVIS AP / AR table.

The reference ends `train_net.py --eval-only` with `YTVOSeval` (mdqe/data/ytvis_eval.py:159-200 -> mdqe/data/pycocotools/ytvoseval.py).
Its one expensive step is the video IoU of every (predicted track, ground-truth track) pair (`computeIoU`, ytvoseval.py:173-219): the
reference produces every full-resolution mask, copies it to the host, RLE-encodes it and merges the RLEs pairwise.  Here the final-mask
sweep counts the overlaps itself (ops.final_masks_overlap, csrc/score_ops.hip): a few hundred integers per video come back, no mask does.

    gt = GroundTruth(masks=m, category_ids=[3, 7])             # [G, L, H, W]; or rles=..., size=(H, W): the YTVIS json form
    res = model([{"image": frames, "height": H, "width": W, "ground_truth": gt}])
    res["pred_gt"]                                             # "inter" [n_out, G], "pred_area" [n_out, L], "gt_area" [G, L], "iou" [n_out, G]
    sc = YTVISScorer(); sc.add(video_id, res, gt); sc.evaluate()["stats"]      # AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl

`GroundTruth.from_result(res_exact)` makes a pseudo ground truth of another run of this model: what a fast mode costs in video IoU / AP.

`YTVISScorer` restates ytvoseval.py's segm path with default parameters in this project's own words; each step cites file:line.  The
reference's evaluator cannot be EXECUTED in this project's setting (its native RLE core, pycocotools' _mask, is neither in the reference
tree nor installed), so this half is held to the reference by reading and to an independent brute-force implementation by test
(tests/_score_ref.py) -- parity with a run of the reference's evaluator is unpinned, like rle.py's string packing.
"""
import numpy as np

from . import rle as R


def _table(x, rows):
    """x as int64 [rows, -1] (no rows: [0, columns of x])."""
    a = np.asarray(x, dtype=np.int64)
    return a.reshape(rows, -1) if rows else np.zeros((0, a.shape[1] if a.ndim == 2 else 0), dtype=np.int64)


def iou_table(inter, pred_area, gt_area):
    """ytvoseval.py:200-214 (iou_seq) from integers.  Its four per-frame cases are one formula once a missing segmentation counts as an
    empty mask: i = sum_f |d & g|, u = sum_f |d | g| = sum_f |d| + sum_f |g| - i; iou = i / u, and 0 where u is 0 (:213).
    inter [n, G], pred_area [n, L], gt_area [G, L] (integers) -> float64 [n, G]."""
    inter = np.asarray(inter, dtype=np.int64)
    pa = _table(pred_area, inter.shape[0]).sum(1)
    ga = _table(gt_area, inter.shape[1]).sum(1)
    union = pa[:, None] + ga[None] - inter
    out = np.zeros(inter.shape, dtype=np.float64)
    np.divide(inter.astype(np.float64), union.astype(np.float64), out=out, where=union > 0)
    return out


def avg_area(areas):
    """The size a track is classed by (ytvoseval.py:97-101): its pixel count averaged over the frames where it has any; 0 for a track
    that never appears.  areas: integers per frame (None counts as zero)."""
    a = np.array([int(x) if x else 0 for x in areas], dtype=np.int64)
    seen = a[a != 0]
    return float(seen.sum()) / seen.size if seen.size else 0.0


class GroundTruth:
    """One video's annotation: G tracks over L frames of (H, W).
    masks: [G, L, H, W] bool / uint8 (tensor on the host or the device, or array); or rles: G lists of L COCO RLE dicts ({"size",
    "counts"}, counts a string or a list of run lengths), None for a frame without the object -- the YTVIS json form -- with size =
    (H, W) (needed when G == 0 or a track has no frame at all).  category_ids [G]; iscrowd [G] (default 0); ids [G] (default 1..G);
    areas [G, L] per-frame areas as the json carries them (None = 0), what ytvoseval.py:97-101 averages -- by default counted from the
    masks.  Kept packed: `words`, ceil(G / 32) uint32 [L, H, W] tensors, bit g % 32 of word g // 32 = track g holds the pixel (built
    with torch ops where the masks live), and `gt_area` int64 [G, L], the masks' own pixel counts (what the IoU needs)."""

    def __init__(self, masks=None, rles=None, size=None, category_ids=(), iscrowd=None, ids=None, areas=None):
        import torch
        if (masks is None) == (rles is None):
            raise ValueError("GroundTruth: give masks or rles (one of them)")
        if masks is not None:
            m = torch.as_tensor(masks)
            if m.dim() != 4:
                raise ValueError("GroundTruth: masks must be [G, L, H, W], got %s" % (tuple(m.shape),))
            G, L, H, W = (int(v) for v in m.shape)
            if size is not None and (int(size[0]), int(size[1])) != (H, W):
                raise ValueError("GroundTruth: size %s differs from the masks' %s" % (tuple(size), (H, W)))
            m = m != 0
            self.gt_area = m.flatten(2).sum(2).to(torch.int64).cpu() if G else torch.zeros((0, L), dtype=torch.int64)
            self.words = []
            for g0 in range(0, G, 32):
                word = torch.zeros((L, H, W), dtype=torch.int32, device=m.device)
                for b in range(min(32, G - g0)):
                    word |= m[g0 + b].to(torch.int32) * (1 << b if b < 31 else -2 ** 31)
                self.words.append(word.view(torch.uint32))
        else:
            G = len(rles)
            lens = {len(r) for r in rles}
            if len(lens) > 1:
                raise ValueError("GroundTruth: every track needs one entry (RLE dict or None) per frame, got lengths %s" % sorted(lens))
            first = next((s for r in rles for s in r if s), None)
            if size is None and first is None:
                raise ValueError("GroundTruth: size = (H, W) is needed when no track has a segmentation")
            H, W = (int(v) for v in (size if size is not None else first["size"]))
            L = lens.pop() if lens else 0
            area = np.zeros((G, L), dtype=np.int64)
            words = np.zeros((-(-G // 32), L, H, W), dtype=np.uint32)
            for g, track in enumerate(rles):
                for f, s in enumerate(track):
                    if not s:
                        continue
                    if (int(s["size"][0]), int(s["size"][1])) != (H, W):
                        raise ValueError("GroundTruth: track %d frame %d has size %s, the video %s" % (g, f, list(s["size"]), [H, W]))
                    d = R.decode_dense(s)
                    area[g, f] = int(d.sum())
                    words[g // 32, f] |= d.astype(np.uint32) << np.uint32(g % 32)
            self.gt_area = torch.from_numpy(area)
            self.words = [torch.from_numpy(w) for w in words]
        self.G, self.length, self.size = G, L, (H, W)
        self._on = {}                                  # `on`: device -> the words there
        self.category_ids = [int(c) for c in category_ids]
        self.iscrowd = [0] * G if iscrowd is None else [int(c) for c in iscrowd]
        self.ids = list(range(1, G + 1)) if ids is None else list(ids)
        if areas is None:
            self.areas = self.gt_area.numpy().copy()
        else:
            self.areas = np.array([[int(a) if a else 0 for a in row] for row in areas], dtype=np.int64).reshape(G, L)
        for name, v in (("category_ids", self.category_ids), ("iscrowd", self.iscrowd), ("ids", self.ids)):
            if len(v) != G:
                raise ValueError("GroundTruth: %s needs one entry per track (%d), got %d" % (name, G, len(v)))

    def on(self, device):
        """The packed form on `device`: a list of ceil(G / 32) uint32 [L, H, W] tensors (the tensors themselves where they live there).
        The copy is made once per device and kept with the object, so a ground truth used for several runs is uploaded once; it holds
        4 * L * H * W bytes per 32 tracks there for as long as the object lives."""
        import torch
        key = str(torch.device(device))
        if key not in self._on:
            self._on[key] = [w.view(torch.int32).to(device).contiguous().view(torch.uint32) for w in self.words]
        return self._on[key]

    @classmethod
    def from_result(cls, res, score_thr=0.0):
        """A result of this model (`pred_masks` or `pred_rles`, `pred_labels`, `pred_scores`) as a pseudo ground truth: the outputs with
        score >= score_thr, in order, category = predicted label -- "a fast mode against the exact mode"."""
        import torch
        keep = [j for j, s in enumerate(res["pred_scores"]) if s >= score_thr]
        cats = [int(res["pred_labels"][j]) for j in keep]
        size = tuple(int(v) for v in res["image_size"])
        if res.get("pred_rles") is not None:
            return cls(rles=[list(res["pred_rles"][j]) for j in keep], size=size, category_ids=cats)
        pm = res["pred_masks"]
        if len(keep) == 0:
            L = int(pm[0].shape[0]) if len(pm) else 0
            return cls(masks=torch.zeros((0, L) + size, dtype=torch.bool), category_ids=cats)
        return cls(masks=torch.stack([torch.as_tensor(pm[j]) for j in keep]), category_ids=cats)


# ---- the evaluation's parameters (the defaults of the reference's segm evaluation, ytvoseval.py:531-540) ------------------------------
IOU_THRS = np.linspace(0.5, 0.95, 10)             # ten overlap thresholds, 0.50, 0.55 .. 0.95
REC_THRS = np.linspace(0.0, 1.0, 101)             # the 101 recall levels a precision curve is sampled at
CAPS = (1, 10, 100)                               # predictions kept per video and category, best scores first
SIZE_EDGES = (0.0, 128.0 ** 2, 256.0 ** 2, 1e10)  # small | medium | large, in pixels of average area (1e10 stands for "no limit")
SIZE_CLASSES = [("all", SIZE_EDGES[0], SIZE_EDGES[-1])] + [(n, SIZE_EDGES[i], SIZE_EDGES[i + 1]) for i, n in enumerate(("small", "medium", "large"))]
# the summary (ytvoseval.py:487-501): name, precision or recall, threshold index (None: all ten), size class, cap
SUMMARY = [("AP", "precision", None, 0, 2), ("AP50", "precision", 0, 0, 2), ("AP75", "precision", 5, 0, 2),
           ("APs", "precision", None, 1, 2), ("APm", "precision", None, 2, 2), ("APl", "precision", None, 3, 2),
           ("AR1", "recall", None, 0, 0), ("AR10", "recall", None, 0, 1), ("AR100", "recall", None, 0, 2),
           ("ARs", "recall", None, 1, 2), ("ARm", "recall", None, 2, 2), ("ARl", "recall", None, 3, 2)]
STAT_NAMES = [row[0] for row in SUMMARY]


def _last_best(ok, iou):
    """Per threshold (rows of ok [T, n]) the admissible column with the largest iou [n], the LAST of them on a tie, and whether one
    exists.  (The reference walks the columns in order and lets an equal overlap replace the earlier one, ytvoseval.py:315-319.)"""
    n = ok.shape[1]
    if n == 0:
        return np.zeros(ok.shape[0], dtype=np.int64), np.zeros(ok.shape[0], dtype=bool)
    key = np.where(ok, iou[None], -1.0)[:, ::-1]
    return n - 1 - key.argmax(1), ok.any(1)


class YTVISScorer:
    """The YTVIS AP / AR table (the reference's segm evaluation with default parameters, ytvoseval.py) over the integers `pred_gt`
    carries; no mask is touched.  add(video_id, result, gt) per video, evaluate() -> {"stats": float64 [12] (STAT_NAMES order), one
    key per name, "precision" [10 thresholds, 101 recall levels, K categories, 4 size classes, 3 caps], "recall" [10, K, 4, 3],
    "category_ids"}; -1 marks a category / size class without a ground truth that counts (:363-364, :481-482).
    category_ids: the K axis (the reference takes the dataset's, :82); default: every category a ground truth or a prediction names
    (a category without ground truth stays -1 either way, :402-403).
    All ten thresholds are matched at once: the state of a video is a [thresholds, ground-truth tracks] table of what is still free."""

    def __init__(self, category_ids=None):
        self.category_ids = None if category_ids is None else sorted(set(int(c) for c in category_ids))
        self.videos = {}

    def add(self, video_id, result, gt):
        """result: a video's result with "pred_gt", "pred_scores", "pred_labels"; gt: the GroundTruth it was scored against."""
        pg = result.get("pred_gt")
        if pg is None:
            raise ValueError("YTVISScorer.add: the result has no 'pred_gt' (hand the ground truth in with the video: 'ground_truth')")
        self.add_tables(video_id, result["pred_scores"], result["pred_labels"], pg["inter"], pg["pred_area"], pg["gt_area"],
                        gt.category_ids, gt.iscrowd, gt.areas)

    def add_tables(self, video_id, scores, labels, inter, pred_area, gt_area, gt_category_ids, iscrowd=None, gt_areas=None):
        """The same from plain tables: scores / labels [n], inter [n, G], pred_area [n, L], gt_area [G, L] (the masks' pixel counts),
        gt_category_ids / iscrowd [G], gt_areas [G, L] (the annotation's per-frame areas, default gt_area)."""
        if video_id in self.videos:
            raise ValueError("YTVISScorer: video %r was added already" % (video_id,))
        n, G = len(scores), len(gt_category_ids)
        inter = np.asarray(inter, dtype=np.int64).reshape(n, G)
        pa, ga = _table(pred_area, n), _table(gt_area, G)
        ann = ga if gt_areas is None else _table(gt_areas, G)
        self.videos[video_id] = {
            "score": np.array([float(x) for x in scores], dtype=np.float64), "label": np.array([int(x) for x in labels], dtype=np.int64),
            "pred_size": np.array([avg_area(r) for r in pa], dtype=np.float64),          # (a prediction's areas are its masks', ytvos.py:229-247)
            "gt_cat": np.array([int(c) for c in gt_category_ids], dtype=np.int64),
            "crowd": np.zeros(G, dtype=bool) if iscrowd is None else np.array([bool(c) for c in iscrowd], dtype=bool),
            "gt_size": np.array([avg_area(r) for r in ann], dtype=np.float64),
            "iou": iou_table(inter, pa, ga)}

    @staticmethod
    def _match(v, cat, lo, hi):
        """One video, one category, one size class [lo, hi] -> None when the video has neither a ground truth nor a prediction of the
        category (:276-277), else (scores [D] best first, matched bool [T, D], ignored bool [T, D], ground truths that count).
        Predictions go best score first, equal scores in the order given, at most CAPS[-1] of them (:183-186).  A ground truth does not
        count ("ignored") when it is a crowd or its size lies outside the class (:117, :279-283); those are looked at after the ones
        that count (:286).  A prediction takes, per threshold, the free ground truth it overlaps most among those that count, at least
        by the threshold (capped just below 1, :305); only when none qualifies, an ignored one by the same rule (:311-313).  A crowd
        stays free however often it is taken (:309).  What matches an ignored ground truth is ignored with it (:323); so is what
        matches nothing and is itself outside the size class (:327-328)."""
        gi, di = np.flatnonzero(v["gt_cat"] == cat), np.flatnonzero(v["label"] == cat)
        if gi.size == 0 and di.size == 0:
            return None
        out_of_class = lambda size: (size < lo) | (size > hi)                                # noqa: E731
        skip = v["crowd"][gi] | out_of_class(v["gt_size"][gi])
        gi = np.concatenate([gi[~skip], gi[skip]])
        n_count = int((~skip).sum())
        crowd = v["crowd"][gi]
        di = di[np.argsort(-v["score"][di], kind="stable")][:CAPS[-1]]
        T, D = IOU_THRS.shape[0], di.size
        bar = np.minimum(IOU_THRS, 1 - 1e-10)[:, None]
        free = np.ones((T, gi.size), dtype=bool)
        matched, ignored = np.zeros((T, D), dtype=bool), np.zeros((T, D), dtype=bool)
        rows = np.arange(T)
        for d, i in enumerate(di):
            iou = v["iou"][i, gi]
            ok = (free | crowd[None]) & (iou[None] >= bar)
            a, has_a = _last_best(ok[:, :n_count], iou[:n_count])
            b, has_b = _last_best(ok[:, n_count:], iou[n_count:])
            pick = np.where(has_a, a, b + n_count)
            hit = has_a | has_b
            matched[:, d] = hit
            ignored[:, d] = hit & ~has_a
            free[rows[hit], pick[hit]] = False
        ignored |= ~matched & out_of_class(v["pred_size"][di])[None]
        return v["score"][di], matched, ignored, n_count

    def evaluate(self):
        cats = self.category_ids
        if cats is None:
            cats = sorted({int(c) for v in self.videos.values() for c in np.concatenate([v["gt_cat"], v["label"]])})
        vids = sorted(self.videos)                                                           # (:142)
        T, R = IOU_THRS.shape[0], REC_THRS.shape[0]
        precision = np.full((T, R, len(cats), len(SIZE_CLASSES), len(CAPS)), -1.0)           # -1: nothing to measure (:363-364)
        recall = np.full((T, len(cats), len(SIZE_CLASSES), len(CAPS)), -1.0)
        eps = np.finfo(np.float64).eps
        for k, cat in enumerate(cats):
            for a, (_, lo, hi) in enumerate(SIZE_CLASSES):
                per_video = [r for r in (self._match(self.videos[vid], cat, lo, hi) for vid in vids) if r is not None]
                n_count = sum(r[3] for r in per_video)
                if n_count == 0:                                                             # (:389-390, :402-403)
                    continue
                for m, cap in enumerate(CAPS):
                    # the videos' best `cap` predictions as one ranking, best first, ties in video order (:391-399)
                    order = np.argsort(-np.concatenate([r[0][:cap] for r in per_video]), kind="stable")
                    hit = np.concatenate([r[1][:, :cap] for r in per_video], 1)[:, order]
                    live = ~np.concatenate([r[2][:, :cap] for r in per_video], 1)[:, order]
                    tp = np.cumsum(hit & live, 1).astype(np.float64)                         # [T, D] down the ranking
                    fp = np.cumsum(~hit & live, 1).astype(np.float64)
                    D = tp.shape[1]
                    if D == 0:                                                               # ground truth but no prediction: all zero
                        recall[:, k, a, m], precision[:, :, k, a, m] = 0.0, 0.0
                        continue
                    rc = tp / n_count
                    pr = tp / (fp + tp + eps)                                                # (:413-414)
                    # a curve's precision at recall r is the best precision at any recall >= r (:427-429)
                    env = np.maximum.accumulate(pr[:, ::-1], 1)[:, ::-1]
                    # rc does not decrease: the first rank that reaches a level = the number of ranks below it; a level never reached reads 0 (:431-437)
                    at = (rc[:, None, :] < REC_THRS[None, :, None]).sum(2)
                    precision[:, :, k, a, m] = np.where(at < D, np.take_along_axis(env, np.minimum(at, D - 1), 1), 0.0)
                    recall[:, k, a, m] = rc[:, -1]
        stats = np.zeros(len(SUMMARY))
        for j, (_, kind, t, a, m) in enumerate(SUMMARY):                                     # (:456-501)
            table = (precision if kind == "precision" else recall)[slice(None) if t is None else slice(t, t + 1), ..., a, m]
            measured = table[table > -1]
            stats[j] = np.mean(measured) if measured.size else -1
        out = {"stats": stats, "precision": precision, "recall": recall, "category_ids": list(cats)}
        out.update({n: float(s) for n, s in zip(STAT_NAMES, stats)})
        return out
