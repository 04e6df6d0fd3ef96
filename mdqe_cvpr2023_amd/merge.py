"""The second half of the clip loop (mdqe/mdqe.py:337-366, 430-471): `ClipMerger` (tracker update per clip, window flushes) and
`video_result` (the video's result from the flushed windows); `meta_arch.MDQE` keeps its entry points as delegates.  A flushed window
becomes final masks per window into pinned memory (`_early_masks`), per window as a record (`_online_window`, online.OnlineVideo) or all
windows in one pass at the end (`video_result`).  What the three share is written once: `dense_masks` / `rle_positions` (window logits
-> masks / run boundaries, with or without geometry), `to_host` (the hop on the copy stream), `rle.positions_to_rles`, `stitch`.
`label_maps` is the third output form (model.label_output, online "labels"): one uint8 plane per frame that names the track owning each
pixel, from the same three places; its frames are disjoint between windows, so it needs no `stitch`.  `overlay_frames` is the fourth
(model.overlay_output, online "overlay"): that map painted over the frames the caller handed in (`FrameStore`), uint8 [F, Ho, Wo, 3].
`OverlapTables` is not an output form but a score: with a ground truth handed in (vis_score.GroundTruth), every flushed window's final
masks are counted against it where they are decided (ops.final_masks_overlap) -- "pred_gt", beside whatever form the masks take."""
import contextlib
import dataclasses
import os

import torch

from . import rle as R
from .tracking import Clips, OverTracker


def dense_masks(m, idx, stride, frame_hw, out_size, geometry, out, f_off):
    """Final masks of rows `idx` (int32, device) of window logits m [n, F, Hm, Wm] into out[:len(idx), f_off:f_off + F] (uint8, device).
    -> the window's geometry table int32 [len(idx), F, 5] on the device (geometry), else None."""
    from . import ops
    (fh, fw), (Ho, Wo) = frame_hw, out_size
    if geometry:
        return ops.final_masks_geom(m, idx, stride, fh, fw, Ho, Wo, out, f_off)[1].view(int(idx.numel()), int(m.shape[1]), 5)
    ops.final_masks(m, idx, stride, fh, fw, Ho, Wo, out, f_off)


def label_maps(m, stride, frame_hw, out_size, geometry, out, f_off):
    """The label map of window logits m [n, F, Hm, Wm] into out[f_off:f_off + F] (uint8 [>= f_off + F, Ho, Wo], device): per pixel the
    track (row + 1) with the largest up-sampled logit among ALL n rows whose final mask holds the pixel, 0 = background (n = 0: zeros).
    Every path lets all rows of the window compete, so the paths agree bit for bit, and a track that later misses the video-level top-k
    still owns its pixels (rle.labels_keep drops such labels).  -> the geometry table of the labels' visible regions, int32 [n, F, 5] on
    the device (geometry), else None."""
    from . import ops
    (fh, fw), (Ho, Wo) = frame_hw, out_size
    n = int(m.shape[0])
    idx = torch.arange(n, dtype=torch.int32, device=m.device)
    geom = ops.final_label_map(m, idx, stride, fh, fw, Ho, Wo, out, f_off, geom=True if geometry else None)[1]
    return geom.view(n, int(m.shape[1]), 5) if geometry else None


class OverlapTables:
    """A video's overlap counts against its ground truth (vis_score.GroundTruth `gt`), gathered window by window for ALL tracker rows
    (idx = arange(n), as `label_maps` does: every path then agrees bit for bit, and the end only selects rows).  On the device: `inter`
    int64 [rows, 32 * groups] (column g = ground-truth track g; one kernel call per group of 32 per window) and, per window, the
    per-frame areas int32 [n, F]; frames before a track's first window count 0.  `result` reads both back once."""

    def __init__(self, gt, device, out_size, rows):
        if (int(out_size[0]), int(out_size[1])) != tuple(gt.size):
            raise ValueError("ground_truth: its size %s is not the output size (height, width) = %s" % (tuple(gt.size), (int(out_size[0]), int(out_size[1]))))
        self.gt, self.device, self.out_size = gt, device, (int(out_size[0]), int(out_size[1]))
        # (a ground truth without tracks still yields the predictions' areas: one all-zero word, one column that stays 0)
        self.words = gt.on(device) or [torch.zeros((gt.length,) + tuple(gt.size), dtype=torch.int32, device=device).view(torch.uint32)]
        self.inter = torch.zeros(max(int(rows), 1), 32 * len(self.words), dtype=torch.int64, device=device)
        # the words' upload and the table's zero-fill are queued on this stream, the windows' kernels on another: they wait for this
        self.ready = torch.cuda.Event()
        self.ready.record(torch.cuda.current_stream(device))
        self.areas = []                                                # (f_off, frames, rows, int32 [rows, frames])

    def window(self, m, stride, frame_hw, f_off):
        """Window logits m [n, F, Hm, Wm] covering video frames [f_off, f_off + F), on the current stream."""
        from . import ops
        n, nf = int(m.shape[0]), int(m.shape[1])
        if f_off + nf > self.gt.length:
            raise RuntimeError("ground_truth: it holds %d frames, the video has reached frame %d" % (self.gt.length, f_off + nf))
        if not n:
            return
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(self.ready)
        if n > self.inter.shape[0]:
            self.inter = torch.cat([self.inter, self.inter.new_zeros(n - self.inter.shape[0], self.inter.shape[1])])
        self.inter.record_stream(cur)
        idx = torch.arange(n, dtype=torch.int32, device=self.device)
        area = None
        for j, w in enumerate(self.words):                             # (every group's call writes the same areas)
            w.record_stream(cur)
            area = ops.final_masks_overlap(m, idx, stride, frame_hw[0], frame_hw[1], self.out_size[0], self.out_size[1], w,
                                           max(1, min(32, self.gt.G - 32 * j)), f_off, self.inter[:, 32 * j:], area)[1]
        self.areas.append((f_off, nf, n, area.view(n, nf)))

    def result(self, inst, n_frames, copy=None):
        """res["pred_gt"] for the outputs whose tracker rows are `inst`: "inter" int64 [n_out, G], "pred_area" int64 [n_out, L], "gt_area"
        int64 [G, L], "iou" float64 [n_out, G] (vis_score.iou_table).  One small read-back, on stream `copy` when the path has one."""
        from .vis_score import iou_table
        if int(n_frames) != self.gt.length:
            raise ValueError("ground_truth: it holds %d frames, the video %d" % (self.gt.length, int(n_frames)))
        G, n_out = self.gt.G, len(inst)
        cur = torch.cuda.current_stream(self.device)
        rows = max([n for _, _, n, _ in self.areas] + [max(inst) + 1 if n_out else 0, self.inter.shape[0]])
        area = torch.zeros(rows, int(n_frames), dtype=torch.int32, device=self.device)
        for f_off, nf, n, a in self.areas:
            a.record_stream(cur)
            area[:n, f_off:f_off + nf] = a
        self.inter.record_stream(cur)
        inter = self.inter
        if rows > inter.shape[0]:
            inter = torch.cat([inter, inter.new_zeros(rows - inter.shape[0], inter.shape[1])])
        sel = torch.tensor(list(inst), dtype=torch.int64, device=self.device)
        dev = torch.cat([inter[sel, :G], area[sel].to(torch.int64)], 1)
        host = torch.empty(dev.shape, dtype=torch.int64, pin_memory=True)
        side = copy if copy is not None else cur
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            host.copy_(dev, non_blocking=True)
            dev.record_stream(side)
        side.synchronize()
        inter, pa = host[:, :G].clone(), host[:, G:].clone()
        return {"inter": inter, "pred_area": pa, "gt_area": self.gt.gt_area.clone(),
                "iou": torch.from_numpy(iou_table(inter.numpy(), pa.numpy(), self.gt.gt_area.numpy()))}


class FrameStore:
    """The frame source of `overlay_frames`: the frames the caller handed in, at their uploaded size and dtype (before
    `resize_on_device`), on the device, as chunks in video order -- one per push of an online session, one for a whole offline video.
    `pieces(f0, f1)` answers "frames [f0, f1)" with a list of (tensor [k, 3, h0, w0], first frame) that tile the range; a range that
    spans two chunks comes back as two pieces.  `drop_before(f)` forgets the chunks that lie wholly before frame f, so what a session
    holds is bounded by its schedule: the frames no window has emitted yet, plus less than one push."""

    def __init__(self):
        self.chunks = []                          # [first frame, tensor [n, 3, h0, w0], upload event or None, owned]

    def add(self, first, frames, ready=None, owned=True):
        """`ready`: the event behind the chunk's upload (None: the frames are there for the current stream; an event is recorded on
        it).  owned=False: the tensor may be the CALLER's memory (frames that arrived on the device are not copied), which `own()`
        replaces by a copy if it is still held."""
        if int(frames.shape[0]):
            if ready is None and frames.is_cuda:
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(frames.device))
            self.chunks.append([int(first), frames, ready, bool(owned)])

    @property
    def frames_held(self):
        return sum(int(c[1].shape[0]) for c in self.chunks)

    def drop_before(self, f):
        self.chunks = [c for c in self.chunks if c[0] + int(c[1].shape[0]) > f]

    def own(self):
        """Before control returns to the caller: a chunk that stays and may alias the caller's buffer is copied (the caller may refill it)."""
        for c in self.chunks:
            if not c[3]:
                c[1], c[3] = c[1].clone(), True
                if c[1].is_cuda:                  # (the copy runs on the current stream; a later window's painting waits for it)
                    c[2] = torch.cuda.Event()
                    c[2].record(torch.cuda.current_stream(c[1].device))

    def pieces(self, f0, f1, stream=None):
        """`stream`: the stream that will read the pieces -- it waits for their uploads and the pieces are `record_stream`ed on it.
        The upload is ordered before that stream's work transitively as well: the painting follows the window's flush, the flush its
        clips' `ready` events, the clips the per-frame stages, and those waited for the upload (or, with `resize_on_device`, for the
        resize that replaced the tensor, which waited for the whole upload).  The explicit wait costs nothing and does not lean on that."""
        out = []
        for first, t, ready, _ in self.chunks:
            a, b = max(f0, first), min(f1, first + int(t.shape[0]))
            if a < b:
                if stream is not None:
                    if ready is not None:
                        stream.wait_event(ready)
                    t.record_stream(stream)
                out.append((t[a - first:b - first], a))
        if sum(int(t.shape[0]) for t, _ in out) != f1 - f0:
            raise RuntimeError("overlay: the frame store does not hold frames [%d, %d)" % (f0, f1))
        return out


def overlay_frames(m, stride, frame_hw, out_size, geometry, labels, l_off, source, f0, style, out, o_off):
    """A window's overlay: the label map of window logits m [n, F, Hm, Wm] into labels[l_off:l_off + F] (`label_maps`: all n rows
    compete, as in every label path), then that map painted over video frames [f0, f0 + F) of `source` (a FrameStore) into
    out[o_off:o_off + F] (uint8 [>= o_off + F, Ho, Wo, 3], device) in `style` (render.Style) -- one ops.render_overlay launch per
    contiguous piece of source frames, on the stream the label map runs on (the current one).  -> `label_maps`' geometry table or None."""
    from . import ops
    geom = label_maps(m, stride, frame_hw, out_size, geometry, labels, l_off)
    nf = int(m.shape[1])
    pal = style.palette_on(m.device)
    for t, first in source.pieces(int(f0), int(f0) + nf, stream=torch.cuda.current_stream(m.device)):
        k, d = int(t.shape[0]), first - int(f0)
        ops.render_overlay(labels[l_off + d:l_off + d + k], t, pal, out, o_off + d, style.a256, style.contour)
    return geom


def rle_positions(m, idx, stride, frame_hw, out_size, geometry):
    """Run boundaries instead of dense masks (KBs instead of MBs per window) of rows `idx` of window logits m, on the host -> (pos
    [len(idx) * F, >= 1], n_pos [len(idx) * F], numpy; geometry table int32 [len(idx), F, 5] or None).  One host sync, on `n_pos.max()`."""
    from . import ops
    (fh, fw), (Ho, Wo) = frame_hw, out_size
    cap = 4 * (Ho + Wo) + 64                            # a blob crosses a column twice: generous for anything mask-like
    while True:
        if geometry:
            pos, n_pos, geom = ops.final_masks_rle_geom(m, idx, stride, fh, fw, Ho, Wo, cap)
        else:
            pos, n_pos = ops.final_masks_rle(m, idx, stride, fh, fw, Ho, Wo, cap)
        mx = int(n_pos.max())
        if mx <= cap:
            break
        cap = mx
    return pos[:, :max(mx, 1)].cpu().numpy(), n_pos.cpu().numpy(), geom.view(int(idx.numel()), int(m.shape[1]), 5).cpu() if geometry else None


def copy_stream(model):
    """The model's copy stream, created at the first call (the order streams are first used in decides their queues: `MDQE._make_streams`)."""
    if model._copy_stream is None:
        model._copy_stream = torch.cuda.Stream(model.device)
    return model._copy_stream


def to_host(cs, side, masks, copies, geom, event):
    """A window's dense masks (device, produced on stream `side`) to pinned host memory on the copy stream `cs`: `copies` = (pinned
    destination, part of `masks`) pairs.  The geometry table (or None) rides on the same stream; `event` is recorded behind both.
    -> the table in pinned memory (valid once `event` has fired), or None."""
    hgeom = None if geom is None else torch.empty(geom.shape, dtype=torch.int32, pin_memory=True)
    cs.wait_stream(side)
    with torch.cuda.stream(cs):
        for dst, src in copies:
            dst.copy_(src, non_blocking=True)
        masks.record_stream(cs)
        if geom is not None:
            hgeom.copy_(geom, non_blocking=True)
            geom.record_stream(cs)
        event.record(cs)
    return hgeom


def stitch(rows, n_frames, windows, empty, join):
    """Per output j, row rows[j] over the whole video.  `windows`: (f_off, frames, n rows the window holds, piece) in video order,
    piece[r] = row r's part for those frames; `join(parts)` concatenates.  Frames no window holds for a row -- those before the window
    in which its track first appears (mdqe/mdqe.py:442) -- are `empty(count)`.  Outputs of the same row share one object."""
    out = {}
    for r in set(rows):
        parts, at = [], 0
        for f_off, nf, n, piece in windows:
            if r < n:
                if f_off > at:
                    parts.append(empty(f_off - at))
                parts.append(piece[r])
                at = f_off + nf
        if at < n_frames or not parts:
            parts.append(empty(n_frames - at))
        out[r] = join(parts)
    return [out[r] for r in rows]


def stitch_rles(rows, n_frames, out_size, windows):
    """`stitch` of per-window RLE lists (piece[r]: one dict per frame): per output the list of its n_frames RLE dicts."""
    return stitch(rows, n_frames, windows, lambda k: [R.empty_rle(out_size) for _ in range(k)], lambda parts: sum(parts, []))


def track_geometry(rows, n_frames, out_size, windows):
    """Per output j the [n_frames] geometry of row rows[j] from the windows' geom tables: `windows` = (f_off, nf, n rows this window
    holds, geom int32 [n, nf, 5] on the host).  -> {"pred_boxes": [float32 [n_frames, 4]], "pred_areas": [int64 [n_frames]]}."""
    Ho, Wo = int(out_size[0]), int(out_size[1])
    none = torch.tensor([[0, Wo, Ho, -1, -1]], dtype=torch.int32)
    wins = [(f, nf, n, torch.as_tensor(g)) for f, nf, n, g in windows]
    geo = [R.geom_to_boxes(t) for t in stitch(rows, int(n_frames), wins, lambda k: none.repeat(k, 1), torch.cat)]   # (fresh tensors per output)
    return {"pred_boxes": [b for b, _ in geo], "pred_areas": [a for _, a in geo]}


def select_tracks(cls_clips, num_classes):
    """mdqe/mdqe.py:431-454 without the masks: the video-level class scores of every track from its per-window class rows
    (`cls_clips`, [tracks so far, K] per window) and their top-k -> (scores [k] host tensor, labels, track index of each output)."""
    total = cls_clips[-1].shape[0]
    cc = torch.stack([torch.cat([c, c.new_zeros(total - c.shape[0], c.shape[1])]) for c in cls_clips])
    out_cls = (0.75 * cc.mean(0) + 0.25 * cc.max(0)[0]).flatten().cpu()
    k = min(max(int(out_cls.gt(0.05).sum()), 10), out_cls.numel())   # (the reference's topk(max(.,10)), :449-450, assumes >= 10 scores)
    sc, ti = out_cls.topk(k, sorted=False)
    return sc, (ti % num_classes).tolist(), torch.div(ti, num_classes, rounding_mode="floor").tolist()


@dataclasses.dataclass
class EarlyMasks:
    """What `ClipMerger._early_masks` has brought to the host by the end of the video, for every track (not only the selected ones)."""
    done: object                                                      # event behind the last copy into `hosts` / the pinned tables of `geom`
    hosts: list = dataclasses.field(default_factory=list)             # dense: per track, pinned uint8 [L, Ho, Wo]
    rle: list = dataclasses.field(default_factory=list)               # RLE: per window (f_off, frames, tracks, pos, n_pos) of rle_positions
    geom: list = dataclasses.field(default_factory=list)              # per window (f_off, frames, tracks, int32 [tracks, frames, 5] host)
    labels: object = None                                             # label map: ONE pinned uint8 [L, Ho, Wo] per video (model.label_output)
    label_geom: list = dataclasses.field(default_factory=list)        # per window, as `geom`, of the labels' visible regions
    overlay: object = None                                            # overlay: ONE pinned uint8 [L, Ho, Wo, 3] per video (model.overlay_output)


def video_result(model, image_size, cls_clips, windows, frame_hw, n_frames, early=None, emit_masks=True, frame_source=None, score=None):
    """mdqe/mdqe.py:430-471.  The x4 aligned-bilinear up-sampling, sigmoid, crop (:357-358), nearest resize to the original size and
    the 0.5 threshold (:458-462) run as ONE kernel per window; windows in which an instance did not exist yet stay zero (:442).
    `early` (EarlyMasks): the masks of every tracked instance are on the host already, only the selection is left.  Without it
    (`windows`: (f_off, mean logits) per flushed window) the selected tracks' masks are produced here, in one pass and one copy.
    `score` (OverlapTables): the video's overlap counts against its ground truth, gathered at every flush on any path -> "pred_gt"."""
    sc, labels, inst = model.select_tracks(cls_clips)
    Ho, Wo = int(image_size[0]), int(image_size[1])
    res = {"image_size": (Ho, Wo), "pred_scores": sc.tolist(), "pred_labels": labels}
    if not emit_masks:
        return dict(res, pred_masks=[])
    if score is not None:                                          # (OverlapTables: the counts of every window are in; select rows, read back)
        res.update(pred_gt=score.result(inst, n_frames, model._copy_stream), pred_track_ids=list(inst))
    geometry = bool(model.geometry_output)
    labels = getattr(model, "label_output", False)
    overlay = (frame_source, model.overlay_style) if frame_source is not None and getattr(model, "overlay_output", False) else None
    if labels or overlay:
        res.update(label_result(model, inst, windows, frame_hw, n_frames, (Ho, Wo), early, geometry and bool(labels), bool(labels), overlay))
        if labels == "only":                                       # no per-track planes in either form
            return dict(res, pred_masks=[])
    rows, geoms = inst, early.geom if early is not None else []
    if early is not None and model.rle_output:
        res["pred_rles"] = stitch_rles(inst, n_frames, (Ho, Wo), [(f, nf, n, R.positions_to_rles(pos, n_pos, (Ho, Wo), nf))
                                                                  for f, nf, n, pos, n_pos in early.rle])
    elif early is not None:
        early.done.synchronize()                                   # (the geom tables ride on the mask copies' stream)
        res["pred_masks"] = [early.hosts[i].view(torch.bool)[:n_frames] for i in inst]
    else:
        sel = sorted(set(inst))
        rows = [sel.index(i) for i in inst]                        # rows of `out` = positions in sel
        out = torch.zeros(len(sel), n_frames, Ho, Wo, dtype=torch.uint8, device=model.device)
        sel_dev = torch.tensor(sel, dtype=torch.int32, device=model.device)
        for f_off, m in windows:
            cnt = sum(1 for i in sel if i < m.shape[0])           # sel is ascending: these are its first `cnt` entries
            if cnt:
                geoms.append((f_off, int(m.shape[1]), cnt,
                              dense_masks(m, sel_dev[:cnt], model.cfg.match_stride, frame_hw, (Ho, Wo), geometry, out, f_off)))
        hbuf = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)   # one D2H into pinned memory (pageable copies run at a fraction of PCIe)
        hbuf.copy_(out, non_blocking=True)
        torch.cuda.current_stream(model.device).synchronize()
        host = hbuf.view(torch.bool)
        if geometry:                                               # (the copies follow the masks' sync)
            geoms = [(f, nf, cnt, g.cpu()) for f, nf, cnt, g in geoms]
        if model.rle_output:                                       # no early path (unknown length): encode on the host
            enc = [[R.encode_dense(fm.numpy()) for fm in host[p]] for p in range(len(sel))]
            res["pred_rles"] = [enc[p] for p in rows]
        else:
            res["pred_masks"] = [host[p] for p in rows]
    if geometry:
        res.update(track_geometry(rows, n_frames, (Ho, Wo), geoms))
    return res


def label_result(model, inst, windows, frame_hw, n_frames, out_size, early, geometry, labels=True, overlay=None):
    """The label-map keys of a video's result: "pred_label_map" (uint8 [L, Ho, Wo], host; label t + 1 = tracker row t, 0 = background),
    "pred_track_ids" (the row behind output j, so pred_label_map == pred_track_ids[j] + 1 is output j's exclusive region) and, with
    geometry, "pred_label_boxes" / "pred_label_areas" of those regions.  `early`: the map is on the host already (EarlyMasks.labels);
    else it is produced here from `windows`, the same kernel over all rows of each window, in one pass and one copy.
    `overlay` = (FrameStore, render.Style): also "pred_overlay" (uint8 [L, Ho, Wo, 3], pinned host), that map painted over the frames
    (`overlay_frames`); with labels=False the map itself stays a device scratch and is not returned."""
    Ho, Wo = out_size
    host = pic = None
    if early is not None:
        early.done.synchronize()
        geoms = early.label_geom
        host = early.labels[:n_frames] if labels else None
        pic = early.overlay[:n_frames] if overlay else None
    else:
        dev = torch.empty(n_frames, Ho, Wo, dtype=torch.uint8, device=model.device)    # (the windows tile [0, n_frames): every row is written)
        if overlay:
            dpic = torch.empty(n_frames, Ho, Wo, 3, dtype=torch.uint8, device=model.device)
            geoms = [(f_off, int(m.shape[1]), int(m.shape[0]), overlay_frames(m, model.cfg.match_stride, frame_hw, (Ho, Wo), geometry, dev, f_off,
                                                                              overlay[0], f_off, overlay[1], dpic, f_off)) for f_off, m in windows]
            pic = torch.empty(dpic.shape, dtype=torch.uint8, pin_memory=True)
            pic.copy_(dpic, non_blocking=True)
        else:
            geoms = [(f_off, int(m.shape[1]), int(m.shape[0]), label_maps(m, model.cfg.match_stride, frame_hw, (Ho, Wo), geometry, dev, f_off))
                     for f_off, m in windows]
        if labels:
            host = torch.empty(dev.shape, dtype=torch.uint8, pin_memory=True)
            host.copy_(dev, non_blocking=True)
        torch.cuda.current_stream(model.device).synchronize()
        if geometry:
            geoms = [(f, nf, n, g.cpu()) for f, nf, n, g in geoms]
    res = {"pred_track_ids": list(inst)}
    if labels:
        res["pred_label_map"] = host
    if overlay:
        res["pred_overlay"] = pic
    if geometry:
        geo = track_geometry(inst, n_frames, (Ho, Wo), geoms)
        res.update(pred_label_boxes=geo["pred_boxes"], pred_label_areas=geo["pred_areas"])
    return res


class ClipMerger:
    """Incremental form of the clip loop's second half (mdqe/mdqe.py:337-366): tracker update per clip, window flushes,
    final video merge.  The tracker runs on its own HIP stream so that its small kernels and per-clip host syncs overlap
    with per-frame work the producer has already queued on the main stream."""

    tracker_cls = OverTracker               # (tests without a GPU substitute a stand-in bank, tests/_standins.py)
    EARLY_TRACKS = 48                       # tracks per video the early-mask path budgets pinned memory for

    def __init__(self, model, frame_hw, out_size, mask_hw, n_frames=None, emit_masks=True, online=None, geometry=None, frame_source=None,
                 style=None, ground_truth=None):
        self.model, self.frame_hw, self.out_size, self.mask_hw = model, frame_hw, out_size, mask_hw
        self.emit_masks = emit_masks                # False: scores / labels only (ranks > 0 of a sharded video)
        # boxes and areas of the final masks from the kernels that produce them (None: model.geometry_output; online sessions pass theirs)
        self.geometry = bool(getattr(model, "geometry_output", False) if geometry is None else geometry)
        # online ("masks" | "rle" | "labels" | "overlay"; online.OnlineVideo, CUDA only): at each flush the window's final masks -- or their
        # RLE, or their label map, or that map and its overlay -- of every current track are built and appended to `emitted`; neither the
        # logits nor a host buffer stay here (n_frames is unknown)
        self.online = online
        # False | True | "only" (model.label_output): the label map next to -- or, "only", instead of -- the per-track planes
        self.labels = getattr(model, "label_output", False) if emit_masks and not online else False
        # the overlay (model.overlay_output, online "overlay"): the label map painted over the frames of `frame_source` (a FrameStore)
        self.overlay = bool(getattr(model, "overlay_output", False)) if emit_masks and not online else online == "overlay"
        self.frame_source = frame_source
        self.style = style if style is not None else getattr(model, "overlay_style", None)
        if self.overlay and frame_source is None:
            raise ValueError("overlay output needs the frames of the whole video on this device; this path does not hold them (the sharded "
                             "driver does not offer it: rank 0 does not hold every frame)")
        # a vis_score.GroundTruth: every flushed window's final masks are counted against it (OverlapTables); None: nothing is
        self.score = None
        if ground_truth is not None:
            if n_frames is not None and int(n_frames) != ground_truth.length:
                raise ValueError("ground_truth: it holds %d frames, the video %d" % (ground_truth.length, int(n_frames)))
            if not emit_masks:
                raise ValueError("ground_truth: a merger that emits no masks cannot score them")
            if torch.device(model.device).type != "cuda":
                raise ValueError("ground_truth: the overlap counts are a device kernel's; the model is on %s (the product has no CPU path)" % (model.device,))
            self.score = OverlapTables(ground_truth, model.device, out_size, model.cfg.n_max_inst)
        self.emitted = []
        self.n_frames = n_frames                    # total frames of the video when known: enables the early mask path
        self.early = None                           # EarlyMasks, from the first window the early path takes
        # MODEL.MDQE.MERGE_ON_CPU (mdqe/mdqe.py:185-186,337,354-355; True in R50_ovis_720 / swinl_ovis): the device the window results
        # wait on for the end of the video -- a memory-placement switch, the outputs are the same.  WHEN the final masks are produced is
        # a separate choice (`model.early_masks`, default on for both settings since round 3): per flushed window, into pinned host
        # buffers under the later windows' compute -- the window's stride-4 logits are then dropped at once under EITHER setting (nothing
        # reads them again) -- or, off, in one pass + one copy at the end, which needs the logits of every window and keeps them in HBM
        # whatever MERGE_ON_CPU says.
        self.merge_on_cpu = bool(model.cfg.merge_on_cpu if model.merge_on_cpu is None else model.merge_on_cpu)
        self.early_on = bool(getattr(model, "early_masks", True))
        # The early path holds one pinned [n_frames, Ho, Wo] buffer per TRACK (the late path: per selected output).  Budget: an estimate
        # of EARLY_TRACKS tracks must fit into MDQE_EARLY_PINNED_GB (default 24) of pinned host memory, else the late path is taken for
        # this video (a 120-frame 360p video: 27.6 MB per track; one rank's view of a 1920-frame one: 442 MB per track).
        if self.early_on and n_frames is not None:
            per_track = int(n_frames) * int(out_size[0]) * int(out_size[1])
            # (the overlay's one pinned [n_frames, Ho, Wo, 3] buffer counts too)
            if per_track * (self.EARLY_TRACKS + (3 if self.overlay else 0)) > float(os.environ.get("MDQE_EARLY_PINNED_GB", "24")) * 2 ** 30:
                self.early_on = False
        self.dev = model.device
        self.use_side = self.dev.type == "cuda"
        self.main = torch.cuda.current_stream(self.dev) if self.use_side else None
        if self.use_side and model._trk_stream is None:
            model._trk_stream = torch.cuda.Stream(self.dev, priority=getattr(model, "trk_priority", 0))
        self.side = model._trk_stream if self.use_side else None
        self.side_is_current = False                # set by sharding.ReplayThread in its own thread
        self.saved, self.tracker = 0, None
        self.cls_clips, self.windows, self.f_off = [], [], 0    # windows: (f_off, mean logits) the late path still has to turn into masks
        self.done = False

    def feed(self, start, end, last, res):
        """Returns True once the last clip has been consumed."""
        return self.feed_many([(start, end, last, res)])

    def feed_many(self, items):
        """Clip results in global order.  The clips between two window flushes go to the tracker as ONE native call
        (`OverTracker.update_many`: no Python between clips -- what keeps rank 0's replay of a gathered round off the critical
        path of a sharded video).  Returns True once the last clip has been consumed."""
        cfg = self.model.cfg
        stride, win = cfg.clip_stride, cfg.n_frames_window_test
        run = []
        for it in items:
            run.append(it)
            start, last = it[0], it[2]
            if last or (start + stride >= win * (self.saved + 1)):
                self._consume(run, True, last)
                run = []
                if last:
                    break
        if run:
            self._consume(run, False, False)
        return self.done

    def _consume(self, run, flush, last):
        cfg = self.model.cfg
        T, stride, win = cfg.n_frames_test, cfg.clip_stride, cfg.n_frames_window_test
        # (a replay thread makes the tracker stream its current stream once instead of entering a stream context per clip)
        ctx = torch.cuda.stream(self.side) if self.use_side and not self.side_is_current else contextlib.nullcontext()
        with ctx:
            clips, seen = [], set()
            for start, end, _, res in run:
                if self.use_side:
                    ev = res.get("ready")
                    if ev is None:
                        self.side.wait_stream(self.main)
                    elif id(ev) not in seen:            # the clips of one decoder batch share their event
                        seen.add(id(ev))
                        self.side.wait_event(ev)
                    res["pred_masks"].record_stream(self.side)
                clips.append(Clips(range(start, end), res))
            if self.tracker is None:
                self.tracker = self.tracker_cls(cfg.n_max_inst, T, win, stride, cfg.num_classes, cfg.mask_dim, cfg.hidden_dim,
                                                self.mask_hw, self.dev, cfg.apply_cls_thres)
            self.tracker.update_many(clips)
            if flush:
                c, m = self.tracker.get_result(is_last_clip=last)   # m: mean logits [n, F, Hm, Wm] of this window
                self.cls_clips.append(c)
                m = m.contiguous()
                if self.score is not None:                          # on every path, at the flush: the counts do not wait for the masks' form
                    self.score.window(m, cfg.match_stride, self.frame_hw, self.f_off)
                # only the late path keeps the window's stride-4 logits for the rest of the video (under either MERGE_ON_CPU setting)
                if not self.emit_masks:
                    pass
                elif self.online:
                    self.emitted.append(self._online_window(c, m))
                elif self.use_side and self.n_frames is not None and (self.early_on or self.model.rle_output):
                    self._early_masks(m)
                else:
                    self.windows.append((self.f_off, m))
                self.f_off += m.shape[1]
                self.saved += 1
        self.done = self.done or bool(last)

    def _early_masks(self, m):
        """Final masks of EVERY instance tracked so far for the window just flushed (m: [n, F, Hm, Wm] mean logits), copied to
        pinned host memory on a copy stream while later windows compute; finish() then only selects rows.  A few rows may
        be produced in vain (instances that miss the final top-k).  One pinned buffer per track (no re-allocation as tracks
        appear; the caching host allocator recycles the blocks of the previous call).  model.rle_output: the run boundaries instead."""
        model = self.model
        n, nf = int(m.shape[0]), int(m.shape[1])
        Ho, Wo = int(self.out_size[0]), int(self.out_size[1])
        cs = copy_stream(model)
        if self.early is None:
            self.early = EarlyMasks(done=torch.cuda.Event())
        early = self.early
        if self.labels or self.overlay:
            # one pinned [L, Ho, Wo] map per video, whatever the number of tracks; a window without tracks is written too (zeros).  The
            # overlay: one pinned [L, Ho, Wo, 3] picture per video the same way; without label_output the map is a device scratch.
            geometry = self.geometry and bool(self.labels)
            dev = torch.empty(nf, Ho, Wo, dtype=torch.uint8, device=self.dev)
            copies, pic = [], None
            if self.labels:
                if early.labels is None:
                    early.labels = model.pinned_mask_buffer((int(self.n_frames), Ho, Wo))
                copies.append((early.labels[self.f_off:self.f_off + nf], dev))
            if self.overlay:
                if early.overlay is None:
                    early.overlay = model.pinned_mask_buffer((int(self.n_frames), Ho, Wo, 3))
                pic = torch.empty(nf, Ho, Wo, 3, dtype=torch.uint8, device=self.dev)
                geom = overlay_frames(m, model.cfg.match_stride, self.frame_hw, self.out_size, geometry, dev, 0, self.frame_source, self.f_off,
                                      self.style, pic, 0)
                copies.append((early.overlay[self.f_off:self.f_off + nf], pic))
            else:
                geom = label_maps(m, model.cfg.match_stride, self.frame_hw, self.out_size, geometry, dev, 0)
            geom = to_host(cs, self.side, dev, copies, geom, early.done)
            if pic is not None:
                pic.record_stream(cs)
            if geometry:
                early.label_geom.append((self.f_off, nf, n, geom))
        if not n or self.labels == "only":
            return
        args = (m, torch.arange(n, dtype=torch.int32, device=self.dev), model.cfg.match_stride, self.frame_hw, self.out_size, self.geometry)
        if model.rle_output:
            pos, n_pos, geom = rle_positions(*args)
            early.rle.append((self.f_off, nf, n, pos, n_pos))
        else:
            while len(early.hosts) < n:             # a new track: its own pinned [L, Ho, Wo] buffer, zero before its first window (:442)
                hbuf = model.pinned_mask_buffer((int(self.n_frames), Ho, Wo))
                if self.f_off > 0:
                    hbuf[:self.f_off].zero_()
                early.hosts.append(hbuf)
            dev = torch.empty(n, nf, Ho, Wo, dtype=torch.uint8, device=self.dev)
            geom = to_host(cs, self.side, dev, [(h[self.f_off:self.f_off + nf], d) for h, d in zip(early.hosts, dev)], dense_masks(*args, dev, 0),
                           early.done)
        if self.geometry:
            early.geom.append((self.f_off, nf, n, geom))

    def _online_window(self, c, m):
        """Online mode: the window just flushed (c: class rows [n, K] on the host, m: mean logits [n, F, Hm, Wm]) as a record --
        frames, class rows, and the final masks of tracks 0..n-1: dense masks copied to a pinned host buffer on the copy stream
        (`ready` fires when they and the geometry table are there), or their RLE dicts, or ("labels") their label map uint8 [F, Ho, Wo],
        copied the same way, with the geometry of the labels' visible regions, or ("overlay") that map and its overlay uint8 [F, Ho, Wo, 3]."""
        n, nf = int(m.shape[0]), int(m.shape[1])
        Ho, Wo = int(self.out_size[0]), int(self.out_size[1])
        rec = {"frames": (self.f_off, self.f_off + nf), "cls_probs": c, "ready": None}
        geom = torch.zeros((0, nf, 5), dtype=torch.int32) if self.geometry else None    # (the table of a window without tracks)
        args = (m, torch.arange(n, dtype=torch.int32, device=self.dev), self.model.cfg.match_stride, self.frame_hw, self.out_size, self.geometry)
        if self.online in ("labels", "overlay"):                     # one plane per frame; a window without tracks is all background
            cs = copy_stream(self.model)
            dev = torch.empty(nf, Ho, Wo, dtype=torch.uint8, device=self.dev)
            host = self.model.pinned_mask_buffer((nf, Ho, Wo))
            copies, pic = [(host, dev)], None
            if self.overlay:                                         # ... and its picture over the frames pushed (a window without tracks: the frames)
                pic = torch.empty(nf, Ho, Wo, 3, dtype=torch.uint8, device=self.dev)
                geom = overlay_frames(m, self.model.cfg.match_stride, self.frame_hw, self.out_size, self.geometry, dev, 0, self.frame_source,
                                      self.f_off, self.style, pic, 0)
                rec["overlay"] = self.model.pinned_mask_buffer((nf, Ho, Wo, 3))
                copies.append((rec["overlay"], pic))
            else:
                geom = label_maps(m, self.model.cfg.match_stride, self.frame_hw, self.out_size, self.geometry, dev, 0)
            rec["ready"] = torch.cuda.Event()
            geom = to_host(cs, self.side, dev, copies, geom, rec["ready"])
            if pic is not None:
                pic.record_stream(cs)
            rec["labels"] = host
        elif self.online == "rle":
            rec["rles"] = []
            if n:
                pos, n_pos, geom = rle_positions(*args)
                rec["rles"] = R.positions_to_rles(pos, n_pos, (Ho, Wo), nf)
        elif not n:
            rec["masks"] = torch.zeros((0, nf, Ho, Wo), dtype=torch.bool)
        else:
            cs = copy_stream(self.model)
            dev = torch.empty(n, nf, Ho, Wo, dtype=torch.uint8, device=self.dev)
            geom = dense_masks(*args, dev, 0)
            host = self.model.pinned_mask_buffer((n, nf, Ho, Wo))
            rec["ready"] = torch.cuda.Event()
            geom = to_host(cs, self.side, dev, [(host, dev)], geom, rec["ready"])
            rec["masks"] = host.view(torch.bool)
        if self.geometry:
            rec["geom"] = geom
        return rec

    def finish(self):
        if self.use_side:
            self.main.wait_stream(self.side)
            for _, m in self.windows:
                m.record_stream(self.main)
        kw = {"frame_source": self.frame_source} if self.overlay else {}
        if self.score is not None:
            kw["score"] = self.score
        return self.model.inference_video(self.out_size, self.cls_clips, self.windows, self.frame_hw, self.f_off, early=self.early,
                                          emit_masks=self.emit_masks, **kw)
