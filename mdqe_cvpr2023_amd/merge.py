"""The second half of the clip loop (mdqe/mdqe.py:337-366, 430-471): `ClipMerger` (tracker update per clip, window flushes) and
`video_result` (the video's result from the flushed windows); `meta_arch.MDQE` keeps its entry points as delegates.
Which forms a video produces is resolved ONCE, into a `Forms` record (from the model's flags offline, from `emit` online): per-track
planes (dense or run boundaries), the label map (one uint8 plane per frame that names the track owning each pixel; its frames are
disjoint between windows, so it needs no `stitch`), its overlay (that map painted over the frames the caller handed in, `FrameStore`,
uint8 [F, Ho, Wo, 3]), per-track crops cut from those frames along the map's visible regions (`crop_frames`, render.Crops; offline they
gather in one device table per video, `CropTable`), the tracks' paths (the centroid of each visible region per frame, kept over the
windows in a `PathTable`: an output, and what an overlay's trails are drawn from), the tracks' outline polygons (the rings around each
visible region, traced on the device and brought to the host per window: `polygon_rings`, polygons.TrackPolygons) and whose geometry.  A flushed window becomes those forms in ONE function,
`build_window`; the three paths differ in the destination only: per window into per-video pinned memory (`_early_masks`), per window
as a record (`_online_window`), or all windows into whole-video device buffers with one copy at the end (`video_result`).  Shared
beside it: `to_host` (the hop on the copy stream), `rle.positions_to_rles`, `stitch`, `result_head` / `track_geometry` (a result's keys).
The occlusion table (`occlusion_counts`, `occlusion_result`: per window how much of each track's mask every track owns) is a form of its
own that needs none of the others.
`OverlapTables` is not an output form but a score: with a ground truth handed in (vis_score.GroundTruth), every flushed window's final
masks are counted against it where they are decided (ops.final_masks_overlap) -- "pred_gt", beside whatever form the masks take."""
import contextlib
import dataclasses
import os

import torch

from . import rle as R
from .tracking import Clips, OverTracker


@dataclasses.dataclass(frozen=True)
class Forms:
    """Which output forms a video produces, resolved ONCE and read by every path; the only reader of the model's output flags here."""
    planes: object = None                 # "dense" | "rle" | None: the per-track planes
    labels: bool = False                  # the label map is RETURNED (an overlay without it keeps the map as a device scratch)
    overlay: bool = False                 # the label map painted over the frames
    plane_geometry: bool = False          # boxes and areas of the planes ...
    label_geometry: bool = False          # ... and of the labels' visible regions
    early_always: bool = False            # model.rle_output: the early path even with model.early_masks off, with or without planes
    surface: bool = False                 # the overlay is painted onto the decoder surfaces handed in: a YuvFrames, not RGB pixels
    crops: bool = False                   # per-track chips cut from the frames (render.Crops; the map and its table: a device scratch if not returned)
    paths: bool = False                   # per-track centroids and moments of the map's visible regions (PathTable; the map: a device scratch if not returned)
    polygons: bool = False                # per-track outline polygons of the map's visible regions (polygons.Polygons; the map: a device scratch if not returned)
    occlusion: bool = False               # the occlusion table of the window's tracks, int32 [n, F, n] (ops.final_occlusion), beside any other form
    matte: bool = False                   # the soft matte of the window's tracks, one uint8 plane per frame (render.Matte), beside any other form

    @classmethod
    def _of(cls, model, geometry, planes, labels, overlay, early_always=False, surface=False, crops=False, paths=False, matte=False,
            polygons=False, occlusion=False):
        """geometry None: the model's flag.  It describes the planes where there are planes, and the labels' regions where the map is returned."""
        g = bool(getattr(model, "geometry_output", False) if geometry is None else geometry)
        return cls(planes, labels, overlay, g and planes is not None, g and labels, early_always, bool(overlay and surface), bool(crops),
                   bool(paths), matte=bool(matte), polygons=bool(polygons), occlusion=bool(occlusion))

    @classmethod
    def of_model(cls, model, emit_masks=True, geometry=None):
        """Offline.  emit_masks=False (ranks > 0 of a sharded video): nothing.  Stand-in models may lack the newer flags."""
        if not emit_masks:
            return cls()
        lab, rle = getattr(model, "label_output", False), bool(getattr(model, "rle_output", False))
        pic = getattr(model, "overlay_output", False)
        return cls._of(model, geometry, None if lab == "only" else "rle" if rle else "dense", bool(lab), bool(pic), rle, pic == "surface",
                       getattr(model, "crop_output", None) is not None, bool(getattr(model, "path_output", False)),
                       getattr(model, "matte_output", None) is not None, getattr(model, "polygon_output", None) is not None,
                       occlusion=bool(getattr(model, "occlusion_output", False)))

    @classmethod
    def of_emit(cls, emit, geometry=False, model=None, surface=False, crops=False, paths=False, matte=False, polygons=False,
                occlusion=False):
        """Online ("masks" | "rle" | "labels" | "overlay"; surface: the overlay onto the surfaces pushed; crops: chips beside it; paths:
        centroids and moments beside it; polygons: outline polygons beside it; occlusion: the occlusion table beside it)."""
        lab = emit in ("labels", "overlay")
        return cls._of(model, geometry, None if lab else {"masks": "dense", "rle": "rle"}[emit], lab, emit == "overlay", surface=surface,
                       crops=crops, paths=paths, matte=matte, polygons=polygons, occlusion=occlusion)


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
    holds is bounded by its schedule: the frames no window has emitted yet, plus less than one push.
    A chunk may also be a preprocess.YuvFrames, the decoder surfaces themselves (1.5 bytes per pixel for NV12 instead of 3): what a
    surface overlay paints on.  A piece is then a YuvFrames of k surfaces; `surface` remembers the kind of the first such chunk
    (YuvFrames.meta()) and every later one must be of that kind."""

    def __init__(self):
        self.chunks = []                          # [first frame, tensor [n, 3, h0, w0] or YuvFrames, upload event or None, owned]
        self.surface = None                       # (height, width, fmt, matrix, full_range, order) of the first YuvFrames chunk

    def add(self, first, frames, ready=None, owned=True):
        """`ready`: the event behind the chunk's upload (None: the frames are there for the current stream; an event is recorded on
        it).  owned=False: the tensor may be the CALLER's memory (frames that arrived on the device are not copied), which `own()`
        replaces by a copy if it is still held."""
        if not torch.is_tensor(frames):           # decoder surfaces
            if self.surface is None:
                self.surface = frames.meta()
            elif frames.meta() != self.surface:
                raise ValueError("overlay: surfaces of (height, width, fmt, matrix, full_range, order) = %s follow surfaces of %s; one "
                                 "video's surfaces are of one kind (start another session for another stream)" % (frames.meta(), self.surface))
        if len(frames):
            if ready is None and frames.is_cuda:
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(frames.device))
            self.chunks.append([int(first), frames, ready, bool(owned)])

    @property
    def frames_held(self):
        return sum(len(c[1]) for c in self.chunks)

    def drop_before(self, f):
        self.chunks = [c for c in self.chunks if c[0] + len(c[1]) > f]

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
            a, b = max(f0, first), min(f1, first + len(t))
            if a < b:
                if stream is not None:
                    if ready is not None:
                        stream.wait_event(ready)
                    t.record_stream(stream)
                out.append((t[a - first:b - first], a))
        if sum(len(t) for t, _ in out) != f1 - f0:
            raise RuntimeError("overlay: the frame store does not hold frames [%d, %d)" % (f0, f1))
        return out


def overlay_frames(m, stride, frame_hw, out_size, geometry, labels, l_off, source, f0, style, cls, out, o_off, paths=None, plate=None):
    """A window's overlay: the label map of window logits m [n, F, Hm, Wm] into labels[l_off:l_off + F] (`label_maps`: all n rows
    compete, as in every label path), then that map painted over video frames [f0, f0 + F) of `source` (a FrameStore) into
    out[o_off:o_off + F] (uint8 [>= o_off + F, Ho, Wo, 3], device) in `style` (render.Style) -- one ops.render_overlay launch per
    contiguous piece of source frames, on the stream the label map runs on (the current one).  A surface picture (`out` a device
    YuvFrames; the pieces are then the surfaces handed in, of the output size): painted in the YUV domain, one
    ops.render_overlay_yuv launch per piece, with the palette in the surfaces' samples.  A style with a mosaic (style.mosaic): the
    same launches of ops.render_mosaic / ops.render_mosaic_yuv with the style's action table; `cls`, the window's class rows [n, K]
    on the host, is what a style with `classes` builds that table from.  A style with a blur (style.blur): the same launches of
    ops.render_blur / ops.render_blur_yuv with that table, the style's tap tables (style.taps_on, style.taps_c_on) and its
    blur_edge ("stop": the blur that stays inside what it blurs; with a margin, inside the grown map's regions).  A style that
    replaces (style.replace): behind the label map one ops.final_matte launch sweeps the same logits into a device scratch [F, Ho, Wo]
    -- the matte of the rows the style's `takes` table selects, with the style's matte_gain -- and the painter launches are
    ops.render_replace / ops.render_replace_yuv with that matte and the style's backdrop (a backdrop picture must have the output's size).  A style that annotates (style.annotates: track boxes,
    captions) takes the geometry table from `label_maps` whether or not `geometry` asks for it and, behind the painter launches, runs
    one ops.annotate / ops.annotate_yuv launch per piece in place on the painted frames, on the same stream, with the captions made
    from `cls`; nothing is read back.  `paths` (a PathTable whose `begin` has been called for this window): the window's centroids are
    made behind the label map (`PathTable.run`), and a style with a trail (style.trails) has one ops.render_trails /
    ops.render_trails_yuv launch per piece draw them between the painter and the annotations, so plates stay legible.  A style with a
    margin (style.grow > 0, and a window with tracks): behind the label map (and `paths.run`) one ops.grow_labels launch dilates the
    labels of the style's `grows` table into a fresh device scratch [F, Ho, Wo], and the painter launches take that scratch's frames
    in place of the label map's: contours and tints are those of the grown map.  Everything else -- `labels` itself, the geometry
    table, the centroids, trails, boxes and captions -- stays that of the map as made; with grow == 0 nothing is allocated or launched.
    A style that removes objects (style.plate: replace="tracks" with backdrop="plate") needs `plate`, the video's Plate: between the label
    map and the painters the window's frames teach it (`Plate.observe`: an optional ops.grow_labels launch for the plate's margin, then
    one ops.plate_update / ops.plate_update_yuv launch per piece, a window without tracks included) and its picture of the scene
    (`Plate.picture`: one ops.plate_picture / ops.plate_picture_yuv launch) is the backdrop the painters composite; with any other
    backdrop nothing of this is made or launched.
    -> `label_maps`' geometry table where `geometry` asks for it, else None."""
    from . import ops
    notes = style.annotates and int(m.shape[0]) > 0
    geom = label_maps(m, stride, frame_hw, out_size, geometry or notes, labels, l_off)
    n, nf = int(m.shape[0]), int(m.shape[1])
    if paths is not None:
        paths.run(labels, l_off)
    surface = not torch.is_tensor(out)
    pal = style.palette_yuv_on(m.device, *out.meta()[2:]) if surface else style.palette_on(m.device)
    act = style.actions_on(m.device, cls) if style.mosaic is not None or style.blur is not None or style.replace is not None else None
    matte = back = None
    if style.replace is not None:
        matte = replace_matte(m, stride, frame_hw, out_size, style, cls)
        if not style.plate:
            back = style.backdrop_yuv_on(m.device, *out.meta()[2:]) if surface else style.backdrop_on(m.device)
        elif plate is None:
            raise RuntimeError("overlay: a style with backdrop='plate' needs the video's Plate (merge.plate_of)")
    taps = style.taps_on(m.device) if style.blur is not None else None
    taps_c = style.taps_c_on(m.device) if taps is not None and surface else None
    edge = {"edge": style.blur_edge} if style.blur_edge != "bleed" else {}     # ("bleed": the blur's calls exactly as they were)
    grown = None
    if style.grow > 0 and n:
        grown = ops.grow_labels(labels[l_off:l_off + nf], style.grows_on(m.device, cls), style.grow,
                                torch.empty((nf,) + tuple(labels.shape[1:]), dtype=torch.uint8, device=m.device))
    pieces = source.pieces(int(f0), int(f0) + nf, stream=torch.cuda.current_stream(m.device))
    if matte is not None and style.plate:
        plate.observe(labels, l_off, nf, [(t, first - int(f0)) for t, first in pieces])
        back = plate.picture()
    for t, first in pieces:
        k, d = len(t), first - int(f0)
        lab = labels[l_off + d:l_off + d + k] if grown is None else grown[d:d + k]
        if matte is not None and surface:
            ops.render_replace_yuv(lab, t, pal, act, matte[d:d + k], back, out, o_off + d, style.a256, style.contour, style.replace)
        elif matte is not None:
            ops.render_replace(lab, t, pal, act, matte[d:d + k], back, out, o_off + d, style.a256, style.contour, style.replace)
        elif taps is not None and surface:
            ops.render_blur_yuv(lab, t, pal, act, taps, taps_c, out, o_off + d, style.a256, style.contour, **edge)
        elif taps is not None:
            ops.render_blur(lab, t, pal, act, taps, out, o_off + d, style.a256, style.contour, **edge)
        elif act is not None and surface:
            ops.render_mosaic_yuv(lab, t, pal, act, out, o_off + d, style.a256, style.contour, style.cell)
        elif act is not None:
            ops.render_mosaic(lab, t, pal, act, out, o_off + d, style.a256, style.contour, style.cell)
        elif surface:
            ops.render_overlay_yuv(lab, t, pal, out, o_off + d, style.a256, style.contour)
        else:
            ops.render_overlay(lab, t, pal, out, o_off + d, style.a256, style.contour)
    if style.trails and n:
        if paths is None or paths.trail != style.trail:
            raise RuntimeError("overlay: a style with trail=%d needs the video's PathTable of that trail (merge.path_table)" % style.trail)
        for t, first in pieces:                                       # (a piece's frame f is column trail + d + f of the table)
            k, d = len(t), first - int(f0)
            (ops.render_trails_yuv if surface else ops.render_trails)(out, paths.pts, n, pal, k, o_off + d, paths.trail + d, style.trail,
                                                                      style.trail_width)
    if notes:
        ink = style.ink_yuv_on(m.device, *out.meta()[2:]) if surface else style.ink_on(m.device)
        text, font = style.captions_on(m.device, cls, n), style.font_on(m.device)
        for t, first in pieces:
            k, d = len(t), first - int(f0)
            g = geom if k == nf else geom[:, d:d + k].contiguous()     # (the table's rows are k * F + f of the frames of ONE call)
            (ops.annotate_yuv if surface else ops.annotate)(out, g, n, pal, ink, text, font, o_off + d, style.box, style.text_scale,
                                                            style.min_area)
    return geom if geometry else None


def check_replace(style, out_size, surface):
    """What a replace style cannot be painted with, refused with the remedy (a ClipMerger asks before the first clip runs).  surface:
    False, True, or the surfaces' format where it is known."""
    from .preprocess import YuvFrames
    Ho, Wo = (int(v) for v in out_size)
    b = style.backdrop
    if style.plate:                                 # object removal: what the plate starts from is checked as a backdrop picture is
        b = style.plate_init
        if isinstance(b, YuvFrames):
            if not surface:
                raise ValueError("overlay style: plate_init is a YuvFrames surface but the session paints RGB pictures; give a uint8 "
                                 "tensor [Ho, Wo, 3], or run the session with surface=True")
            if (b.height, b.width) != (Ho, Wo) or (isinstance(surface, str) and b.fmt != surface):
                raise ValueError("overlay style: the plate_init surface is %d x %d %s but the output is %d x %d%s; resize the picture to "
                                 "the output's size (height, width) and convert it to the session's format"
                                 % (b.height, b.width, b.fmt, Ho, Wo, " " + surface if isinstance(surface, str) else ""))
        elif torch.is_tensor(b):
            if surface:
                raise ValueError("overlay style: plate_init is an RGB picture but the session paints decoder surfaces; give a "
                                 "preprocess.YuvFrames of one surface of the session's kind, or run the session with surface=False")
            if tuple(b.shape[:2]) != (Ho, Wo):
                raise ValueError("overlay style: the plate_init picture is %d x %d but the output is %d x %d; resize the picture to the "
                                 "output's size (height, width)" % (b.shape[0], b.shape[1], Ho, Wo))
        return
    if isinstance(b, YuvFrames):
        if not surface:
            raise ValueError("overlay style: the backdrop is a YuvFrames surface but the session paints RGB pictures; give a uint8 "
                             "tensor [Ho, Wo, 3] or three ints, or run the session with surface=True")
        if (b.height, b.width) != (Ho, Wo) or (isinstance(surface, str) and b.fmt != surface):
            raise ValueError("overlay style: the backdrop surface is %d x %d %s but the output is %d x %d%s; resize the picture to the "
                             "output's size (height, width) and convert it to the session's format"
                             % (b.height, b.width, b.fmt, Ho, Wo, " " + surface if isinstance(surface, str) else ""))
    elif torch.is_tensor(b):
        if surface:
            raise ValueError("overlay style: the backdrop is an RGB picture but the session paints decoder surfaces; give a "
                             "preprocess.YuvFrames of one surface of the session's kind or three ints, or run the session with surface=False")
        if tuple(b.shape[:2]) != (Ho, Wo):
            raise ValueError("overlay style: the backdrop picture is %d x %d but the output is %d x %d; resize the picture to the output's "
                             "size (height, width)" % (b.shape[0], b.shape[1], Ho, Wo))


def replace_matte(m, stride, frame_hw, out_size, style, cls):
    """The matte a replace style composites with: of window logits m [n, F, Hm, Wm], the rows `style.takes` selects (`cls`: the window's
    class rows on the host, for a style with `classes`), with style.matte_gain, into a fresh device scratch uint8 [F, Ho, Wo] on the
    current stream (ops.final_matte: one more sweep of the logits the label map was made from).  What the style cannot be painted with
    was refused when the merger was made (`check_replace`)."""
    from . import ops
    (fh, fw), (Ho, Wo) = frame_hw, out_size
    n, nf = int(m.shape[0]), int(m.shape[1])
    idx = torch.arange(n, dtype=torch.int32, device=m.device)
    matte = torch.empty((nf, Ho, Wo), dtype=torch.uint8, device=m.device)
    return ops.final_matte(m, idx, stride, fh, fw, Ho, Wo, matte, 0, style.takes_on(m.device, cls), style.matte_gain)


def crop_frames(n, nf, labels, l_off, geom, source, f0, spec, out, rects, c_off):
    """A window's crops: for the window's n rows and the frames `spec` (render.Crops) takes among video frames [f0, f0 + nf), the chips
    into out[:n, c_off:] and their rects into rects[:n, c_off:] (device), cut from the frames of `source` (a FrameStore) by the label map
    labels[l_off:l_off + nf] and its geometry table geom [n, nf, 5] (`label_maps`) -- one ops.track_crops launch per contiguous piece
    of source frames (ops.track_crops_yuv where the store holds decoder surfaces), the table sliced per piece as `overlay_frames` does
    for the annotation pass and the first frame taken counted from the piece's own start, on the current stream.  -> chips written."""
    from . import ops
    done = 0
    if not n:
        return len(spec.taken(f0, int(f0) + nf))
    for t, first in source.pieces(int(f0), int(f0) + nf, stream=torch.cuda.current_stream(labels.device)):
        k, d = len(t), first - int(f0)
        fst = spec.first_in(first)
        cnt = len(range(fst, k, spec.every))
        if cnt:
            g = geom if k == nf else geom[:, d:d + k].contiguous()     # (the table's rows are k * F + f of the frames of ONE call)
            fn = ops.track_crops if torch.is_tensor(t) else ops.track_crops_yuv
            fn(labels[l_off + d:l_off + d + k], t, g, n, spec.size, out, c_off + done, rects, fst, spec.every, spec.pad256, spec.min_area,
               spec.cutout, spec.fill)
        done += cnt
    return done


class CropTable:
    """A whole video's crops on the device (the offline paths): chips uint8 [rows, Lc, Sh, Sw, 3] and rects int32 [rows, Lc, 4] for the
    tracker rows seen so far, Lc = ceil(L / every) -- rows * Lc * Sh * Sw * 3 bytes, which `every` scales.  Every window's launches write
    straight into it; a row that appears grows the table, and the frames before its first window hold `fill` and the rect (0, 0, -1, -1)
    (`stitch`'s rule for absent rows).  `result` selects the outputs' rows and reads them back once."""

    def __init__(self, spec, n_frames, device):
        self.spec, self.n_frames, self.device = spec, int(n_frames), device
        self.out = self.rects = None

    def _blank(self, rows):
        sh, sw = self.spec.size
        out = torch.tensor(self.spec.fill, dtype=torch.uint8, device=self.device).expand(rows, self.spec.count(self.n_frames), sh, sw, 3).contiguous()
        rects = torch.tensor([0, 0, -1, -1], dtype=torch.int32, device=self.device).expand(rows, self.spec.count(self.n_frames), 4).contiguous()
        return out, rects

    def rows(self, n):
        """The table with at least n rows (a few more: a video's tracks appear over its first windows), on the current stream."""
        have = 0 if self.out is None else int(self.out.shape[0])
        if n > have or self.out is None:
            out, rects = self._blank(max(n, 1) + 3 - have)
            self.out, self.rects = (out, rects) if self.out is None else (torch.cat([self.out, out]), torch.cat([self.rects, rects]))
        return self.out, self.rects

    def result(self, inst):
        """{"pred_crops": uint8 [n_out, Lc, Sh, Sw, 3], "pred_crop_rects": int32 [n_out, Lc, 4]} in pinned host memory for the outputs whose
        tracker rows are `inst`, and "pred_crop_frames", the video frames of the Lc columns."""
        cur = torch.cuda.current_stream(self.device)
        out, rects = self.rows(max(list(inst) + [0]) + 1)
        for t in (out, rects):
            t.record_stream(cur)
        sel = torch.tensor(list(inst), dtype=torch.int64, device=self.device)
        dev = (out[sel], rects[sel])
        host = tuple(torch.empty(d.shape, dtype=d.dtype, pin_memory=True) for d in dev)
        for h, d in zip(host, dev):
            h.copy_(d, non_blocking=True)
        cur.synchronize()
        return {"pred_crops": host[0], "pred_crop_rects": host[1], "pred_crop_frames": self.spec.taken(0, self.n_frames)}


class PathTable:
    """Where each tracker row has been: the history a trail is drawn from and the `paths` output.  On the device `pts` int32 [255,
    trail + Fmax, 2], (-1, -1) = absent: columns [0, trail) hold the `trail` frames before the current window, columns [trail, trail +
    F) the window's centroids (ops.label_centroids with p_off = trail; `mom`: the window's moments int64 [n, F, 3]).  A label is a
    tracker row + 1 and rows are stable across windows, so a row of the table is one track's path.  Per window `begin` moves the last
    `trail` columns to the front (through a copy of them: source and destination overlap) and blanks the window's columns of the rows
    the window does not hold -- a track that appears later starts without a past -- and `run`, behind the label map, fills in the
    centroids.  The history is bounded by `trail`: the table does not grow with the video.  keep=True (the offline paths): each
    window's centroids and moments wait on the device, 32 bytes per track and frame, for one read-back at the end (`result`)."""
    ROWS = 255

    def __init__(self, trail, min_area, device, keep=False):
        self.trail, self.min_area, self.device = int(trail), int(min_area), device
        self.pts = self.mom = self.cen = None
        self.n = self.nf = 0
        self.windows = [] if keep else None                            # (f_off, frames, rows, centroids [n, F, 2], moments [n, F, 3]) on the device

    def begin(self, n, nf):
        """The table made ready for a window of n rows and nf frames, on the current stream.  -> (the window's centroids int32 [n, nf, 2]
        -- a copy of the table's columns of its own, since the next window moves those while this one may still be on its way to the
        host -- and its moments int64 [n, nf, 3]): what `run` fills in."""
        T, held = self.trail, self.nf
        if self.pts is None or self.pts.shape[1] < T + nf:
            new = torch.full((self.ROWS, T + max(nf, 1), 2), -1, dtype=torch.int32, device=self.device)
            if self.pts is not None and T:
                new[:, :T] = self.pts[:, held:held + T]
            self.pts = new
        else:
            if T and held:
                self.pts[:, :T] = self.pts[:, held:held + T].clone()
            if n < self.ROWS and nf:
                self.pts[n:, T:T + nf] = -1
        self.n, self.nf = int(n), int(nf)
        self.mom = torch.empty((self.n, self.nf, 3), dtype=torch.int64, device=self.device)
        self.cen = torch.empty((self.n, self.nf, 2), dtype=torch.int32, device=self.device)
        return self.cen, self.mom

    def run(self, labels, l_off):
        """The centroids of the window `begin` announced, from its label map labels[l_off:l_off + nf], on the current stream."""
        from . import ops
        if self.n and self.nf:
            ops.label_centroids(labels[l_off:l_off + self.nf], self.n, self.min_area, self.mom, self.pts, self.trail)
            self.cen.copy_(self.pts[:self.n, self.trail:self.trail + self.nf])

    def keep(self, f_off):
        if self.windows is not None:
            self.windows.append((int(f_off), self.nf, self.n, self.cen, self.mom))

    def result(self, inst, n_frames):
        """`path_result` of the windows kept, read back once."""
        cur = torch.cuda.current_stream(self.device)
        for _, _, _, p, q in self.windows:
            p.record_stream(cur)
            q.record_stream(cur)
        return path_result(inst, n_frames, [(f, nf, n, p.cpu(), q.cpu()) for f, nf, n, p, q in self.windows])


def path_table(forms, style, device, keep=False):
    """The PathTable of a video with `forms` and overlay style `style`, or None where neither a trail is drawn nor paths are asked
    for.  An overlay's table has the style's trail and min_area (the one its boxes and captions use); without an overlay: 0 and 0."""
    drawn = forms.overlay and style is not None
    trail = style.trail if drawn else 0
    if not forms.paths and not trail:
        return None
    return PathTable(trail, style.min_area if drawn else 0, device, keep)


class Plate:
    """The background plate of one video on one device: what object removal (render.Style(replace="tracks", backdrop="plate")) shows
    in place of the tracks.  State on the output grid (the rule: include/mdqe_hip.h, above mdqe_plate_update_u8): RGB `state` int32
    [Ho, Wo, 4], cells (P_0, P_1, P_2, n); surfaces (`kind`: the YuvFrames.meta() of the session's surfaces) `state` int32 [H, W, 2] and
    `state_c` int32 [ceil(H/2), ceil(W/2), 4].  All zero when fresh, or P = 256 * value and n = 1 everywhere from style.plate_init.
    `observe` teaches it a window's frames where the window's label map -- grown by style.plate_margin into `scratch` -- is free;
    `picture` makes the backdrop the painters take, into `back`, which the video keeps and reuses.  The state, the backdrop and the
    scratch (one window of labels) are made once: nothing grows with the video.  It belongs to the video, not to the style, which
    sessions share."""

    def __init__(self, style, out_size, device, kind=None):
        from .preprocess import YuvFrames
        self.style, self.device, self.kind = style, device, kind
        H, W = int(out_size[0]), int(out_size[1])
        i32 = dict(dtype=torch.int32, device=device)
        init = style.plate_init_on(device) if style.plate_init is not None else None
        self.state_c = self.scratch = None
        if kind is None:
            self.state = torch.zeros(H, W, 4, **i32)
            self.back = torch.empty(H, W, 3, dtype=torch.uint8, device=device)
            self.fill = style.plate_fill_on(device)
            if init is not None:
                self.state[..., :3] = init.to(torch.int32) * 256
                self.state[..., 3] = 1
        else:
            ch, cw = (H + 1) // 2, (W + 1) // 2
            self.state, self.state_c = torch.zeros(H, W, 2, **i32), torch.zeros(ch, cw, 4, **i32)
            self.back = YuvFrames.empty(1, H, W, fmt=kind[2], device=device, matrix=kind[3], full_range=kind[4], order=kind[5])
            self.fill = style.plate_fill_yuv_on(device, *kind[2:])
            if init is not None:
                def values(t):                     # samples as int32: a P010 word's value is word >> 6
                    v = t.to(torch.int32) if t.dtype == torch.uint8 else t.view(torch.int16).to(torch.int32) & 0xFFFF
                    return v >> 6 if kind[2] == "p010" else v
                self.state[..., 0] = values(init.y[0, :H, :W]) * 256
                self.state[..., 1] = 1
                self.state_c[..., :2] = values(init.uv[0, :ch, :2 * cw]).reshape(ch, cw, 2) * 256
                self.state_c[..., 2] = 1
        self.every = torch.ones(256, dtype=torch.uint8, device=device) if style.plate_margin > 0 else None     # ops.grow_labels' table: every label grows

    def observe(self, labels, l_off, nf, pieces):
        """The window's frames teach the plate, on the current stream: labels[l_off:l_off + nf] is the window's label map, `pieces` its
        frames as (frames [k, 3, h0, w0] or a YuvFrames of k surfaces, offset in the window) in video order."""
        from . import ops
        if not nf:
            return
        block = labels[l_off:l_off + nf]
        if self.every is not None:
            if self.scratch is None or self.scratch.shape[0] < nf:       # (one window of labels; windows have a bounded length)
                self.scratch = torch.empty((nf,) + tuple(block.shape[1:]), dtype=torch.uint8, device=self.device)
            block = ops.grow_labels(block, self.every, self.style.plate_margin, self.scratch[:nf])
        for t, d in pieces:
            if self.kind is None:
                ops.plate_update(self.state, t, block[d:d + len(t)], self.style.plate_frames)
            else:
                ops.plate_update_yuv(self.state, self.state_c, t, block[d:d + len(t)], self.style.plate_frames)

    def picture(self):
        """The plate's picture in `back`, on the current stream: uint8 [Ho, Wo, 3], or a YuvFrames of one surface -- what
        ops.render_replace / ops.render_replace_yuv take as their backdrop picture."""
        from . import ops
        if self.kind is None:
            return ops.plate_picture(self.state, self.fill, self.style.plate_reach, self.back)
        return ops.plate_picture_yuv(self.state, self.state_c, self.fill, self.back, self.style.plate_reach)


def plate_of(forms, style, out_size, device, picture):
    """The Plate of a video with `forms` and overlay style `style`, or None where the style does not ask for it.  picture: the buffer
    the overlay is painted into -- a YuvFrames says the kind of the session's surfaces."""
    if not forms.overlay or style is None or not style.plate:
        return None
    return Plate(style, out_size, device, None if torch.is_tensor(picture) else picture.meta())


def path_result(rows, n_frames, windows):
    """{"pred_centroids": int32 [n_out, L, 2], "pred_moments": int64 [n_out, L, 3]}: per output j the path of tracker row rows[j] from
    the windows' tables (`windows`: (f_off, frames, rows the window holds, centroids [n, F, 2], moments [n, F, 3]) on the host); the
    frames before a row's first window are absent, (-1, -1) with moments 0 (`stitch`'s rule)."""
    L = int(n_frames)
    out = {}
    for key, at, fill, dtype in (("pred_centroids", 3, -1, torch.int32), ("pred_moments", 4, 0, torch.int64)):
        wins = [(w[0], w[1], w[2], w[at]) for w in windows]
        parts = stitch(list(rows), L, wins, lambda k, width=at - 1, v=fill, dt=dtype: torch.full((k, width), v, dtype=dt), torch.cat)
        out[key] = torch.stack(parts) if parts else torch.zeros((0, L, at - 1), dtype=dtype)
    return out


def surface_kind(source, out_size):
    """What a surface overlay paints on: the kind (YuvFrames.meta()) of the surfaces `source` (a FrameStore) holds, which must be of the
    output size (None: not looked at) -- the painting kernel does not resample.  Raises the two refusals of the form."""
    if source is None or source.surface is None:
        raise ValueError("surface overlay: the video's frames are RGB tensors; it paints onto decoder surfaces -- hand the video in as a "
                         "preprocess.YuvFrames, or ask for the RGB picture (overlay_output = True, online: surface=False)")
    h, w, fmt, matrix, full_range, order = source.surface
    if out_size is not None and (h, w) != (int(out_size[0]), int(out_size[1])):
        raise ValueError("surface overlay: the output size (height, width) = %s is not the surfaces' %s, and surfaces are painted at their "
                         "own size; ask for height=%d, width=%d (to run the model below that size, hand in full-size surfaces and set "
                         "model.resize_on_device)" % ((int(out_size[0]), int(out_size[1])), (h, w), h, w))
    return source.surface


def surface_picture(source, n, out_size, device, pitch_align=1, pin_memory=False):
    """The buffer of a surface overlay: n fresh surfaces of `surface_kind(source, out_size)`."""
    from .preprocess import YuvFrames
    h, w, fmt, matrix, full_range, order = surface_kind(source, out_size)
    return YuvFrames.empty(n, h, w, fmt=fmt, device=device, pitch_align=pitch_align, pin_memory=pin_memory, matrix=matrix,
                           full_range=full_range, order=order)


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


def polygon_rings(labels, l_off, n, nf, out_size, spec, cls, f0):
    """The outline polygons of a window's n rows from its label map labels[l_off:l_off + nf], on the host -> polygons.TrackPolygons with
    f in video frames (the window starts at f0) and k the window's row; the only caller of ops.label_polygons.  `spec`
    (polygons.Polygons): its min_area goes to the kernel; `every` and `classes` (by the window's class rows `cls`, on the host)
    filter the ring records here and xy is compacted.  Like `rle_positions` the size depends on the data: the default caps, one host
    sync on the true totals, one more call with them as caps where they overflow, then exactly `totals` rows to pinned host memory
    behind a second sync."""
    from . import ops
    from .polygons import TrackPolygons, select_rings
    size = (int(out_size[0]), int(out_size[1]))
    if not n or not nf:
        return TrackPolygons(torch.zeros((0, 2), dtype=torch.int32).numpy(), torch.zeros((0, 5), dtype=torch.int32).numpy(), size)
    lab = labels[l_off:l_off + nf]
    xy, rings, totals = ops.label_polygons(lab, n, spec.min_area)
    V, R = (int(v) for v in totals.tolist())                       # the one sync the data's size takes
    if V > xy.shape[0] or R > rings.shape[0]:
        xy, rings, totals = ops.label_polygons(lab, n, spec.min_area, max(V, 1), max(R, 1))
    host = (torch.empty((V, 2), dtype=torch.int32, pin_memory=bool(V)), torch.empty((R, 5), dtype=torch.int32, pin_memory=bool(R)))
    if V:
        host[0].copy_(xy[:V], non_blocking=True)
        host[1].copy_(rings[:R], non_blocking=True)
        torch.cuda.current_stream(lab.device).synchronize()
    hx, hr = host[0].numpy(), host[1].numpy().copy()
    hx, hr = select_rings(hx, hr, spec.keep(hr, f0, cls, n))
    hr[:, 1] += int(f0)
    return TrackPolygons(hx, hr, size)


def polygon_result(rows, out_size, parts):
    """{"pred_polygons": polygons.TrackPolygons} of a whole video from its windows' (`parts`, in video order; k = tracker row): k becomes
    the output j with rows[j] == k -- the FIRST such j where a track stands behind several outputs -- and the rings of a track that
    misses the selection are dropped, as rle.labels_keep drops its label."""
    from .polygons import TrackPolygons
    table = {}
    for j, r in enumerate(rows):
        table.setdefault(int(r), j)
    return {"pred_polygons": TrackPolygons.concat([p.renumbered(table) for p in parts], size=out_size)}


def matte_planes(m, stride, frame_hw, out_size, spec, cls, out, f_off):
    """The matte output of window logits m [n, F, Hm, Wm] into out[f_off:f_off + F] (uint8 [>= f_off + F, Ho, Wo], device): the union
    matte of ALL n rows, or with spec.classes (render.Matte) of the rows those classes select by the window's class rows `cls`; n = 0:
    zeros (ops.final_matte)."""
    from . import ops
    (fh, fw), (Ho, Wo) = frame_hw, out_size
    idx = torch.arange(int(m.shape[0]), dtype=torch.int32, device=m.device)
    take = spec.takes(cls)
    ops.final_matte(m, idx, stride, fh, fw, Ho, Wo, out, f_off, None if take is None else take.to(m.device), spec.gain)


def occlusion_counts(m, stride, frame_hw, out_size, out=None):
    """The occlusion table of window logits m [n, F, Hm, Wm] on the device: int32 [n, F, n] over ALL n rows (idx = arange(n), as
    `label_maps` does, so column j is the track whose label is j + 1 and every path agrees bit for bit): occ[k, f, j] = the pixels of
    k's final mask that j owns (ops.final_occlusion: one more sweep of the logits; no label map is made or needed).  n = 0: an empty
    table, nothing launched.  out: the buffer to write into."""
    from . import ops
    (fh, fw), (Ho, Wo) = frame_hw, out_size
    idx = torch.arange(int(m.shape[0]), dtype=torch.int32, device=m.device)
    return ops.final_occlusion(m, idx, stride, fh, fw, Ho, Wo, out)


def occlusion_result(rows, n_frames, windows):
    """{"pred_occlusion": int32 [n_out, L, n_out + 1]} of a whole video from its windows' tables, on the host (`windows`: (f_off, frames,
    rows the window holds, table [n, F, n]) in video order): row a is tracker row rows[a], column b < n_out the pixels of a's mask that
    tracker row rows[b] owns (0 where the window does not hold that row), the last column those owned by tracks that are not among
    `rows`.  The frames before a row's first window are zero (`stitch`'s rule)."""
    rows, L = [int(r) for r in rows], int(n_frames)
    width = len(rows) + 1
    wins = []
    for f_off, nf, n, table in windows:
        t = torch.as_tensor(table).to(torch.int64).reshape(int(n), int(nf), int(n))
        piece = torch.zeros((int(n), int(nf), width), dtype=torch.int64)
        for b, r in enumerate(rows):
            if r < n:
                piece[:, :, b] = t[:, :, r]
        inside = sorted({r for r in rows if r < n})
        piece[:, :, -1] = t.sum(-1) - t[:, :, inside].sum(-1)
        wins.append((f_off, nf, n, piece.to(torch.int32)))
    parts = stitch(rows, L, wins, lambda k: torch.zeros((k, width), dtype=torch.int32), torch.cat)
    return {"pred_occlusion": torch.stack(parts) if parts else torch.zeros((0, L, 1), dtype=torch.int32)}


def build_window(m, forms, rows, stride, frame_hw, out_size, planes=None, labels=None, picture=None, paint=None,
                 hop=lambda stage, geom: geom, crops=None, paths=None, matte=None, polygons=None, plate=None, occlusion=None):
    """What `forms` asks for of ONE flushed window (logits m [n, F, Hm, Wm]), on the current stream, for every path; the only caller
    of `overlay_frames`, `label_maps`, `dense_masks` and `rle_positions`.  First the label map of ALL n rows into labels = (device
    buffer, frame offset) and, with picture = (buffer, offset), its overlay, painted from paint = (FrameStore, first video frame,
    render.Style, the window's class rows [n, K] on the host -- what a mosaic of classes is chosen by).  Then the planes of `rows`
    (int32 device; None or empty: none): dense into planes = (buffer, offset) when given, else, with forms.planes == "rle", their run boundaries on the host.  `hop(stage, geom) -> geom` runs behind each stage ("labels" |
    "crops" | "planes") that filled device buffers: the early and the online path send them to the host there, the map under the planes' kernel.
    crops = (render.Crops, FrameStore, first video frame, chips buffer, rects buffer, chip offset): behind the labels stage the window's
    chips (`crop_frames`) from the map and its table, which are then made whether or not `forms` returns them.
    paths (a PathTable, `begin` called for this window): behind the label map the window's centroids (`PathTable.run`), which the
    overlay's trail pass draws and, with forms.paths, the stage "paths" sends on; the map is then made whether or not it is returned.
    matte = (render.Matte, the window's class rows on the host, buffer, offset): the window's matte (`matte_planes`), stage "matte".
    polygons = (polygons.Polygons, the window's class rows on the host, first video frame): behind the labels stage the outlines of
    the map's visible regions (`polygon_rings`: they come to the host there), stage "polygons"; the map is then made whether or not it is
    returned.
    plate (a Plate): the video's background plate, which an overlay in a style with backdrop="plate" teaches and composites.
    occlusion (int32 device buffer [n, F, n]): the window's occlusion table over ALL n rows (`occlusion_counts`), stage "occlusion",
    behind "matte"; it needs no label map.
    -> (labels' geometry table [n, F, 5] or None, planes' table [len(rows), F, 5] or None, (pos, n_pos) of `rle_positions` or None,
    the window's TrackPolygons or None)."""
    lgeom = pgeom = runs = poly = None
    if labels is not None:
        table = forms.label_geometry or crops is not None
        if picture is not None:
            dgeom = overlay_frames(m, stride, frame_hw, out_size, table, *labels, *paint, *picture, paths=paths,
                                   **({"plate": plate} if plate is not None else {}))
        else:
            dgeom = label_maps(m, stride, frame_hw, out_size, table, *labels)
            if paths is not None:
                paths.run(*labels)
        lgeom = hop("labels", dgeom if forms.label_geometry else None)
        if paths is not None and forms.paths:
            hop("paths", None)
        if crops is not None:
            spec, source, f0, chips, rects, c_off = crops
            crop_frames(int(m.shape[0]), int(m.shape[1]), *labels, dgeom, source, f0, spec, chips, rects, c_off)
            hop("crops", None)
        if polygons is not None:
            poly = polygon_rings(*labels, int(m.shape[0]), int(m.shape[1]), out_size, *polygons)
            hop("polygons", None)
    if matte is not None:
        matte_planes(m, stride, frame_hw, out_size, *matte)
        hop("matte", None)
    if occlusion is not None:
        occlusion_counts(m, stride, frame_hw, out_size, occlusion)
        hop("occlusion", None)
    if rows is not None and int(rows.numel()):
        if planes is not None:
            pgeom = hop("planes", dense_masks(m, rows, stride, frame_hw, out_size, forms.plane_geometry, *planes))
        elif forms.planes == "rle":
            *runs, pgeom = rle_positions(m, rows, stride, frame_hw, out_size, forms.plane_geometry)
    return lgeom, pgeom, runs, poly


def copy_stream(model):
    """The model's copy stream, created at the first call (the order streams are first used in decides their queues: `MDQE._make_streams`)."""
    if model._copy_stream is None:
        model._copy_stream = torch.cuda.Stream(model.device)
    return model._copy_stream


def to_host(cs, side, copies, geom, event):
    """A window's device buffers (produced on stream `side`) to pinned host memory on the copy stream `cs`: `copies` = (pinned
    destination, device source) pairs; every source is `record_stream`ed there (sources that are views of one buffer: once).  The
    geometry table (or None) rides on the same stream; `event` is recorded behind both.  -> the table in pinned memory (valid once
    `event` has fired), or None."""
    hgeom = None if geom is None else torch.empty(geom.shape, dtype=torch.int32, pin_memory=True)
    cs.wait_stream(side)
    with torch.cuda.stream(cs):
        for dst, src in copies:
            dst.copy_(src, non_blocking=True)
        for src in {src.untyped_storage().data_ptr(): src for _, src in copies}.values():
            src.record_stream(cs)
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


def track_geometry(rows, n_frames, out_size, windows, labels=False):
    """Per output j the [n_frames] geometry of row rows[j] from the windows' geom tables: `windows` = (f_off, nf, n rows this window
    holds, geom int32 [n, nf, 5] on the host).  -> {"pred_boxes": [float32 [n_frames, 4]], "pred_areas": [int64 [n_frames]]}; labels:
    the tables are those of the labels' visible regions, the keys "pred_label_boxes" / "pred_label_areas"."""
    Ho, Wo = int(out_size[0]), int(out_size[1])
    none = torch.tensor([[0, Wo, Ho, -1, -1]], dtype=torch.int32)
    wins = [(f, nf, n, torch.as_tensor(g)) for f, nf, n, g in windows]
    geo = [R.geom_to_boxes(t) for t in stitch(rows, int(n_frames), wins, lambda k: none.repeat(k, 1), torch.cat)]   # (fresh tensors per output)
    pre = "pred_label_" if labels else "pred_"
    return {pre + "boxes": [b for b, _ in geo], pre + "areas": [a for _, a in geo]}


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
    matte: object = None                                              # matte: ONE pinned uint8 [L, Ho, Wo] per video (model.matte_output)
    polygons: list = dataclasses.field(default_factory=list)          # per window, its TrackPolygons (k = tracker row; model.polygon_output)
    occlusion: list = dataclasses.field(default_factory=list)         # per window (f_off, frames, tracks, int32 [tracks, frames, tracks] pinned host; model.occlusion_output)


def result_head(model, cls_clips, out_size, n_frames, score=None, track_ids=True):
    """The head of a video's result, offline and online: the video-level top-k (`select_tracks`), "pred_track_ids" (the tracker row
    behind output j; `track_ids`, and always beside a score) and, with `score` (OverlapTables), "pred_gt".  -> (res, those rows)."""
    sc, labels, inst = model.select_tracks(cls_clips)
    res = {"image_size": (int(out_size[0]), int(out_size[1])), "pred_scores": sc.tolist(), "pred_labels": labels}
    if track_ids:
        res["pred_track_ids"] = list(inst)
    if score is not None:                                          # (the counts of every window are in; select rows, read back)
        res["pred_gt"] = score.result(list(inst), n_frames, model._copy_stream)
        res.setdefault("pred_track_ids", list(inst))
    return res, list(inst)


def video_result(model, image_size, cls_clips, windows, frame_hw, n_frames, early=None, emit_masks=True, frame_source=None, score=None,
                 forms=None, crops=None, paths=None):
    """mdqe/mdqe.py:430-471.  The x4 aligned-bilinear up-sampling, sigmoid, crop (:357-358), nearest resize to the original size and
    the 0.5 threshold (:458-462) run as ONE kernel per window; windows in which an instance did not exist yet stay zero (:442).
    `forms`: the merger's record (ClipMerger.finish); None: resolved from the model here.  `early` (EarlyMasks): every form is on the
    host already, only the selection is left.  Without it (`windows`: (f_off, mean logits) per flushed window) the forms are built here
    (`build_window`; planes: the selected tracks only) into whole-video device buffers, one copy at the end; model.rle_output: the
    planes are then encoded on the host.  `score` (OverlapTables): the counts gathered at every flush on any path -> "pred_gt".
    "pred_label_map": uint8 [L, Ho, Wo], host; label t + 1 = tracker row t, 0 = background, so pred_label_map == pred_track_ids[j] + 1
    is output j's exclusive region.  "pred_overlay": uint8 [L, Ho, Wo, 3], pinned host; with forms.surface a YuvFrames of
    L painted surfaces (pinned host, tight pitch).  `crops` (CropTable): the early path's table, filled at every flush; without it and
    with forms.crops the table is filled here, window by window -> "pred_crops", "pred_crop_rects", "pred_crop_frames".  `paths`
    (PathTable): the early path's table with every window's centroids kept; without it and with forms.paths, or with a style that
    draws trails, the table is made and filled here -> "pred_centroids" int32 [n_out, L, 2], "pred_moments" int64 [n_out, L, 3]."""
    if forms is None:
        forms = Forms.of_model(model, emit_masks)
        forms = dataclasses.replace(forms, overlay=forms.overlay and frame_source is not None, crops=forms.crops and frame_source is not None)
    out_size = Ho, Wo = int(image_size[0]), int(image_size[1])
    res, inst = result_head(model, cls_clips, out_size, n_frames, score, track_ids=False)
    rows, host, planes_res = inst, {}, {"pred_masks": []}          # ([]: no per-track planes in either form)
    if forms == Forms():                                           # (emit_masks=False: nothing to build, nothing to wait for)
        return dict(res, **planes_res)
    if early is not None:
        early.done.synchronize()                                   # (the geom tables ride on the copies' stream)
        plane_geoms, label_geoms = early.geom, early.label_geom
        if forms.planes == "rle":
            planes_res = {"pred_rles": stitch_rles(inst, n_frames, out_size, [(f, nf, n, R.positions_to_rles(pos, n_pos, out_size, nf))
                                                                              for f, nf, n, pos, n_pos in early.rle])}
        elif forms.planes:
            planes_res = {"pred_masks": [early.hosts[i].view(torch.bool)[:n_frames] for i in inst]}
        host = {"labels": early.labels, "overlay": early.overlay, "matte": early.matte}
        polys, occs = early.polygons, early.occlusion
    else:
        sel = sorted(set(inst))
        rows = [sel.index(i) for i in inst]                        # rows of the planes' buffer = positions in sel
        plane_geoms, label_geoms, polys, occs, u8 = [], [], [], [], dict(dtype=torch.uint8, device=model.device)
        # (the windows tile [0, n_frames): every row of the map and the picture is written; a track's planes start at its first window)
        d_lab = torch.empty(n_frames, Ho, Wo, **u8) if forms.labels or forms.overlay or forms.crops or forms.paths or forms.polygons else None
        if forms.crops:
            crops = CropTable(model.crop_output, n_frames, model.device)
        paths = path_table(forms, model.overlay_style if forms.overlay else None, model.device, keep=forms.paths)
        d_pic = torch.empty(n_frames, Ho, Wo, 3, **u8) if forms.overlay and not forms.surface else None
        if forms.surface:
            d_pic = surface_picture(frame_source, n_frames, out_size, model.device)
        plate = plate_of(forms, model.overlay_style if forms.overlay else None, out_size, model.device, d_pic)
        d_planes = torch.zeros(len(sel), n_frames, Ho, Wo, **u8) if forms.planes else None
        d_mat = torch.empty(n_frames, Ho, Wo, **u8) if forms.matte else None
        sel_dev = torch.tensor(sel, dtype=torch.int32, device=model.device) if forms.planes else None
        for i, (f_off, m) in enumerate(windows):
            n, nf = int(m.shape[0]), int(m.shape[1])
            cnt = sum(1 for i in sel if i < n)                     # sel is ascending: these are its first `cnt` entries
            at = [None if t is None else (t, f_off) for t in (d_planes, d_lab, d_pic)]
            if paths is not None:
                paths.begin(n, nf)
            occ = torch.empty((n, nf, n), dtype=torch.int32, device=model.device) if forms.occlusion else None
            lg, pg, _, poly = build_window(m, forms, sel_dev[:cnt] if forms.planes else None, model.cfg.match_stride, frame_hw, out_size, *at,
                                     paint=(frame_source, f_off, model.overlay_style, cls_clips[i]) if forms.overlay else None,
                                     crops=(crops.spec, frame_source, f_off, *crops.rows(n), crops.spec.count(f_off)) if forms.crops else None,
                                     paths=paths, matte=(model.matte_output, cls_clips[i], d_mat, f_off) if forms.matte else None,
                                     **({"plate": plate} if plate is not None else {}),
                                     **({"polygons": (model.polygon_output, cls_clips[i], f_off)} if forms.polygons else {}),
                                     **({"occlusion": occ} if occ is not None else {}))
            if occ is not None:
                occs.append((f_off, nf, n, occ))
            if forms.polygons:
                polys.append(poly)
            if paths is not None:
                paths.keep(f_off)
            label_geoms.append((f_off, nf, n, lg))
            if cnt:
                plane_geoms.append((f_off, nf, cnt, pg))
        # one D2H each into pinned memory (pageable copies run at a fraction of PCIe), one sync behind them
        for k, t in (("overlay", d_pic), ("labels", d_lab if forms.labels else None), ("planes", d_planes), ("matte", d_mat)):
            if t is not None and not torch.is_tensor(t):           # a surface picture: both planes
                host[k] = surface_picture(frame_source, n_frames, out_size, "cpu", pin_memory=True)
                host[k].y.copy_(t.y, non_blocking=True)
                host[k].uv.copy_(t.uv, non_blocking=True)
            elif t is not None:
                host[k] = torch.empty(t.shape, dtype=torch.uint8, pin_memory=True)
                host[k].copy_(t, non_blocking=True)
        torch.cuda.current_stream(model.device).synchronize()
        # (the tables' copies follow the buffers' sync)
        plane_geoms, label_geoms = ([(f, nf, n, g.cpu() if on else g) for f, nf, n, g in gs]
                                    for on, gs in ((forms.plane_geometry, plane_geoms), (forms.label_geometry, label_geoms)))
        occs = [(f, nf, n, t.cpu()) for f, nf, n, t in occs]
        if forms.planes:
            planes = host["planes"].view(torch.bool)
            if forms.planes == "rle":                              # no early path (unknown length): encode on the host
                enc = [[R.encode_dense(fm.numpy()) for fm in planes[p]] for p in range(len(sel))]
                planes_res = {"pred_rles": [enc[p] for p in rows]}
            else:
                planes_res = {"pred_masks": [planes[p] for p in rows]}
    if forms.labels or forms.overlay or forms.crops or forms.paths or forms.matte or forms.polygons or forms.occlusion:
        res.setdefault("pred_track_ids", list(inst))
    if forms.matte:
        res["pred_matte"] = host["matte"][:n_frames]
    if forms.occlusion:
        res.update(occlusion_result(inst, n_frames, occs))
    if forms.crops:
        res.update(crops.result(inst))
    if forms.paths:
        res.update(paths.result(inst, n_frames))
    if forms.polygons:
        res.update(polygon_result(inst, out_size, polys))
    if forms.labels:
        res["pred_label_map"] = host["labels"][:n_frames]
    if forms.overlay:
        res["pred_overlay"] = host["overlay"][:n_frames]
    if forms.label_geometry:
        res.update(track_geometry(inst, n_frames, out_size, label_geoms, labels=True))
    res.update(planes_res)
    if forms.plane_geometry:
        res.update(track_geometry(rows, n_frames, out_size, plane_geoms))
    return res


class ClipMerger:
    """Incremental form of the clip loop's second half (mdqe/mdqe.py:337-366): tracker update per clip, window flushes,
    final video merge.  The tracker runs on its own HIP stream so that its small kernels and per-clip host syncs overlap
    with per-frame work the producer has already queued on the main stream."""

    tracker_cls = OverTracker               # (tests without a GPU substitute a stand-in bank, tests/_standins.py)
    EARLY_TRACKS = 48                       # tracks per video the early-mask path budgets pinned memory for

    def __init__(self, model, frame_hw, out_size, mask_hw, n_frames=None, emit_masks=True, online=None, geometry=None, frame_source=None,
                 style=None, ground_truth=None, surface=False, surface_pitch_align=1, crops=None, paths=False, matte=None, polygons=None,
                 occlusion=False):
        self.model, self.frame_hw, self.out_size, self.mask_hw = model, frame_hw, out_size, mask_hw
        self.emit_masks = emit_masks                # False: scores / labels only (ranks > 0 of a sharded video)
        # online ("masks" | "rle" | "labels" | "overlay"; online.OnlineVideo, CUDA only): at each flush the window's final masks -- or their
        # RLE, or their label map, or that map and its overlay -- of every current track are built and appended to `emitted`; neither the
        # logits nor a host buffer stay here (n_frames is unknown)
        self.online = online
        # the forms of this video, for every path (geometry None: model.geometry_output; online sessions pass theirs)
        # (surface, surface_pitch_align: an online session's; offline the model's overlay_output == "surface", at a tight pitch)
        # crops (render.Crops): an online session's; offline the model's crop_output
        self.crop_spec = crops if online else (getattr(model, "crop_output", None) if emit_masks else None)
        # paths: an online session's; offline the model's path_output
        # matte (render.Matte): an online session's; offline the model's matte_output
        self.matte_spec = matte if online else (getattr(model, "matte_output", None) if emit_masks else None)
        # polygons (polygons.Polygons): an online session's; offline the model's polygon_output
        self.polygon_spec = polygons if online else (getattr(model, "polygon_output", None) if emit_masks else None)
        self.forms = forms = (Forms.of_emit(online, geometry, model, surface, self.crop_spec is not None, bool(paths), matte is not None,
                                            self.polygon_spec is not None, occlusion=bool(occlusion)) if online
                              else Forms.of_model(model, emit_masks, geometry))
        self.crop_table = None                      # the early path's CropTable, from its first window
        self.path_table = None                      # the early and the online path's PathTable, from their first window
        self.plate = None                           # the early and the online path's Plate (a style with backdrop="plate"), from their first window
        self.surface_pitch_align = surface_pitch_align
        self.geometry = forms.plane_geometry or forms.label_geometry
        # False | True | "only" (model.label_output): the label map next to -- or, "only", instead of -- the per-track planes
        self.labels = False if online else forms.labels and ("only" if forms.planes is None else True)
        # what an overlay paints on: the frames of `frame_source` (a FrameStore), in `style`
        self.frame_source = frame_source
        self.style = style if style is not None else getattr(model, "overlay_style", None)
        if forms.crops and frame_source is None:
            raise ValueError("crop output needs the frames of the whole video on this device; this path does not hold them (the sharded "
                             "driver does not offer it: rank 0 does not hold every frame)")
        if forms.overlay and frame_source is None:
            raise ValueError("overlay output needs the frames of the whole video on this device; this path does not hold them (the sharded "
                             "driver does not offer it: rank 0 does not hold every frame)")
        if forms.overlay and self.style is not None and self.style.replace is not None:
            check_replace(self.style, out_size, forms.surface)
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
            if per_track * (self.EARLY_TRACKS + (3 if forms.overlay else 0)) > float(os.environ.get("MDQE_EARLY_PINNED_GB", "24")) * 2 ** 30:
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
                if self.online:
                    self.emitted.append(self._online_window(c, m))
                elif self.emit_masks and self.use_side and self.n_frames is not None and (self.early_on or self.forms.early_always):
                    self._early_masks(m, c)
                elif self.emit_masks:
                    self.windows.append((self.f_off, m))
                self.f_off += m.shape[1]
                self.saved += 1
        self.done = self.done or bool(last)

    def _window_to_host(self, m, pairs, event, c=None):
        """The early and the online path: the forms of ALL n rows of the window just flushed (m: [n, F, Hm, Wm] mean logits) into
        per-window device scratch (`build_window`), each stage sent to the host behind it (`to_host`): pairs(kind, buffer) -> its (pinned
        destination, source) pairs, kind = "labels" | "overlay" | "planes"; `event()` is recorded behind each hop; c: the window's class rows on the host (an
        overlay's mosaic of classes).  The video's PathTable (`path_table`: for paths or a style with a trail) is made at the first
        window and announced each window (`PathTable.begin`); online its window's centroids and moments are the stage "paths".
        -> build_window's."""
        forms, u8 = self.forms, dict(dtype=torch.uint8, device=self.dev)
        n, nf, Ho, Wo = int(m.shape[0]), int(m.shape[1]), int(self.out_size[0]), int(self.out_size[1])
        lab = torch.empty(nf, Ho, Wo, **u8) if forms.labels or forms.overlay or forms.crops or forms.paths or forms.polygons else None    # (an overlay, crops, paths or polygons alone: a scratch, not copied)
        pic = torch.empty(nf, Ho, Wo, 3, **u8) if forms.overlay and not forms.surface else None
        if forms.surface:                           # (the host's pitch: the window copy is then two plain copies, padding and all)
            pic = surface_picture(self.frame_source, nf, self.out_size, self.dev, self.surface_pitch_align)
        rows = torch.arange(n, dtype=torch.int32, device=self.dev) if n and forms.planes else None
        planes = torch.empty(n, nf, Ho, Wo, **u8) if rows is not None and forms.planes == "dense" else None
        mat = torch.empty(nf, Ho, Wo, **u8) if forms.matte else None
        copies = {"labels": (pairs("labels", lab) if forms.labels else []) + (pairs("overlay", pic) if forms.overlay else []),
                  "planes": pairs("planes", planes) if planes is not None else [], "crops": [], "paths": [], "polygons": [],
                  "matte": pairs("matte", mat) if mat is not None else [], "occlusion": []}
        occ = None
        if forms.occlusion:                         # the window's table [n, F, n], sent to the host (offline: selected and stitched at the end)
            occ = torch.empty((n, nf, n), dtype=torch.int32, device=self.dev)
            copies["occlusion"] = pairs("occlusion", occ)
        crop = None
        if forms.crops:
            spec = self.crop_spec
            if self.online:                         # the window's own chips: [n, frames taken, Sh, Sw, 3] and their rects, sent to the host
                fc = len(spec.taken(self.f_off, self.f_off + nf))
                chips = torch.empty((n, fc) + spec.size + (3,), **u8)
                rects = torch.empty((n, fc, 4), dtype=torch.int32, device=self.dev)
                copies["crops"] = pairs("crops", chips) + pairs("crop_rects", rects)
                crop = (spec, self.frame_source, self.f_off, chips, rects, 0)
            else:                                   # the video's table on the device: read back once, at the end
                if self.crop_table is None:
                    self.crop_table = CropTable(spec, self.n_frames, self.dev)
                crop = (spec, self.frame_source, self.f_off, *self.crop_table.rows(n), spec.count(self.f_off))
        # (the copy stream is created BEFORE the window's kernels are launched, and only by a window that copies, as ever: the order
        # streams are first used in decides their queues)
        sends_paths = bool(forms.paths and self.online and n)        # (offline the windows' tables wait on the device: PathTable.keep)
        cs = copy_stream(self.model) if copies["labels"] or copies["planes"] or copies["crops"] or copies["matte"] or copies["occlusion"] or sends_paths else None
        if self.path_table is None:
            self.path_table = path_table(forms, self.style, self.dev, keep=forms.paths and not self.online)
        if self.plate is None:
            self.plate = plate_of(forms, self.style, self.out_size, self.dev, pic)
        if self.path_table is not None:
            views = self.path_table.begin(n, nf)
            if forms.paths and self.online:
                copies["paths"] = pairs("centroids", views[0]) + pairs("moments", views[1])
        at = [None if t is None else (t, 0) for t in (planes, lab, pic)]
        out = build_window(m, forms, rows, self.model.cfg.match_stride, self.frame_hw, self.out_size, *at,
                           paint=(self.frame_source, self.f_off, self.style, c), crops=crop, paths=self.path_table,
                           matte=(self.matte_spec, c, mat, 0) if mat is not None else None,
                           **({"plate": self.plate} if self.plate is not None else {}),
                           **({"polygons": (self.polygon_spec, c, self.f_off)} if forms.polygons else {}),
                           **({"occlusion": occ} if occ is not None else {}),
                           hop=lambda stage, geom: (to_host(cs, self.side, copies[stage], geom, event())
                                                    if copies[stage] or geom is not None else None))   # (a scratch stage: nothing to send)
        if self.path_table is not None:
            self.path_table.keep(self.f_off)
        return out

    def _early_masks(self, m, c=None):
        """Every form of EVERY instance tracked so far goes to pinned host memory while later windows compute; finish() then only
        selects rows.  A few rows may be produced in vain (instances that miss the final top-k).  Planes: one pinned [L, Ho, Wo] buffer
        per track (no re-allocation as tracks appear; the caching host allocator recycles the blocks of the previous call), or the run
        boundaries.  Label map, overlay: one pinned [L, Ho, Wo(, 3)] buffer per video; a window without tracks is written too."""
        model, forms = self.model, self.forms
        n, nf, f0 = int(m.shape[0]), int(m.shape[1]), self.f_off
        shape = (int(self.n_frames), int(self.out_size[0]), int(self.out_size[1]))
        copy_stream(model)                          # (created here also when nothing is copied: the order of first use decides the queues)
        if self.early is None:
            self.early = EarlyMasks(done=torch.cuda.Event())
        early = self.early

        def pairs(kind, buf):
            if kind == "occlusion":                 # the window's own table: its shape changes with the tracks
                early.occlusion.append((f0, nf, n, torch.empty(tuple(buf.shape), dtype=buf.dtype, pin_memory=bool(buf.numel()))))
                return [(early.occlusion[-1][3], buf)] if buf.numel() else []
            if kind == "planes":
                while len(early.hosts) < n:         # a new track: its own pinned buffer, zero before its first window (:442)
                    early.hosts.append(model.pinned_mask_buffer(shape))
                    if f0 > 0:
                        early.hosts[-1][:f0].zero_()
                return [(h[f0:f0 + nf], d) for h, d in zip(early.hosts, buf)]
            if not torch.is_tensor(buf):            # a surface picture: ONE pinned YuvFrames of L surfaces per video, both planes
                if early.overlay is None:
                    early.overlay = surface_picture(self.frame_source, shape[0], self.out_size, "cpu", pin_memory=True)
                return [(early.overlay.y[f0:f0 + nf], buf.y), (early.overlay.uv[f0:f0 + nf], buf.uv)]
            if getattr(early, kind) is None:
                setattr(early, kind, model.pinned_mask_buffer(shape + (3,) * (kind == "overlay")))
            return [(getattr(early, kind)[f0:f0 + nf], buf)]
        lgeom, pgeom, runs, poly = self._window_to_host(m, pairs, lambda: early.done, c)
        if forms.polygons:
            early.polygons.append(poly)
        if forms.label_geometry:
            early.label_geom.append((f0, nf, n, lgeom))
        if runs is not None:
            early.rle.append((f0, nf, n, *runs))
        if n and forms.plane_geometry:
            early.geom.append((f0, nf, n, pgeom))

    def _online_window(self, c, m):
        """Online mode: the window just flushed (c: class rows [n, K] on the host) as a record -- frames, class rows, and the final masks
        of tracks 0..n-1: "masks" in a pinned host buffer (`ready` fires when they and the geometry table "geom" are there), or their
        "rles", or their label map "labels" uint8 [F, Ho, Wo], copied the same way, with the geometry of the labels' visible regions,
        or that map and its "overlay" uint8 [F, Ho, Wo, 3] (a window without tracks: all background, the picture is the frames)."""
        forms, n, nf, out_size = self.forms, int(m.shape[0]), int(m.shape[1]), (int(self.out_size[0]), int(self.out_size[1]))
        rec = {"frames": (self.f_off, self.f_off + nf), "cls_probs": c, "ready": None}
        if forms.planes == "dense":
            rec["masks"] = torch.zeros((0, nf) + out_size, dtype=torch.bool)

        def pairs(kind, buf):                       # fresh pinned buffers, the record's
            if not torch.is_tensor(buf):            # a surface picture: pinned surfaces of the same pitch, both planes
                host = rec["overlay"] = surface_picture(self.frame_source, nf, out_size, "cpu", self.surface_pitch_align, pin_memory=True)
                return [(host.y, buf.y), (host.uv, buf.uv)]
            if kind in ("crops", "crop_rects", "centroids", "moments", "occlusion"):     # (their shape changes with the tracks: not the mask pool's kind of buffer)
                rec[kind] = torch.empty(tuple(buf.shape), dtype=buf.dtype, pin_memory=bool(buf.numel()))
                return [(rec[kind], buf)] if buf.numel() else []
            host = self.model.pinned_mask_buffer(tuple(buf.shape))
            rec.update({"masks": host.view(torch.bool)} if kind == "planes" else {kind: host})
            return [(host, buf)]

        def event():                                # (None stays where nothing is copied: RLE, or a window without tracks)
            rec["ready"] = rec["ready"] or torch.cuda.Event()
            return rec["ready"]
        lgeom, pgeom, runs, poly = self._window_to_host(m, pairs, event, c)
        if forms.polygons:
            rec["polygons"] = poly
        if forms.crops:
            rec["crop_frames"] = self.crop_spec.taken(self.f_off, self.f_off + nf)
        if forms.planes == "rle":
            rec["rles"] = R.positions_to_rles(*runs, out_size, nf) if n else []
        if forms.label_geometry:
            rec["geom"] = lgeom
        elif forms.plane_geometry:                  # (a window without tracks: an empty table)
            rec["geom"] = pgeom if n else torch.zeros((0, nf, 5), dtype=torch.int32)
        return rec

    def feed_batches(self, results, to_the_end=False):
        """Clip results in global order (`iter_clip_results`), fed to the tracker per decoder batch: the clips of one batch go together.
        Stops behind the last clip, or (to_the_end) runs the iterator out.  Returns True once the last clip has been consumed."""
        buf = []
        for item in results:
            buf.append(item)
            if item[3].get("batch_end", True):
                if self.feed_many(buf) and not to_the_end:
                    return True
                buf = []
        return self.feed_many(buf)

    def finish(self):
        if self.use_side:
            self.main.wait_stream(self.side)
            for _, m in self.windows:
                m.record_stream(self.main)
        return self.model.inference_video(self.out_size, self.cls_clips, self.windows, self.frame_hw, self.f_off, early=self.early,
                                          emit_masks=self.emit_masks, frame_source=self.frame_source, score=self.score, forms=self.forms,
                                          **({"crops": self.crop_table} if self.forms.crops else {}),
                                          **({"paths": self.path_table} if self.forms.paths and self.path_table is not None else {}))
