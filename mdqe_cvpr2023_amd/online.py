"""Online video inference: frames arrive in pushes of any size, tracker windows come back as soon as they are final.

    ov = model.online_video(height=H, width=W, emit="masks", keep=False, geometry=False)
    for chunk in source:                   # [n, 3, h, w] uint8 / float32, host or device, n >= 1 (n == 0: no-op),
                                           # or n NV12 / P010 decoder surfaces: preprocess.YuvFrames (converted on the device)
        for win in ov.push(chunk):         # the windows this push completed, in order
            win.frames, win.track_ids, win.cls_probs, win.masks   # (or win.rles with emit="rle", win.labels with emit="labels")
            win.boxes, win.areas           # geometry=True: XYXY_ABS float32 [n, F, 4] and pixel counts int64 [n, F] of those masks
    for win in ov.close():                 # the clamped last clip and the final flush
        ...
    res = ov.result()                      # {"image_size", "pred_scores", "pred_labels", "pred_track_ids"} (+ "pred_masks" / "pred_rles" if keep)

ground_truth=gt (a vis_score.GroundTruth, to `online_video`): every window's final masks are also counted against it on the device and
result() carries "pred_gt", equal to forward()'s with the input's "ground_truth"; a push past its length raises at that push.

Same clips in the same order and the same window flushes as `MDQE.forward` on the whole video (mdqe/mdqe.py:308-366), so with
keep=True the result equals forward()'s bit for bit.  A push runs every clip whose frames are all present (the schedule's last clip,
`end > L`, can only run at close(), when L is known); each frame goes through the per-frame stages once -- a clip that straddles two
pushes reads the carried cache rows of the earlier frames (`_Carry`, at most T-1 frames).  What stays on the device between pushes is
the tracker bank and the carry; the masks of a window leave for the host when it is flushed.  With geometry=True the kernels that
write / encode a window's masks also return each mask's pixel count and tight box (ops.final_masks_geom / final_masks_rle_geom): no pass
over the masks on the host, no decoding of the RLEs; result() then carries "pred_boxes" / "pred_areas" whatever `keep` says.  MERGE_ON_CPU has no meaning here (it
only places the window results the offline merge waits on).  One GPU, one video per session.

emit="labels": a window carries ONE uint8 [F, H, W] map instead of n planes (`win.labels`; win.masks / win.rles are None): per pixel
track_id + 1 of the track that owns it -- the largest up-sampled logit among the window's tracks whose mask holds the pixel -- and 0
for background (ops.final_label_map; 1 byte per pixel however many tracks).  geometry=True then describes the labels' visible regions
(win.boxes / win.areas, result()'s "pred_label_boxes" / "pred_label_areas"); keep=True adds "pred_label_map", equal to forward()'s
with model.label_output.  A label can name a track that misses the video-level top-k: rle.labels_keep(map, result["pred_track_ids"]).

emit="overlay" (style=render.Style(alpha=0.5, contour=1, palette=None)): what emit="labels" gives and, painted from the map on the
device, `win.overlay`: uint8 [F, H, W, 3] on the host, pixel-interleaved, channel order = the frames' -- the frames that were pushed
with every track's region blended towards its colour and a full-colour line where regions meet (ops.render_overlay; 3 bytes per pixel
of read-back however many tracks).  A track's colour depends on its tracker row only, so it is the same in every window.  win.labels
says which colour is which track.  The picture is painted on the frames AS PUSHED: when height / width exceed their size it is a nearest
up-sample of them -- for a sharp picture push original-size uint8 frames and set model.resize_on_device.  The session keeps each push's
frames on the device until the windows they belong to are out: after any push `ov.frames_held <= frames not yet emitted + the largest
push - 1` (whole pushes are dropped), so the store does not grow with the video.  keep=True adds "pred_overlay" [L, H, W, 3] and
"pred_label_map" to result(), equal to forward()'s with model.overlay_output / label_output.

emit="overlay", surface=True (pushes of preprocess.YuvFrames only): the two ends of a streaming pipeline meet -- decoder surfaces in,
PAINTED SURFACES of the same format out, painted in the YUV domain on the device (ops.render_overlay_yuv; the rule is in
include/mdqe_hip.h).  `win.overlay` is a preprocess.YuvFrames on the host (pinned) with f1 - f0 surfaces, carrying the fmt, matrix, range
and order of the first push; its pitch is tight (width / 2*ceil(width/2) samples) unless surface_pitch_align=k rounds it up to a multiple
of k bytes, and padding bytes are zero.  A background pixel keeps the decoder's bits exactly (no YUV -> RGB -> YUV round trip), the
session keeps the pushed surfaces themselves -- 1.5 bytes per pixel for NV12 instead of 3, never the converted RGB frames -- under the
same `frames_held` bound, and reads 1.5 bytes per pixel back.  The output size must be the surfaces' size (nothing is resampled: to run
the model below it, push full-size surfaces and set model.resize_on_device).  win.labels is what it is without `surface`; keep=True
makes result()["pred_overlay"] one YuvFrames of L surfaces, equal to forward()'s with model.overlay_output = "surface".

crops=render.Crops(size=(128, 64), pad=0.0, cutout=False, fill=(0, 0, 0), min_area=0, every=1), beside ANY emit: every window also
carries one fixed-size picture per track and taken frame, cut from the frames AS PUSHED (with model.resize_on_device: the original-size
frames) along the track's visible region of the label map and resized on the device (ops.track_crops; the rule is in
include/mdqe_hip.h): `win.crops` uint8 [n, Fc, Sh, Sw, 3] (pinned host, channel order = the frames'), `win.crop_rects` int32 [n, Fc, 4]
(the source rect (X0, Y0, X1, Y1) in output pixels, inclusive; (0, 0, -1, -1) and a chip of `fill` where the track has no region) and
`win.crop_frames`, the Fc video frames taken -- those with f % every == 0.  The label map and its table are then made for every emit (a
device scratch where the emit does not return them), and the session keeps the pushed frames under the `frames_held` bound above
whatever the emit.  keep=True adds "pred_crops" / "pred_crop_rects" / "pred_crop_frames" to result(), equal to forward()'s with
model.crop_output.

matte=render.Matte(classes=None, gain=1.0), beside ANY emit: every window also carries `win.matte`, uint8 [F, H, W] on pinned host, the
soft matte of its tracks (with `classes`: of the tracks those classes select by the window's class rows) from one more sweep of the
window's logits (ops.final_matte): >= 128 exactly on the union of their masks.  keep=True adds "pred_matte" [L, H, W] to result(),
equal to forward()'s with model.matte_output.
paths=True, beside ANY emit: every window also carries where its tracks are -- `win.centroids` int32 [n, F, 2] (pinned host: (x, y) of
the track's visible region of the label map, ((SX + m/2) / m, (SY + m/2) / m) in integers, (-1, -1) where it has none) and
`win.moments` int64 [n, F, 3] = (m, SX, SY) -- summed on the device from the label map (ops.label_centroids; the map is then made for
every emit).  keep=True adds "pred_centroids" / "pred_moments" to result(), equal to forward()'s with model.path_output.  The trails of
Style(trail=...) are drawn from the same points and need no `paths`; their history is a device table of `trail` columns
(merge.PathTable), so lines continue across windows and pushes and nothing grows with the video.
polygons=Polygons(...) (polygons.py), beside ANY emit: every window also carries `win.polygons`, a polygons.TrackPolygons of the outlines
of its tracks' visible regions of the label map -- rings of lattice corners, traced on the device (ops.label_polygons; the map is then
made for every emit), a few KB per window; f counts video frames, k is the window's row.  keep=True adds "pred_polygons" to result(),
equal to forward()'s with model.polygon_output.
occlusion=True, beside ANY emit (surface=True sessions included): every window also carries `win.occlusion`, int32 [n, F, n] on pinned
host -- occlusion[k, f, j] = the pixels of track k's final mask in frame f that track j owns (j == k: k's visible region; j != k: the
part of k that j hides; the row's sum: the area of k's mask), rows and columns being the window's tracker rows -- counted on the device
in one more sweep of the window's logits (ops.final_occlusion); no label map is made for it, so emit="rle" stays without one.  keep=True
adds "pred_occlusion" int32 [n_out, L, n_out + 1] to result(), equal to forward()'s with model.occlusion_output; helpers: occlusion.py.
"""
import contextlib
import dataclasses

import numpy as np
import torch

from .schedule import cache_budget_frames


# ---- the schedule, as pure functions (tests/test_online_cpu.py drives them without a GPU) --------------------------------------------
def push_clips(next_start, received, T, stride):
    """The clips a push runs once `received` frames are in: every (s, s+T, False) with s = next_start, next_start + stride, ...
    and s + T <= received.  Returns (clips, the start of the next clip)."""
    clips, s = [], int(next_start)
    while s + T <= received:
        clips.append((s, s + T, False))
        s += stride
    return clips, s


def close_clips(n_run, L, T, stride):
    """The clips close() runs: those of the offline schedule (`MDQE.clip_schedule(L, T, stride)`) that no push ran -- at most the
    clamped last one, because a push runs every clip with s + T <= frames received and `last` means s + T > L."""
    from .meta_arch import MDQE
    sched = MDQE.clip_schedule(L, T, stride)
    return sched[n_run:]


def is_flush(start, last, saved, stride, win):
    """ClipMerger.feed_many's rule: the clip at `start` flushes tracker window `saved` (0-based)."""
    return bool(last) or start + stride >= win * (saved + 1)


def carry_from(next_start, received):
    """First frame whose cache rows a later clip reads: the start of the next clip, or nothing (`received`) if it starts later."""
    return min(int(next_start), int(received))


def plan(push_sizes, T, stride, win):
    """The whole online schedule of a video pushed in `push_sizes` (a final 0 stands for close()): per call, the clips it runs and the
    windows (0-based indices) whose flush clip is among them.  Pure bookkeeping; `OnlineVideo` follows the same steps."""
    out, nxt, received, n_run, saved = [], 0, 0, 0, 0
    sizes = list(push_sizes)
    for i, n in enumerate(sizes + [None]):
        if n is None:
            clips = close_clips(n_run, received, T, stride)
        else:
            received += int(n)
            clips, nxt = push_clips(nxt, received, T, stride)
        n_run += len(clips)
        wins = []
        for s, _, last in clips:
            if is_flush(s, last, saved, stride, win):
                wins.append(saved)
                saved += 1
        out.append({"clips": clips, "windows": wins, "received": received})
    return out


# ---- the session -----------------------------------------------------------------------------------------------------------------
class _Carry:
    """The cache rows (every kind of `MDQE.alloc_cache`) of the frames a later push's clips read -- at most T-1 -- kept on the device
    between pushes: the same-process counterpart of sharding._Halo.  `head` writes them in front of the next chunk, `on_tail`
    takes the new ones (a copy: the chunk's cache is released behind it), `tail_sent` marks that hand-over done for the chunk."""

    def __init__(self):
        self.rows, self.store, self.tail_from, self.tail_sent = 0, {}, 0, False

    def head(self, ring, at):
        for k, v in self.store.items():
            ring[k][at:at + self.rows].copy_(v)

    def on_tail(self, views):
        self.tail_sent = True
        self.store = {k: v.clone() for k, v in views.items()}
        self.rows = int(next(iter(views.values())).shape[0]) if views else 0


@dataclasses.dataclass
class Window:
    """One tracker window: frames [f0, f1), tracker instance index of each row, this window's class probabilities per track
    (provisional: the video-level class is decided at close), and the final masks -- bool [n, f1-f0, H, W] on the host -- or,
    with emit="rle", per track per frame {"size", "counts"}.  With geometry=True: boxes float32 [n, f1-f0, 4] ([xmin, ymin, xmax+1,
    ymax+1] in output pixels, zeros for an empty mask) and areas int64 [n, f1-f0] of those masks.  With emit="labels": `labels`, uint8
    [f1-f0, H, W] on the host (track_ids[i] + 1 where track i owns the pixel, 0 = background), masks and rles None, boxes / areas those
    of the labels' visible regions.  With emit="overlay": `labels` as above and `overlay`, uint8 [f1-f0, H, W, 3] on the host, the
    frames with that map painted on -- or, in a surface=True session, a preprocess.YuvFrames of f1-f0 painted surfaces.  (`labels` and `overlay` are init-only pseudo-fields stored as plain attributes:
    dataclasses.fields(Window) is what it was.)  In a session with crops=: `crops` uint8 [n, Fc, Sh, Sw, 3], `crop_rects` int32 [n, Fc, 4]
    and `crop_frames`, the Fc video frames taken (pseudo-fields of the same kind).  In a session with paths=True: `centroids` int32 [n,
    f1-f0, 2], (x, y) of each track's visible region of the label map per frame, (-1, -1) where it has none, and `moments` int64 [n,
    f1-f0, 3], its (pixels, sum of X, sum of Y) (pseudo-fields of the same kind).  In a session with matte=: `matte` uint8 [f1-f0, H, W]
    on pinned host, the soft matte of the window's tracks (render.Matte; a pseudo-field of the same kind).  In a session with
    polygons=: `polygons`, a polygons.TrackPolygons of the outlines of the window's tracks, f in video frames, k the window's row (a
    pseudo-field of the same kind).  In a session with occlusion=True: `occlusion` int32 [n, f1-f0, n] on pinned host, [k, f, j] = the
    pixels of track k's mask that track j owns (a pseudo-field of the same kind)."""
    frames: tuple
    track_ids: list
    cls_probs: torch.Tensor
    masks: torch.Tensor = None
    rles: list = None
    boxes: torch.Tensor = None
    areas: torch.Tensor = None
    labels: dataclasses.InitVar[torch.Tensor] = None
    overlay: dataclasses.InitVar[torch.Tensor] = None
    crops: dataclasses.InitVar[torch.Tensor] = None
    crop_rects: dataclasses.InitVar[torch.Tensor] = None
    crop_frames: dataclasses.InitVar[list] = None
    centroids: dataclasses.InitVar[torch.Tensor] = None
    moments: dataclasses.InitVar[torch.Tensor] = None
    matte: dataclasses.InitVar[torch.Tensor] = None
    polygons: dataclasses.InitVar[object] = None
    occlusion: dataclasses.InitVar[torch.Tensor] = None

    def __post_init__(self, labels, overlay, crops, crop_rects, crop_frames, centroids, moments, matte, polygons=None, occlusion=None):
        self.matte = matte
        self.occlusion = occlusion
        self.polygons = polygons
        self.labels = labels
        self.overlay = overlay
        self.crops, self.crop_rects, self.crop_frames = crops, crop_rects, crop_frames
        self.centroids, self.moments = centroids, moments


class OnlineVideo:
    def __init__(self, model, height=None, width=None, emit="masks", keep=False, geometry=False, style=None, ground_truth=None,
                 surface=False, surface_pitch_align=1, crops=None, paths=False, matte=None, polygons=None, occlusion=False):
        if emit not in ("masks", "rle", "labels", "overlay"):
            raise ValueError("online_video: emit must be 'masks', 'rle', 'labels' or 'overlay'")
        if not isinstance(surface, bool):
            raise ValueError("online_video: surface must be a bool, got %r" % (surface,))
        if surface and emit != "overlay":
            raise ValueError("online_video: surface=True is the form of an overlay and goes with emit='overlay' (got emit=%r)" % (emit,))
        k = surface_pitch_align
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or (k != 1 and not surface):
            raise ValueError("online_video: surface_pitch_align must be an int >= 1 (bytes) and goes with surface=True, got %r" % (k,))
        if surface and model.cfg.is_coco:
            raise ValueError("online_video: surface=True with a COCO image config: painted surfaces are a video output (use a video config)")
        self.surface, self.surface_pitch_align = surface, int(k)
        if crops is not None:
            from .render import Crops
            if not isinstance(crops, Crops):
                raise ValueError("online_video: crops must be a render.Crops, got %s" % type(crops).__name__)
            if model.cfg.is_coco:
                raise ValueError("online_video: crops with a COCO image config: per-track crops are a video output (use a video config)")
        self.crops = crops
        if not isinstance(paths, bool):
            raise ValueError("online_video: paths must be a bool, got %r" % (paths,))
        if paths and model.cfg.is_coco:
            raise ValueError("online_video: paths with a COCO image config: track centroids are a video output (use a video config)")
        self.paths = paths
        if matte is not None:
            from .render import Matte
            if not isinstance(matte, Matte):
                raise ValueError("online_video: matte must be a render.Matte, got %s" % type(matte).__name__)
            if model.cfg.is_coco:
                raise ValueError("online_video: matte with a COCO image config: the soft matte is a video output (use a video config)")
        self.matte = matte
        if polygons is not None:
            from .polygons import Polygons
            if not isinstance(polygons, Polygons):
                raise ValueError("online_video: polygons must be a polygons.Polygons, got %s" % type(polygons).__name__)
            if model.cfg.is_coco:
                raise ValueError("online_video: polygons with a COCO image config: track outlines are a video output (use a video config)")
        self.polygons = polygons
        if not isinstance(occlusion, bool):
            raise ValueError("online_video: occlusion must be a bool, got %r" % (occlusion,))
        if occlusion and model.cfg.is_coco:
            raise ValueError("online_video: occlusion with a COCO image config: the occlusion table is a video output (use a video config)")
        if occlusion:
            model.check_occlusion_capacity()
        self.occlusion = occlusion
        if emit in ("labels", "overlay") or crops is not None or paths or matte is not None or polygons is not None:
            model.check_label_capacity()
        from .render import Style
        if style is not None and (emit != "overlay" or not isinstance(style, Style)):
            raise ValueError("online_video: style must be a render.Style and goes with emit='overlay'")
        self.style = (style if style is not None else Style()) if emit == "overlay" else None
        if ground_truth is not None:
            from .vis_score import GroundTruth
            if not isinstance(ground_truth, GroundTruth):
                raise ValueError("online_video: ground_truth must be a vis_score.GroundTruth, got %s" % type(ground_truth).__name__)
        self.ground_truth = ground_truth          # the session's video is scored against it: result()["pred_gt"] (forward()'s)
        self.store = None                         # emit="overlay": the frames pushed and not yet painted (merge.FrameStore)
        if model.cfg.is_coco:
            raise RuntimeError("online_video: a COCO image config takes the single-image branch; online inference is for videos")
        if model.device.type != "cuda":
            raise RuntimeError("online_video: the model must be on a HIP device (the product has no CPU path)")
        self.model, self.emit, self.keep = model, emit, bool(keep)
        self.geometry = bool(geometry)
        self.geoms = []                           # per window (f0, frames, tracks, geom [n, F, 5] host): a few KB, kept without `keep`
        self.height, self.width = height, width
        cfg = model.cfg
        self.T, self.stride, self.win = cfg.n_frames_test, cfg.clip_stride, cfg.n_frames_window_test
        self.received, self.next_start, self.n_run = 0, 0, 0
        self.carry = _Carry()
        self.merger = None
        self.in_hw = None                         # (h0, w0) of the first push: every push must match it
        self.kept = []
        self.closed = False
        self._result = None

    @property
    def frames_held(self):
        """Frames the session holds on the device for painting or cropping (emit="overlay" or crops=; else 0): at most those no window
        has emitted yet plus the largest push - 1."""
        return self.store.frames_held if self.store is not None else 0

    @contextlib.contextmanager
    def _ctx(self):
        m = self.model
        with m._on_device(), torch.autocast(device_type="cuda", enabled=False), torch.no_grad(), m.work_stream():
            yield

    @staticmethod
    def _hw(frames):
        from .preprocess import YuvFrames
        if isinstance(frames, YuvFrames):
            return frames.height, frames.width
        f = frames if torch.is_tensor(frames) else frames[0]
        return int(f.shape[-2]), int(f.shape[-1])

    def _start(self, frames_dev, h0, w0):
        from .meta_arch import ClipMerger
        model, cfg = self.model, self.model.cfg
        self.out_size = (int(self.height if self.height is not None else h0), int(self.width if self.width is not None else w0))
        if self.surface and self.out_size != (int(h0), int(w0)):
            raise ValueError("online_video: surface=True paints the surfaces at their own size %s, the session's output size (height, "
                             "width) is %s; ask for height=%d, width=%d (to run the model below that size, push full-size surfaces and "
                             "set model.resize_on_device)" % ((int(h0), int(w0)), self.out_size, h0, w0))
        h, w = int(frames_dev.shape[-2]), int(frames_dev.shape[-1])
        self.hw = (h, w)
        self.geo = model.engine.geometry(h, w)
        self.mask_hw = (self.geo.Hp // cfg.match_stride, self.geo.Wp // cfg.match_stride)
        if self.emit == "overlay" or self.crops is not None:
            from .merge import FrameStore
            self.store = FrameStore()
        self.merger = ClipMerger(model, self.hw, self.out_size, self.mask_hw, n_frames=None, online=self.emit,
                                 geometry=self.geometry, frame_source=self.store, style=self.style, ground_truth=self.ground_truth,
                                 surface=self.surface, surface_pitch_align=self.surface_pitch_align, crops=self.crops, paths=self.paths,
                                 matte=self.matte, polygons=self.polygons, **({"occlusion": True} if self.occlusion else {}))
        shapes = model.engine.cache_shapes(self.geo)
        per_frame = 4 * sum(int(np.prod(sh)) for sh in shapes.values())
        budget = cache_budget_frames(per_frame, model.CACHE_GB)
        self.chunk = max(1, budget - (self.T - 1))   # frames of one iter_clip_results call: chunk + carry fit one cache buffer

    def _run(self, frames_dev, h2d, clips, offset):
        """The clips of one chunk (frames_dev[0] = global frame `offset`) through iter_clip_results with the carry, fed to the
        tracker per decoder batch as merge_clips does.  Returns the windows flushed."""
        model, m = self.model, self.merger
        self.carry.tail_sent = False
        self.carry.tail_from = carry_from(self.next_start, offset + int(frames_dev.shape[0]))
        n0 = len(m.emitted)
        m.feed_batches(model.iter_clip_results(frames_dev, clips, offset, h2d=h2d, carry=self.carry), to_the_end=True)
        m.main.wait_stream(m.side)
        self.n_run += len(clips)
        return m.emitted[n0:]

    def _windows(self, recs):
        out = []
        for r in recs:
            if r["ready"] is not None:
                r["ready"].synchronize()
            n = int(r["cls_probs"].shape[0])
            boxes = areas = None
            if self.geometry:                     # (the table came with the masks: same stream and event, or the same sync as the positions)
                from . import rle as R
                boxes, areas = R.geom_to_boxes(r["geom"])
                self.geoms.append((r["frames"][0], r["frames"][1] - r["frames"][0], n, r["geom"]))
            out.append(Window(frames=r["frames"], track_ids=list(range(n)), cls_probs=r["cls_probs"],
                              masks=r.get("masks"), rles=r.get("rles"), boxes=boxes, areas=areas, labels=r.get("labels"),
                              overlay=r.get("overlay"), crops=r.get("crops"), crop_rects=r.get("crop_rects"),
                              crop_frames=r.get("crop_frames"), centroids=r.get("centroids"), moments=r.get("moments"),
                              matte=r.get("matte"), polygons=r.get("polygons"), occlusion=r.get("occlusion")))
        del self.merger.emitted[:]
        if self.store is not None:
            # the chunks that lie wholly before the first frame no window has emitted are done with; what stays and may be the caller's
            # own device tensor is copied before control returns (the caller may refill its buffer for the next push)
            self.store.drop_before(self.merger.f_off)
            self.store.own()
        if self.keep:
            self.kept.extend(out)
        return out

    def push(self, frames):
        """Frames [n, 3, h, w] (uint8 or float32, host or device) of the video, in order, or n decoder surfaces (a
        preprocess.YuvFrames, host or device: converted on the device, the picture of an overlay is painted on the converted frames in
        their `order`).  Runs every clip whose frames are all present now and returns the windows that completed, in order."""
        if self.closed:
            raise RuntimeError("online_video: push() after close()")
        n = int(frames.shape[0]) if torch.is_tensor(frames) else len(frames)
        if n == 0:
            return []
        if self.ground_truth is not None and self.received + n > self.ground_truth.length:
            raise RuntimeError("online_video: this push brings the video to %d frames, the ground truth holds %d"
                               % (self.received + n, self.ground_truth.length))
        if self.surface:
            from .preprocess import YuvFrames
            if not isinstance(frames, YuvFrames):
                raise ValueError("online_video: a surface=True session paints onto decoder surfaces and takes pushes of "
                                 "preprocess.YuvFrames, got %s (for RGB frames open the session with surface=False)" % type(frames).__name__)
        hw0 = self._hw(frames)
        if self.in_hw is not None and hw0 != self.in_hw:
            raise RuntimeError("online_video: frame size %s differs from the first push's %s" % (hw0, self.in_hw))
        if self.surface and self.store is not None and self.store.surface is not None and frames.meta() != self.store.surface:
            raise ValueError("online_video: this push's surfaces are (height, width, fmt, matrix, full_range, order) = %s, the first "
                             "push's %s; one session's surfaces are of one kind" % (frames.meta(), self.store.surface))
        with self._ctx():
            model = self.model
            frames_dev, h2d, h0, w0, src, src_ready, uploaded = model._frames_and_source({"image": frames}, surface=self.surface)
            if self.merger is None:
                self.in_hw = hw0
                self._start(frames_dev, h0, w0)
            recs, r0 = [], self.received
            if self.store is not None:
                self.store.add(r0, src, src_ready, owned=uploaded)
            if n > self.chunk and h2d:
                torch.cuda.current_stream(model.device).wait_event(h2d[-1][1])   # (sub-chunks: the whole upload first)
                h2d = None
            for a in range(0, n, self.chunk):
                b = min(n, a + self.chunk)
                self.received = r0 + b
                clips, self.next_start = push_clips(self.next_start, self.received, self.T, self.stride)
                recs += self._run(frames_dev[a:b], h2d, clips, r0 + a)
            return self._windows(recs)

    def close(self):
        """The end of the video: the clips of the offline schedule no push could run (the clamped last clip) and the final flush.
        Returns the remaining windows."""
        if self.closed:
            raise RuntimeError("online_video: close() after close()")
        if self.received == 0:
            raise RuntimeError("online_video: close() without frames")
        self.closed = True
        L = self.received
        clips = close_clips(self.n_run, L, self.T, self.stride)
        if not clips:
            return []
        self.next_start = L
        with self._ctx():
            h, w = self.hw
            empty = torch.empty((0, 3, h, w), dtype=torch.float32, device=self.model.device)
            return self._windows(self._run(empty, None, clips, L))

    def result(self):
        """After close(): {"image_size", "pred_scores", "pred_labels", "pred_track_ids"} -- the video-level top-k of
        `inference_video`; pred_track_ids[j] is the track behind output j.  keep=True adds "pred_masks" (or "pred_rles", or
        "pred_label_map", or that and "pred_overlay"), assembled from the windows handed out, equal to forward()'s; geometry=True adds "pred_boxes" / "pred_areas"
        (forward()'s with model.geometry_output; emit="labels": "pred_label_boxes" / "pred_label_areas"), with or without keep."""
        if not self.closed:
            raise RuntimeError("online_video: result() before close()")
        if self._result is not None:
            return self._result
        if not self.merger.cls_clips:
            raise RuntimeError("online_video: no tracker window was flushed (the schedule of this length has no last clip)")
        from . import merge
        forms, (Ho, Wo) = self.merger.forms, self.out_size
        with self._ctx() if self.merger.score is not None else contextlib.nullcontext():
            res, inst = merge.result_head(self.model, self.merger.cls_clips, self.out_size, self.received, self.merger.score)
        if self.geometry:                         # (the windows' tables: the planes' or, for the label forms, the labels' visible regions')
            res.update(merge.track_geometry(inst, self.received, self.out_size, self.geoms, labels=forms.labels))
        if self.keep and forms.labels:
            res["pred_label_map"] = torch.cat([w.labels for w in self.kept])
            if forms.overlay:
                if self.surface:
                    from .preprocess import YuvFrames
                    res["pred_overlay"] = YuvFrames.cat([w.overlay for w in self.kept])
                else:
                    res["pred_overlay"] = torch.cat([w.overlay for w in self.kept])
        elif self.keep:
            wins = [(w.frames[0], w.frames[1] - w.frames[0], len(w.track_ids), w.rles if forms.planes == "rle" else w.masks) for w in self.kept]
            if forms.planes == "rle":
                res["pred_rles"] = merge.stitch_rles(inst, self.received, (Ho, Wo), wins)
            else:
                res["pred_masks"] = merge.stitch(inst, self.received, wins, lambda k: torch.zeros((k, Ho, Wo), dtype=torch.bool), torch.cat)
        if self.keep and forms.crops:             # (per output the track's chips over the taken frames; absent before its first window)
            spec = self.crops
            fill = torch.tensor(spec.fill, dtype=torch.uint8).expand(spec.size + (3,))
            none = torch.tensor([0, 0, -1, -1], dtype=torch.int32)
            at = [(spec.count(w.frames[0]), len(w.crop_frames), len(w.track_ids)) for w in self.kept]
            lc = spec.count(self.received)
            for key, attr, empty in (("pred_crops", "crops", fill), ("pred_crop_rects", "crop_rects", none)):
                rows = merge.stitch(inst, lc, [a + (getattr(w, attr),) for a, w in zip(at, self.kept)],
                                    lambda k, e=empty: e.expand((k,) + tuple(e.shape)), torch.cat)
                res[key] = torch.stack(rows) if rows else torch.zeros((0, lc) + tuple(empty.shape), dtype=empty.dtype)
            res["pred_crop_frames"] = spec.taken(0, self.received)
        if self.keep and forms.matte:             # (the windows tile the video: their planes in a row)
            res["pred_matte"] = torch.cat([w.matte for w in self.kept])
        if self.keep and forms.paths:             # (per output the track's path; absent before its first window)
            res.update(merge.path_result(inst, self.received, [(w.frames[0], w.frames[1] - w.frames[0], len(w.track_ids), w.centroids, w.moments)
                                                               for w in self.kept]))
        if self.keep and forms.polygons:          # (the windows' rings in a row, their rows renumbered to the outputs)
            res.update(merge.polygon_result(inst, self.out_size, [w.polygons for w in self.kept]))
        if self.keep and forms.occlusion:         # (per output the track's rows of the windows' tables; zero before its first window)
            res.update(merge.occlusion_result(inst, self.received, [(w.frames[0], w.frames[1] - w.frames[0], len(w.track_ids), w.occlusion)
                                                                    for w in self.kept]))
        self._result = res
        return res
