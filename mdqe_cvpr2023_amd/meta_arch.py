"""MDQE meta-architecture: the drop-in for the reference's `MDQE` (mdqe/mdqe.py:60-471) on the
eval-only VIS path.

    model = MDQE(cfg)                      # cfg: the reference's CfgNode, or an MDQEConfig
    model.load_state_dict(ckpt["model"])   # reference checkpoint names (prefix `detr.`)
    out = model([{"image": [uint8 [3,h,w], ...], "height": H, "width": W}])
    # -> {"image_size", "pred_scores", "pred_labels", "pred_masks": [BoolTensor[L,H,W] (CPU)]}

Same call contract and output dict as MDQE.forward -> inference_vis -> inference_video.  When
detectron2 is importable the class is registered in its META_ARCH_REGISTRY under the names "MDQE" (taking the slot over from the
reference's model if `mdqe` was imported first) and "MDQE_MI355X" -- `register_with_detectron2` at the end of this file.
COCO image sets (`DATASETS.TEST[0]` = coco*) take the single-image branch (`inference_image`); training is out of scope and raises.
"""
import contextlib
import os
from collections import OrderedDict, deque

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .config import MDQEConfig, from_d2_cfg
from .engine import Engine
from .params import ALIASES, full_manifest, random_state
from . import merge, schedule
from .merge import ClipMerger      # (merge_clips, sharding and online resolve the class through THIS namespace at call time)


def _register(root: nn.Module, dotted: str, tensor: torch.Tensor, buffer=False):
    parts = dotted.split(".")
    m = root
    for p in parts[:-1]:
        if p not in m._modules:
            m.add_module(p, nn.Module())
        m = m._modules[p]
    if buffer:
        m.register_buffer(parts[-1], tensor)
    else:
        m.register_parameter(parts[-1], nn.Parameter(tensor, requires_grad=False))


# The pipeline's HIP streams, ONE set per device and process, shared by every MDQE instance (a process runs one model at a time, as the
# reference's harness does).  HIP deals streams onto its hardware queues in the order they are first used and a queue is served in order,
# so WHICH streams share a queue decides how well the pipeline overlaps (tools/stream_map_ab.py): a second model in the same process -- the
# bench's extra configurations, an evaluator that rebuilds the model -- used to create a second set of streams and land on another, usually
# worse, deal (Swin-L as the third model of a bench process: 135 against 150 frames/s in a process of its own).
_STREAMS = {}
HALO_EARLY_DECODE = os.environ.get("MDQE_HALO_EARLY_DECODE", "1") != "0"     # (A/B knob: 0 = round 4's behaviour)
HALO_OWN_STREAM = os.environ.get("MDQE_HALO_OWN_STREAM", "1") != "0"         # (A/B knob: 0 = the halo hand-over on the frame stream)


def _shared_stream(name):
    def key(self):
        d = self.device
        return ("cpu",) if d.type != "cuda" else (d.index if d.index is not None else torch.cuda.current_device(),)

    def get(self):
        return _STREAMS.get(key(self) + (name,))

    def put(self, stream):
        if stream is not None:
            _STREAMS[key(self) + (name,)] = stream
    return property(get, put)


class _PlannedGroup:
    """Runtime state of a planned group of clips (schedule.Group): the rows it reads and the events around it."""
    __slots__ = ("cache", "ready", "dec_ready", "outs", "done")

    def __init__(self, cache, ready, dec_ready):
        self.cache = cache                        # name -> the buffer's rows [0, rows)
        self.ready, self.dec_ready = ready, dec_ready   # behind its last frame pass / behind what the DECODER reads of that pass
        self.outs = None                          # decoder outputs, where the group was decoded ahead
        self.done = None                          # behind its inference_clips: the group no longer reads its buffer


class _ClipIssuer:
    """The issuing half of `MDQE.iter_clip_results`: the streams, the two cache buffers and the planned groups of one call, and one
    method per step of the plan (schedule.plan_steps) that issues the work the step stands for.  It decides nothing about the schedule;
    what it checks at run time is what the plan cannot know (a GPU or not, the A/B knobs, a trace)."""

    def __init__(self, model, frames_dev, geo, chunk, trace, on_frames_queued, h2d, halo, carry, side_streams):
        self.model, self.eng, self.frames_dev, self.geo, self.chunk = model, model.engine, frames_dev, geo, chunk
        self.trace, self.on_frames_queued, self.h2d, self.halo, self.carry = trace, on_frames_queued, h2d, halo, carry
        self.side_streams = side_streams
        self.cuda = cuda = frames_dev.is_cuda
        self.clip_stream = torch.cuda.current_stream(frames_dev.device) if cuda else None
        if cuda and model._frame_stream is None:
            model._frame_stream = torch.cuda.Stream(frames_dev.device)
        self.fstream = (model._frame_stream if model.overlap_streams else self.clip_stream) if cuda else None
        self.bufs = [model.alloc_cache(chunk.capf, geo, keep_enc=halo is not None), None]
        self.readers = [[], []]                   # buffer -> the groups that read it since it was last switched to
        self.groups = deque()                     # planned (their frames queued on the frame stream) and not yet decoded, in clip order
        self.started = False
        self.pass_ready = self.pass_dec_ready = None      # the events of the pass queued last
        self.tail_views = self.tail_ev = None     # (halo) the chunk's last T-1 frames and the event they are complete behind
        self.consuming = False                    # False while the generator is being primed
        self.carry_ev = None                      # (online carry) the event behind the hand-over of the chunk's tail rows
        if carry is not None and chunk.lead:
            with self.fctx():
                if cuda and self.fstream is not self.clip_stream:
                    self.fstream.wait_stream(self.clip_stream)
                carry.head(self.bufs[0], 0)       # in front of every pass and every `ready` event of this chunk

    def fctx(self):
        return torch.cuda.stream(self.fstream) if self.cuda else contextlib.nullcontext()

    def switch_segment(self, step):
        """Frames [first, first + keep) are copied over once; the groups that read that buffer two segments ago have finished (events)."""
        bufs, nb = self.bufs, step.buffer
        if bufs[nb] is None:
            bufs[nb] = self.model.alloc_cache(self.chunk.capf, self.geo)
        with self.fctx():
            for g in self.readers[nb]:
                if self.cuda and g.done is not None:
                    self.fstream.wait_event(g.done)
            self.readers[nb] = []
            if step.keep > 0:
                o = step.src_row
                for k, v in bufs[nb].items():
                    v[:step.keep].copy_(bufs[1 - nb][k][o:o + step.keep])

    def queue_pass(self, step):
        """A frame pass, asynchronous on the frame stream, stored in place at the rows of its frames."""
        cuda, fstream = self.cuda, self.fstream
        with self.fctx():
            if cuda:
                if not self.started and fstream is not self.clip_stream:
                    fstream.wait_stream(self.clip_stream)              # the frames (and weights) were produced on the caller's stream
                if self.h2d:                                           # the upload chunks this pass reads (upload_frames)
                    for end, ev in self.h2d:
                        if end > step.n0:
                            fstream.wait_event(ev)
                        if end >= step.n1:
                            break
            self.started = True
            # what the DECODER reads of this pass is complete (the mask features may still be on their way).  (Also with the halo
            # exchange since round 5: the neighbour's rows are written on the clip stream itself, in front of the group that reads them.)
            dr = torch.cuda.Event() if cuda and self.model.early_decode and (self.halo is None or HALO_EARLY_DECODE) else None
            self.model._frame_cache(self.frames_dev[step.n0:step.n1], self.geo, ring=self.bufs[step.buffer], at=step.row, dec_ready=dr)
            ready = None
            if cuda:
                ready = torch.cuda.Event()
                ready.record(fstream)
        self.pass_ready, self.pass_dec_ready = ready, dr

    def halo_tail(self, step):
        buf = self.bufs[step.buffer]
        self.tail_views = (buf["enc"][step.row0:step.row1], buf["mf"][step.row0:step.row1])
        self.tail_ev = self.pass_ready if step.new_pass else None
        if self.cuda and self.tail_ev is None:
            self.tail_ev = torch.cuda.Event()
            self.tail_ev.record(self.fstream)

    def plan_group(self, step):
        ready, dec_ready = (self.pass_ready, self.pass_dec_ready) if step.new_frames else (None, None)
        if self.cuda and ready is None:           # no new pass (rows of earlier passes, maybe copied by a segment switch): all that is queued so far
            ready = torch.cuda.Event()
            with self.fctx():
                ready.record(self.fstream)
        g = _PlannedGroup({k: v[:step.rows] for k, v in self.bufs[step.buffer].items()}, ready, dec_ready)
        self.readers[step.buffer].append(g)
        self.groups.append(g)
        if step.frames_queued and self.on_frames_queued is not None:
            # once, when the LAST frame of this video has been queued on the frame stream: a caller that streams videos
            # queues the next video's first pass now, under this video's remaining clip / tracker work
            cb, self.on_frames_queued = self.on_frames_queued, None
            cb()

    def carry_tail(self, step):
        """(online carry) Once every clip is planned and the frames from `carry.tail_from` on are through the per-frame stages: their
        cache rows -- carried rows in front of the chunk included -- to `carry.on_tail` on the frame stream."""
        with self.fctx():
            self.carry.on_tail({k: v[step.row0:step.row1] for k, v in self.bufs[0].items()})
            if self.cuda:
                self.carry_ev = torch.cuda.Event()
                self.carry_ev.record(self.fstream)

    def send_tail(self):
        """The grouped send/recv of the halo exchange, behind the chunk's last pass.  Never while the
        generator is being primed: every rank must issue it at the same point of its program -- between the gathers of two
        rounds -- or a rank whose chunk is a single pass would queue it BEFORE the previous round's gather and RCCL, which runs
        a rank's operations in issue order, would deadlock against a rank that queued it after."""
        halo, model = self.halo, self.model
        # What keeps the exchange out of the priming phase is the PLAN: it puts `send_tail` on Consume steps only, and the generator's
        # loop sets `consuming` right in front of each.  The check below cannot fire as the code stands; it only catches a future edit
        # that calls this from a planning step (which hangs ranks) -- do not rely on it.
        if not self.consuming:
            raise RuntimeError("halo exchange: send_tail() while the generator is being primed -- the grouped send/recv must be "
                               "issued between the gathers of two rounds on every rank")
        if not self.cuda or not HALO_OWN_STREAM:
            with self.fctx():
                if self.cuda:
                    self.fstream.wait_event(self.tail_ev)
                halo.on_tail(*self.tail_views)
            return
        # On the model's COPY stream, behind the event of the chunk's last pass only.  (Rounds 3-4 issued it on the frame stream --
        # which by now holds the NEXT round's primed passes: the message, and with it the last decoder group of every rank of this
        # round, waited for 1-3 passes of the next round.)
        if model._copy_stream is None:
            model._copy_stream = torch.cuda.Stream(self.frames_dev.device)
        hs = model._copy_stream
        hs.wait_event(self.tail_ev)
        with torch.cuda.stream(hs):
            halo.on_tail(*self.tail_views)
        for v in self.tail_views:
            v.record_stream(hs)

    def consume(self, step):
        """Decoder + inference_clips of the oldest planned group; yields its clips' (start, end, last, res)."""
        model, eng, cuda, clip_stream = self.model, self.eng, self.cuda, self.clip_stream
        if step.send_tail:
            self.send_tail()
        cur = self.groups.popleft()
        cache, T, starts = cur.cache, step.group.T, list(step.starts)
        dr = cur.dec_ready if cuda else None
        if cuda:
            clip_stream.wait_event(dr if dr is not None else cur.ready)
        if step.straddlers:
            enc_h, mf_h = self.halo.head()                     # (waits for the neighbour's message on this stream)
            model._cache_from_tokens(enc_h, mf_h, self.geo, self.bufs[step.group.buffer], 0)
        outs = cur.outs
        if outs is None:
            # side_streams=False (the sharded schedule): HIP multiplexes its streams onto 4 hardware queues, and with RCCL's stream
            # and the replay thread's tracker stream in play the decoder's instance-chain stream lands on a queue behind the frame
            # stream's long GEMMs -- 616 against 708 frames/s per rank (tools/hwq_ab2.sh; GPU_MAX_HW_QUEUES=8 recovers most of it,
            # 697, but costs the single-GPU path 1.6 %)
            outs = eng.decode_clips(cache, starts, T, self.geo, two_streams=self.side_streams)
        elif cuda:
            clip_stream.wait_stream(model._ahead_stream)       # decoded ahead (below) on the auxiliary stream
            for v in outs.values():
                v.record_stream(clip_stream)
        # Decode-ahead: a following group that needs NO new frame pass -- the short clips at the end of a video, whose frames the
        # last pass has already produced -- is decoded now, on an auxiliary stream beside this group's decoder, instead of after
        # this group's inference_clip syncs and tracker run.  Both decoders are chains of small dependent launches (latency-bound
        # at these sizes), so the second one is nearly free: the tail of a 120-frame video drops by the 2.6 ms the lone 3-frame
        # clip took (tools/tail_time.py).  Same kernels, same inputs, same bits.
        if step.ahead is not None and cuda and model.decode_ahead and self.side_streams and self.trace is None and self.groups[0].outs is None:
            nx, nxg = self.groups[0], step.ahead
            if model._ahead_stream is None:
                model._ahead_stream = torch.cuda.Stream(self.frames_dev.device, priority=-1)
            aux = model._ahead_stream
            aux.wait_event(nx.ready)                           # its frames (the pass this group waits for too)
            with torch.cuda.stream(aux):
                nx.outs = eng.decode_clips(nx.cache, list(nxg.starts), nxg.T, self.geo)
        if dr is not None:
            clip_stream.wait_event(cur.ready)                  # the mask features of the group's last pass (inference_clip reads them)
        ress = eng.inference_clips(outs, cache["mf"], starts, T)
        ready = None
        if cuda:
            ready = torch.cuda.Event()
            ready.record(clip_stream)             # the clip results are complete once this event fires
        cur.done = ready                          # ... and the group no longer reads its buffer
        group = self.chunk.clips[step.group.i:step.group.j] + step.straddlers
        for gi, ((start, end, last), res) in enumerate(zip(group, ress)):
            if self.trace is not None:
                self.trace.append({k_: v.clone() for k_, v in res.items() if torch.is_tensor(v)})
            res["ready"] = ready
            res["batch_end"] = gi == len(group) - 1
            yield start, end, last, res

    def finish(self):
        if self.carry_ev is not None:
            # the tail passes no group waited for: the chunk's frames and cache are released on the caller's stream after them
            self.clip_stream.wait_event(self.carry_ev)

    # step type -> the method that issues it (plain functions: an issuer that held its own bound methods would be a reference cycle, and
    # its cache buffers would wait for the garbage collector instead of being released with the generator)
    ISSUE = {schedule.Switch: switch_segment, schedule.Pass: queue_pass, schedule.HaloTail: halo_tail, schedule.Group: plan_group,
             schedule.CarryTail: carry_tail}


class MDQE(nn.Module):
    _trk_stream = _shared_stream("tracker")
    _frame_stream = _shared_stream("frame")
    _copy_stream = _shared_stream("copy")
    _ahead_stream = _shared_stream("ahead")
    _work_stream = _shared_stream("work")

    def __init__(self, cfg, state_dict=None, backbone_fn=None, seed=0):
        super().__init__()
        self.cfg = cfg if isinstance(cfg, MDQEConfig) else from_d2_cfg(cfg)
        self.device = torch.device(self.cfg.device)
        self._backbone_fn = backbone_fn
        self._engine = None
        sd = state_dict if state_dict is not None else random_state(self.cfg, seed)
        man = full_manifest(self.cfg)
        if state_dict is not None:
            sd = dict(sd)
            for k in list(sd):                       # released checkpoints carry the decoder's shared modules under an alias too
                for a, b in ALIASES.items():
                    if k.startswith(a) and (b + k[len(a):]) not in sd:
                        sd[b + k[len(a):]] = sd[k]
            missing = [n for n in man if n not in sd]
            if missing:                              # a partial / mis-prefixed checkpoint must not become silent all-zero layers
                raise KeyError("MDQE(cfg, state_dict=...): %d parameters of the manifest are missing, e.g. %s" % (len(missing), missing[:5]))
        for name, shape in man.items():
            t = sd[name]
            _register(self, name, t.detach().clone().float(), buffer=name.endswith(("running_mean", "running_var")))
        self._extra = {k: v for k, v in sd.items() if k not in man}      # e.g. custom-backbone weights
        # frames per pass of the per-frame stages: 0 = by resolution (~300k encoder tokens per pass: at most 40 frames: 40 at 360p, 20 at 640p)
        self.frame_batch = int(os.environ.get("MDQE_FRAME_BATCH", "0"))
        # priority of the tracker's stream (0 normal, -1 high): its kernels are small and sit on the per-clip critical path of the replay
        self.trk_priority = int(os.environ.get("MDQE_TRK_PRIORITY", "0"))
        self.resize_on_device = False               # True: frames arrive at native size and get the mapper's ResizeShortestEdge here
        self.rle_output = False                     # True: forward() returns per-frame COCO RLEs ("pred_rles") instead of dense masks
        # True: forward() on a video adds "pred_boxes" (float32 [L, 4] XYXY_ABS per output) and "pred_areas" (int64 [L]) of the final masks,
        # gathered by the kernels that write / encode the masks (ops.final_masks_geom / final_masks_rle_geom); off: nothing changes
        self.geometry_output = False
        # True: forward() on a video adds "pred_label_map" (uint8 [L, Ho, Wo] on the host: which track owns each pixel, label t + 1 = tracker
        # row t, 0 = background; the row with the largest up-sampled logit among ALL tracks of the window whose mask holds the pixel --
        # also one that misses the video-level top-k: rle.labels_keep drops those) and "pred_track_ids" (the row behind output j), built on
        # the device by ops.final_label_map: 1 byte per pixel however many tracks.  "only": the same without the per-track planes
        # ("pred_masks" is []: no dense-mask kernels, pinned buffers or copies).  With geometry_output also "pred_label_boxes" /
        # "pred_label_areas" of the labels' visible regions.  False: nothing changes.  (A property: see `label_output` below.)
        self.label_output = False
        # True: forward() on a video adds "pred_overlay" (uint8 [L, Ho, Wo, 3], pinned host: the label map painted over the frames handed
        # in, at their uploaded size -- before `resize_on_device` -- nearest-sampled to the output size; pixel-interleaved, channel order =
        # the frames'; ops.render_overlay behind ops.final_label_map, 3 bytes per pixel however many tracks) and "pred_track_ids".  The map
        # itself is returned only with label_output.  `overlay_style` (render.Style): alpha, contour reach, palette.  Videos only (the COCO
        # image branch has no overlay), one device (sharding.py refuses it).  False: nothing changes.  (Properties: see below.)
        # "surface": for a video handed in as decoder surfaces (preprocess.YuvFrames) "pred_overlay" is a YuvFrames of L PAINTED SURFACES
        # of the same format (pinned host, tight pitch), painted in the YUV domain (ops.render_overlay_yuv): a background pixel keeps the
        # decoder's bits, 1.5 bytes per pixel are kept and read back instead of 3, and the result goes to an encoder as it is.  The
        # output size must be the surfaces' (nothing is resampled); RGB frames are refused.
        self.overlay_output = False
        # A render.Crops: forward() on a video adds "pred_crops" / "pred_crop_rects" / "pred_crop_frames", one fixed-size picture per
        # output and taken frame, cut and resized on the device (ops.track_crops).  None: nothing changes.  (A property: see below.)
        self.crop_output = None
        # True: forward() on a video adds "pred_centroids" / "pred_moments", where each output's track is in every frame, summed on the
        # device from the label map (ops.label_centroids).  False: nothing changes.  (A property: see below.)
        self.path_output = False
        # A polygons.Polygons: forward() on a video adds "pred_polygons", the outlines of each output's visible regions as rings of
        # lattice corners, traced on the device from the label map (ops.label_polygons).  None: nothing changes.  (A property: see below.)
        self.polygon_output = None
        # True: forward() on a video adds "pred_occlusion" (int32 [n_out, L, n_out + 1]: how much of each output's mask every output owns,
        # counted on the device by ops.final_occlusion).  False: nothing changes.  (A property: see below.)
        self.occlusion_output = False
        self.merge_on_cpu = None                 # None: cfg.merge_on_cpu (MODEL.MDQE.MERGE_ON_CPU); True / False override it
        # Final masks of a tracker window leave the device when the window is flushed (pinned host buffers, copied under the later
        # windows' compute) instead of in one pass + one 100-MB copy after the last window.  Independent of MERGE_ON_CPU, which in the
        # reference only picks the device the window results wait on (mdqe/mdqe.py:185-186,337,354-355) and never changes an output.
        self.early_masks = os.environ.get("MDQE_EARLY_MASKS", "1") != "0"
        self.decode_ahead = os.environ.get("MDQE_DECODE_AHEAD", "1") != "0"         # trailing short clips decoded beside the last full group
        # the decoder of a group starts as soon as ITS inputs of the group's last frame pass exist (queries + value projections); the
        # mask-feature head of that pass, which only inference_clip reads, runs beside the decoder's first layers (round 4)
        self.early_decode = os.environ.get("MDQE_EARLY_DECODE", "1") != "0"
        self.overlap_streams = os.environ.get("MDQE_OVERLAP_STREAMS", "1") != "0"   # frame stages on their own stream
        self.clip_priority = os.environ.get("MDQE_CLIP_PRIORITY", "1") != "0"       # per-clip stages on a high-priority stream
        self.stage_times = None
        self.taper_passes = os.environ.get("MDQE_TAPER_PASSES", "1") != "0"   # half-size first / last frame pass (pipeline fill / drain)
        self.taper_tail = int(os.environ.get("MDQE_TAPER_TAIL", "0"))          # frames of the last pass (0: half a pass)
        self.lookahead = max(1, int(os.environ.get("MDQE_LOOKAHEAD", "2")))   # groups whose frame passes are queued ahead of the one being decoded
        # clips per decoder batch the planner waits for before it fixes a group (0: the clips ONE frame pass completes, rounds 2-4): the
        # cache is per frame and the decoder reads it through index tables, so its batch is independent of the pass size
        self.dec_batch = int(os.environ.get("MDQE_DEC_BATCH", "0"))

    # ---- checkpoint contract ---------------------------------------------------------------------
    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        # accept (and drop) the reference checkpoint's aliased / non-eval keys
        for k in list(state_dict):
            kk = k[len(prefix):]
            # (+ the SwinV2 blocks' fixed buffers -- `relative_coords_table`, `relative_position_index`, swin_transformer_v2.py:120,133 -- and
            # the shift masks some exports carry: functions of the window size, rebuilt here)
            if any(kk.startswith(a) for a in ALIASES) or kk.endswith((".sampling_offsets", "lvl_spatial_scales",
                                                                      "query_relpos_grid", "num_batches_tracked",
                                                                      "relative_coords_table", "relative_position_index", "attn_mask")) \
                    or kk.startswith("criterion."):
                if not (kk.endswith(".sampling_offsets.weight") or kk.endswith(".sampling_offsets.bias")):
                    state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        self._engine = None

    def train(self, mode=True):
        if mode:
            raise RuntimeError("mdqe_cvpr2023_amd.MDQE implements the eval-only path (SURVEY.md §8); training is out of scope -- to train, "
                               "select the reference's model: MODEL.META_ARCHITECTURE MDQE_REFERENCE, or MDQE_MI355X_REGISTER=alias in the "
                               "environment so that 'MDQE' stays the reference's")
        return super().train(False)

    @property
    def engine(self) -> Engine:
        if self._engine is None:
            sd = OrderedDict((k, v) for k, v in self.state_dict().items())
            sd.update(self._extra)
            with self._on_device():
                self._engine = Engine(self.cfg, sd, self.device, backbone_fn=self._backbone_fn)
        return self._engine

    @property
    def precision_map(self):
        """"" = exact fp32 everywhere (default); "reference" = the reference harness's own precision map on a GPU with its fp16 regions on the
        f16x3 split-precision kernels (engine.Engine.precision_map; env MDQE_PRECISION_MAP)."""
        return self.engine.precision_map

    @precision_map.setter
    def precision_map(self, v):
        if v not in ("", "reference", "autocast_f16"):
            raise ValueError("precision_map: '', 'reference' or 'autocast_f16'")
        self.engine.precision_map = v

    # ---- forward (mdqe/mdqe.py:194-242) ------------------------------------------------------------
    def _make_streams(self):
        """The pipeline's normal-priority streams, created TOGETHER and in a fixed order (copy, frame, tracker) the first time the model
        runs on a GPU.  HIP deals its streams onto 4 hardware queues in creation order and a queue is served in order, so WHICH streams
        share a queue is decided here -- and it matters: with one / three foreign normal-priority streams created before these, the
        same pipeline runs 5 % / 11 % slower (tools/stream_map_ab.py: 760 -> 719 / 679 frames/s; two: 754).  `MDQE_STREAM_PAD=k` shifts
        the deal by k queues for a process that has created streams of its own before the model's first call."""
        pad = int(os.environ.get("MDQE_STREAM_PAD", "0"))
        self._pad_streams = [torch.cuda.Stream(self.device) for _ in range(max(pad, 0))]
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        if self._frame_stream is None:
            self._frame_stream = torch.cuda.Stream(self.device)
        if self._trk_stream is None:
            self._trk_stream = torch.cuda.Stream(self.device, priority=self.trk_priority)
        # a stream gets its hardware queue when it is first USED, not when it is created (unused foreign streams change nothing,
        # tools/stream_pad_ab.sh).  The pipeline's natural first-use order (copy, frame, tracker, between the high-priority streams'
        # first uses) is the best deal measured; MDQE_STREAM_TOUCH=1 instead touches [pads,] copy, frame, tracker here, in that order --
        # a knob for a host process whose own streams have shifted the deal (tools/stream_touch_ab.sh: 731-735 against 737-745 frames/s)
        order = os.environ.get("MDQE_STREAM_ORDER", "")          # tools/stream_order_ab.sh: first-use order of ALL the pipeline's streams
        if order:
            if self._ahead_stream is None:
                self._ahead_stream = torch.cuda.Stream(self.device, priority=-1)
            from .engine import INST_STREAMS as pool
            inst = pool.setdefault(self._work_stream.cuda_stream, torch.cuda.Stream(self.device, priority=-1))
            table = {"w": self._work_stream, "i": inst, "a": self._ahead_stream, "c": self._copy_stream, "f": self._frame_stream, "t": self._trk_stream}
            for ch in order:
                st = table.get(ch) or torch.cuda.Stream(self.device, priority=-1 if ch == "X" else 0)
                if ch not in table:
                    self._pad_streams.append(st)
                with torch.cuda.stream(st):
                    torch.zeros(1, device=self.device)
        elif os.environ.get("MDQE_STREAM_TOUCH", "0") == "1" or getattr(self, "_touch_on_create", False):
            for st in self._pad_streams + [self._copy_stream, self._frame_stream, self._trk_stream]:
                with torch.cuda.stream(st):
                    torch.zeros(1, device=self.device)

    def touch_streams(self):
        """Give the pipeline's normal-priority streams their hardware queues NOW, in a fixed order (copy, frame, tracker): a stream gets its
        queue when it is first used, and whatever creates streams of its own in between -- a second RCCL communicator (the halo exchange's),
        a host application -- shifts the deal.  The sharded schedule calls this before it creates anything else (one-rank halo-exchange
        rehearsal under 8 queues: 180.9 ms per step without, 153.5 with; profiles/r05_ab_halo_exchange_queues.txt).  Once per process."""
        if self.device.type != "cuda" or os.environ.get("MDQE_NO_STREAM_TOUCH") == "1":
            return
        key = ("touched", self.device.index if self.device.index is not None else torch.cuda.current_device())
        if _STREAMS.get(key):
            return
        _STREAMS[key] = True
        if self._work_stream is not None:
            return                                     # the streams are in use already: their queues are taken
        # the same order as MDQE_STREAM_TOUCH=1: copy, frame, tracker are touched inside `_make_streams`, right when the streams are
        # created and BEFORE the work stream's own first use (touching them behind it measured no better than not touching at all)
        self._touch_on_create = True
        try:
            with self._on_device(), self.work_stream():
                pass
        finally:
            self._touch_on_create = False

    @contextlib.contextmanager
    def work_stream(self):
        """The model's own HIGH-PRIORITY stream for the per-clip stages (decoder, inference_clip: hundreds of small kernels
        and three host syncs per pass).  Their blocks are then dispatched ahead of the queued blocks of the frame stream's
        large GEMMs instead of waiting for whole waves of them to drain: +4-7 % frames/s (tools/prio_ab.py; the opposite,
        a high-priority frame stream, costs 7 %).  Entering makes it wait for the caller's stream (the inputs), leaving makes
        the caller's stream wait for it (device-side outputs); re-entrant; a no-op on CPU or with MDQE_CLIP_PRIORITY=0."""
        if self.device.type != "cuda" or not self.clip_priority:
            yield
            return
        cur = torch.cuda.current_stream(self.device)
        if self._work_stream is None:
            self._work_stream = torch.cuda.Stream(self.device, priority=-1)
            self._make_streams()
        ws = self._work_stream
        if cur == ws:
            yield
            return
        ws.wait_stream(cur)
        try:
            with torch.cuda.stream(ws):
                yield
        finally:
            cur.wait_stream(ws)

    @property
    def label_output(self):
        return self.__dict__.get("_label_output", False)

    @label_output.setter
    def label_output(self, value):
        if value not in (False, True, "only"):
            raise ValueError("label_output must be False, True or 'only', got %r" % (value,))
        if value:
            self.check_label_capacity()
        self.__dict__["_label_output"] = value

    @property
    def overlay_output(self):
        return self.__dict__.get("_overlay_output", False)

    @overlay_output.setter
    def overlay_output(self, value):
        if value is not False and value is not True and not (isinstance(value, str) and value == "surface"):
            raise ValueError("overlay_output must be False, True or 'surface', got %r" % (value,))
        if value:
            self.check_label_capacity()
        self.__dict__["_overlay_output"] = value

    @property
    def crop_output(self):
        """None, or a render.Crops: forward() on a video adds "pred_crops" (uint8 [n_out, Lc, Sh, Sw, 3], pinned host: per output and
        taken frame one fixed-size picture cut from the frames handed in -- with resize_on_device the original-size frames -- along the
        track's visible region of the label map and resized on the device, ops.track_crops), "pred_crop_rects" (int32 [n_out, Lc, 4],
        the source rects (X0, Y0, X1, Y1) in output pixels; (0, 0, -1, -1) beside a chip of `fill` where the track has no region),
        "pred_crop_frames" (the Lc = ceil(L / every) video frames taken) and "pred_track_ids".  Beside every other output form.  The
        video's chips wait on the device, n_tracks * Lc * Sh * Sw * 3 bytes, for one read-back at the end.  Videos only, one device
        (sharding.py refuses it).  None: nothing changes."""
        return self.__dict__.get("_crop_output", None)

    @crop_output.setter
    def crop_output(self, value):
        from .render import Crops
        if value is not None and not isinstance(value, Crops):
            raise ValueError("crop_output must be None or a render.Crops, got %r" % (value,))
        if value is not None:
            self.check_label_capacity()
        self.__dict__["_crop_output"] = value

    @property
    def matte_output(self):
        """None, or a render.Matte: forward() on a video adds "pred_matte" (uint8 [L, Ho, Wo], pinned host: per frame the soft matte of
        the window's tracks -- of the spec's classes, by the window's class rows -- rint(255 * sigmoid(gain * the largest up-sampled
        logit)), >= 128 exactly on the union of their final masks, ops.final_matte) and "pred_track_ids".  Beside every other output
        form, on both mask paths; the bits of the other outputs are left alone.  Videos only, one device (sharding.py refuses it).
        None: nothing changes."""
        return self.__dict__.get("_matte_output", None)

    @matte_output.setter
    def matte_output(self, value):
        from .render import Matte
        if value is not None and not isinstance(value, Matte):
            raise ValueError("matte_output must be None or a render.Matte, got %r" % (value,))
        if value is not None:
            self.check_label_capacity()
        self.__dict__["_matte_output"] = value

    @property
    def path_output(self):
        """False or True: forward() on a video adds "pred_centroids" (int32 [n_out, L, 2]: per output and frame the centroid (x, y) of
        the track's visible region of the label map, ((SX + m/2) / m, (SY + m/2) / m) in integers, ops.label_centroids; (-1, -1) where
        the track has no region, the frames before its first window included), "pred_moments" (int64 [n_out, L, 3]: that region's
        pixels m and the sums SX, SY of their coordinates) and "pred_track_ids".  Beside every other output form, on either mask path;
        the label map is then made whether or not it is returned.  Videos only, one device (sharding.py refuses it)."""
        return self.__dict__.get("_path_output", False)

    @path_output.setter
    def path_output(self, value):
        if not isinstance(value, bool):
            raise ValueError("path_output must be False or True, got %r" % (value,))
        if value:
            self.check_label_capacity()
        self.__dict__["_path_output"] = value

    @property
    def polygon_output(self):
        """None, or a polygons.Polygons: forward() on a video adds "pred_polygons" (a polygons.TrackPolygons on the host: per output
        and taken frame the closed rings of lattice corners around the track's visible region of the label map, holes flagged --
        include/mdqe_hip.h's rule, traced on the device by ops.label_polygons window by window, a few KB each; row k of a ring is
        output k of "pred_track_ids", and a track behind several outputs has its rings under the first) and "pred_track_ids".  Beside
        every other output form, on either mask path; the label map is then made whether or not it is returned, and the bits of the
        other outputs are left alone.  Videos only, one device (sharding.py refuses it).  None: nothing changes."""
        return self.__dict__.get("_polygon_output", None)

    @polygon_output.setter
    def polygon_output(self, value):
        from .polygons import Polygons
        if value is not None and not isinstance(value, Polygons):
            raise ValueError("polygon_output must be None or a polygons.Polygons, got %r" % (value,))
        if value is not None:
            self.check_label_capacity()
        self.__dict__["_polygon_output"] = value

    @property
    def occlusion_output(self):
        """False or True: forward() on a video adds "pred_occlusion" (int32 [n_out, L, n_out + 1], host: entry [a, f, b] with b < n_out is
        the number of pixels of output a's final mask in frame f that output b's track owns -- b == a: a's visible region, b != a: the
        part of a that b hides -- and the last column the pixels owned by tracks that are not among the outputs, so a row sums to the
        area of a's mask; the owner is the label map's, ops.final_occlusion; zero in the frames before the track's first window) and
        "pred_track_ids", the order of its rows and columns.  Beside every other output form, on either mask path; no label map is made
        for it and the bits of the other outputs are left alone.  Helpers on the table: occlusion.py.  Videos only, one device
        (sharding.py refuses it)."""
        return self.__dict__.get("_occlusion_output", False)

    @occlusion_output.setter
    def occlusion_output(self, value):
        if not isinstance(value, bool):
            raise ValueError("occlusion_output must be False or True, got %r" % (value,))
        if value:
            self.check_occlusion_capacity()
        self.__dict__["_occlusion_output"] = value

    @property
    def overlay_style(self):
        if "_overlay_style" not in self.__dict__:
            from .render import Style
            self.__dict__["_overlay_style"] = Style()
        return self.__dict__["_overlay_style"]

    @overlay_style.setter
    def overlay_style(self, value):
        from .render import Style
        if not isinstance(value, Style):
            raise ValueError("overlay_style must be a render.Style, got %r" % (value,))
        self.__dict__["_overlay_style"] = value

    def check_label_capacity(self):
        """uint8 labels are tracker row + 1: the bank may hold at most 255 rows."""
        if int(self.cfg.n_max_inst) > 255:
            raise ValueError("label maps are uint8 (label = track + 1): n_max_inst (MODEL.MDQE.MAX_NUM_INSTANCES) = %d exceeds 255"
                             % int(self.cfg.n_max_inst))

    def check_occlusion_capacity(self):
        """The occlusion sweep keeps a pixel's owner among at most 255 rows, as the label map does."""
        if int(self.cfg.n_max_inst) > 255:
            raise ValueError("the occlusion table takes at most 255 tracker rows: n_max_inst (MODEL.MDQE.MAX_NUM_INSTANCES) = %d exceeds "
                             "255; lower it to 255 or less" % int(self.cfg.n_max_inst))

    PIN_POOL_GB = float(os.environ.get("MDQE_PIN_POOL_GB", "8"))       # pinned host memory the model keeps for mask read-back between calls

    def pinned_mask_buffer(self, shape):
        """A pinned uint8 host buffer for one track's final masks.  A video's result hands VIEWS of these buffers to the caller, so a
        buffer is free again when the caller has dropped that result: the pool keeps the buffers it has made (up to PIN_POOL_GB) and
        re-issues one as soon as nothing but the pool references its storage.  A fresh pinned allocation costs ~75 us per MB (7 tracks of a
        960-frame 360p video: 120 ms; tools/pinned_probe.py), and the framework's own host allocator recycles only every other video."""
        pool = self.__dict__.setdefault("_pin_pool", {})
        free = pool.setdefault(tuple(shape), [])
        # What is handed out is a VIEW (its own tensor object on the pooled storage): the storage's use count then stays above the pool's
        # own for as long as a merger, or a result the caller still holds, references the buffer -- the pool's tensor itself is never
        # given away (two Python references to ONE tensor object count once, and a second track of the same video would get the same
        # buffer: tests/test_fullsize_gpu.py caught exactly that).
        use_count, idle = self._pin_pool_probe()
        if use_count is not None:
            for t in free:
                if use_count(t.untyped_storage()._cdata) == idle:      # exactly what an unshared pooled buffer shows (calibrated, not assumed)
                    return t[:]         # (every frame row is rewritten by the windows' read-backs before the result is handed out)
        t = torch.empty(tuple(shape), dtype=torch.uint8, pin_memory=True)
        held = sum(b.numel() for bufs in pool.values() for b in bufs)
        if use_count is not None and held + t.numel() <= self.PIN_POOL_GB * 2 ** 30:
            free.append(t)
            return t[:]
        return t

    _PIN_PROBE = None

    @classmethod
    def _pin_pool_probe(cls):
        """(use-count accessor, the count an UNSHARED pooled buffer shows) or (None, None): pooling off.  The accessor is a private torch
        call whose baseline depends on the torch version's storage wrapper handling, so it is CALIBRATED once per process on a scratch
        tensor -- the count with only the owner alive, and that a view raises it by exactly one and dropping the view restores it -- instead
        of assumed; if the self-check fails the pool is disabled (fresh pinned buffers per call: slower, never wrong)."""
        if cls._PIN_PROBE is None:
            fn = getattr(torch._C, "_storage_Use_Count", None)
            probe = (None, None)
            if fn is not None:
                try:
                    t = torch.empty(16, dtype=torch.uint8)
                    idle = fn(t.untyped_storage()._cdata)
                    v = t[:]
                    shared = fn(t.untyped_storage()._cdata)
                    del v
                    if shared == idle + 1 and fn(t.untyped_storage()._cdata) == idle:
                        probe = (fn, idle)
                except Exception:
                    pass
            cls._PIN_PROBE = probe
        return cls._PIN_PROBE

    def _on_device(self):
        """Every ctypes launch goes to the CURRENT device's current stream: make the model's device current for the call."""
        return torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    @torch.no_grad()
    def forward(self, batched_inputs):
        if len(batched_inputs) != 1:
            raise RuntimeError("MDQE eval takes exactly one video per call (mdqe/mdqe.py:292)")
        with self._on_device(), torch.autocast(device_type="cuda", enabled=False), self.work_stream():   # neutralise ambient autocast
            if self.cfg.is_coco:                                           # DATASETS.TEST[0] is a COCO set (mdqe/mdqe.py:213,233-236)
                return self.inference_image(batched_inputs)
            return self.inference_vis(batched_inputs)

    def alloc_cache(self, frames, geo, keep_enc=False):
        """An empty frame cache for `frames` frames: name -> [frames, ...] device buffer (engine.cache_shapes)."""
        return {k: torch.empty((int(frames),) + tuple(sh), dtype=torch.float32, device=self.device)
                for k, sh in self.engine.cache_shapes(geo, keep_enc).items()}

    def _frame_cache(self, frames, geo, ring=None, at=0, keep_enc=False, dec_ready=None):
        """Per-frame stages a1-a11 for a batch of frames: everything a clip needs, computed once, stored IN PLACE into rows
        [at, at+n) of the frame cache `ring` (name -> [capacity, ...] buffer; None: a cache of exactly these frames is allocated and
        returned) -- the 63 MB/frame decoder value cache by its GEMM, the mask features by the mask head's last product, the query
        coordinates / contents / embeddings by their kernels: no device-to-device copy of any result (round 5; rounds 2-4 copied the
        mask features and the small tensors into the ring and carried T-1 frames from ring to ring).  keep_enc: the encoder tokens go
        into the cache too (5.2 MB per frame; a sharded video ships the tokens of a chunk's last T-1 frames to the neighbour,
        sharding._Halo).
        Order (round 4): what the DECODER reads -- query selection / content / embeddings and the value projections -- comes first and
        `dec_ready` (an event) is recorded behind it; the mask-feature head, which only `inference_clip` reads, runs after.  The decoder
        of a group can then start while the mask head of its last frame pass is still running: at the end of a video that pass has
        nothing else to overlap with, and the decoder's chain of small dependent launches is latency-bound."""
        eng = self.engine
        n = frames.shape[0]
        ret = ring is None
        if ring is None:
            ring, at = self.alloc_cache(n, geo, keep_enc), 0
        feats = eng.backbone(frames, geo)
        enc = eng.encode(feats, geo)
        del feats
        eng.frame_queries(enc, geo, out=(ring["coords"][at:at + n], ring["content"][at:at + n], ring["emb"][at:at + n]))
        eng.dec_values(enc, geo, out=ring["vals"][at:at + n])
        if "enc" in ring:
            ring["enc"][at:at + n].copy_(enc)
        if dec_ready is not None:
            dec_ready.record(torch.cuda.current_stream(self.device))
        eng.mask_features(enc, geo, out=ring["mf"][at:at + n])
        return ring if ret else None

    def _cache_from_tokens(self, enc, mf, geo, ring, at):
        """Cache entries of frames whose encoder tokens and mask features were computed elsewhere (a neighbour rank's halo):
        only query selection / content sampling and the decoder value projections are redone here."""
        eng = self.engine
        n = enc.shape[0]
        eng.frame_queries(enc, geo, out=(ring["coords"][at:at + n], ring["content"][at:at + n], ring["emb"][at:at + n]))
        eng.dec_values(enc, geo, out=ring["vals"][at:at + n])
        ring["mf"][at:at + n].copy_(mf)
        if "enc" in ring:
            ring["enc"][at:at + n].copy_(enc)

    pass_bounds = staticmethod(schedule.pass_bounds)

    @staticmethod
    def stacked_view(imgs):
        """A list of per-frame host tensors that are consecutive views of ONE buffer (a loader that decoded into one block,
        `list(video)` of a stacked tensor) as a single [L, ...] view of that buffer, else None."""
        f0 = imgs[0]
        if f0.is_cuda or not f0.is_contiguous() or len(imgs) < 2:
            return None
        nb = f0.numel() * f0.element_size()
        if not all(f.dtype == f0.dtype and f.shape == f0.shape and f.is_contiguous() and f.data_ptr() == f0.data_ptr() + i * nb
                   for i, f in enumerate(imgs)):
            return None
        try:                                               # (as_strided checks the storage bounds)
            return f0.as_strided((len(imgs),) + tuple(f0.shape), (f0.numel(),) + tuple(f0.stride()))
        except RuntimeError:
            return None

    clip_schedule = staticmethod(schedule.clip_schedule)

    CACHE_GB = float(os.environ.get("MDQE_CACHE_GB", "24"))       # HBM budget of ONE frame-cache buffer (a long video uses two)

    def iter_clip_results(self, frames_dev, clips, frame_offset=0, trace=None, primed=False, on_frames_queued=None, h2d=None,
                          halo=None, side_streams=True, prime_all=True, split_small=False, carry=None):
        """Per-frame features (computed once, streamed in passes of `frame_batch` frames) + decoder + inference_clip for
        `clips` (global frame indices; frames_dev[0] is global frame `frame_offset`).  Yields (start, end, last, res).

        carry (online video, online._Carry): the cache rows of the `carry.rows` frames in front of this chunk, computed by earlier
        calls, go into the rows in front of its first frame (`carry.head`), so a clip may start anywhere in them -- a 1-frame push
        owns only such straddling clips.  The chunk's frames from global frame `carry.tail_from` on (what later calls' clips read)
        go through the per-frame stages even if no clip here reads them, and their rows are handed to `carry.on_tail`.
        `carry.rows` / `tail_from` / `tail_sent` and `halo.tail_sent` are sampled ONCE, when the generator starts (they go into the
        plan); afterwards only the generator's own `on_tail` call is taken to change them.

        Two HIP streams: the per-frame stages (backbone .. decoder value cache: large GEMMs) of the next passes run on a frame
        stream while the decoder + inference_clip of group k (small kernels and two host syncs) run on the caller's
        stream, so the matrix cores stay fed through the data-dependent part.

        The frame cache (round 5) is ONE linear buffer per kind, row = frame: every pass stores its results in place at the rows of its
        frames (`_frame_cache`) and a group of clips reads them through index tables (`starts`), so nothing is copied from buffer to
        buffer -- no carried T-1 frames, no first fill -- and the decoder batch is free of the pass size (`dec_batch`).  A video
        longer than the cache budget (MDQE_CACHE_GB per buffer, 24 GB = 360 frames at 360p) continues in a second buffer, to which the
        frames still to be read are copied once per segment; the buffers then alternate, events order their reuse.

        WHAT is issued and in which order is decided in schedule.py, over integers alone (`schedule.plan_steps`); this generator
        resolves the parameters, pulls the plan one step at a time and has a `_ClipIssuer` issue it."""
        eng = self.engine
        geo = eng.geometry(int(frames_dev.shape[-2]), int(frames_dev.shape[-1]))
        fbatch = self.frame_batch if self.frame_batch > 0 else max(8, min(40, 306000 // max(geo.N, 1)))
        # cache capacity (frames): the whole chunk if the budget allows, else segments in two alternating buffers (schedule.cache_capacity)
        per_frame = 4 * sum(int(np.prod(sh)) for sh in eng.cache_shapes(geo, keep_enc=halo is not None).values())
        chunk = schedule.resolve(clips, frame_offset, frames_dev.shape[0], self.cfg.n_frames_test, fbatch, self.dec_batch, self.lookahead,
                                 self.taper_passes, self.taper_tail, split_small, per_frame, self.CACHE_GB,
                                 halo=halo is not None, halo_tail_sent=halo is not None and halo.tail_sent, carry=carry is not None,
                                 carry_rows=carry.rows if carry is not None else 0,
                                 carry_tail_from=carry.tail_from if carry is not None else 0,
                                 carry_tail_sent=carry is not None and carry.tail_sent)
        issuer = _ClipIssuer(self, frames_dev, geo, chunk, trace, on_frames_queued, h2d, halo, carry, side_streams)
        # `lookahead` groups' passes are queued BEFORE a group's clip work (the plan's order): with one, the frame stream ran dry at
        # every group boundary -- the clip kernels share the chip with the pass queued behind them and finish together with it, and
        # the next pass was only queued after the host had consumed the group (2-3 ms of whole-GPU idle per boundary in
        # the HIP trace, tools/trace_gaps.py)
        for step in schedule.plan_steps(chunk):
            consume = type(step) is schedule.Consume
            if not consume:
                issuer.ISSUE[type(step)](issuer, step)
            if primed and (consume or (not prime_all and type(step) is schedule.Group)):
                # a primed generator (sharded videos) is resumed only after the caller has gathered the previous round -- host syncs,
                # collectives: the frame stream gets its whole look-ahead now so that it does not run dry meanwhile.  prime_all=False
                # (forward_stream): only the first pass -- the host has the previous video's last decoder batch to launch right now, and
                # three passes of launches (13 ms of host time) in front of it cost more than they hide
                primed = False
                yield None                        # per-frame work of the first passes is queued; the caller resumes later
            if consume:
                issuer.consuming = True          # from here on the caller has gathered the previous round: the exchange may be issued
                yield from issuer.consume(step)
        if primed:
            yield None                            # (no clip to plan: nothing, or only the carry's tail, is queued)
        issuer.finish()

    def merge_clips(self, results, frame_hw, out_size, mask_hw, n_frames=None, frame_source=None, ground_truth=None):
        """Tracker + window flushes + video merge (mdqe/mdqe.py:337-366) over clip results in global order.  frame_source: the video's
        frames as handed in (merge.FrameStore), what `overlay_output` paints on.  ground_truth: the video's vis_score.GroundTruth or None
        (`_ground_truth`): the final masks are counted against it, "pred_gt"."""
        m = ClipMerger(self, frame_hw, out_size, mask_hw, n_frames, frame_source=frame_source, ground_truth=ground_truth)
        m.feed_batches(results)
        return m.finish()

    H2D_CHUNK = 10                                  # frames per host->device copy (one event each)

    def upload_frames(self, imgs):
        """a1's host->device step (mdqe/mdqe.py:473-484 copies every frame inside the call): frames that arrive in host
        memory go to ONE device buffer in chunks of a few frames on the model's copy stream, an event per chunk; the
        per-frame stages wait only for the chunks they read, so the upload of the rest of the video runs under the first
        pass (asynchronous when the frames are pinned; pageable frames are staged by the runtime).  A list whose tensors are
        consecutive views of one buffer (a loader that decoded into one block) is copied chunk-wise too.
        Returns (frames [L,3,h,w] on the device, [(end_frame, event), ...] or None when nothing is in flight)."""
        if torch.is_tensor(imgs):
            stack = imgs
        else:
            imgs = list(imgs)
            if len(imgs) == 0:
                raise RuntimeError("MDQE: a video needs at least one frame")
            f0 = imgs[0]
            stack = self.stacked_view(imgs)
            if stack is None and f0.is_cuda:
                stack = torch.stack(imgs)
        if self.device.type != "cuda" and stack is None:
            stack = torch.stack(imgs)
        if stack is not None and (stack.is_cuda or self.device.type != "cuda"):
            if stack.dtype not in (torch.uint8, torch.float32):
                stack = stack.float()
            return stack.to(self.device).contiguous(), None
        # host frames -> device, chunked on the copy stream
        first = stack[0] if stack is not None else imgs[0]
        L = stack.shape[0] if stack is not None else len(imgs)
        dt = first.dtype if first.dtype in (torch.uint8, torch.float32) else torch.float32
        dev = torch.empty((L,) + tuple(first.shape), dtype=dt, device=self.device)
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.device)
        cs = self._copy_stream
        cs.wait_stream(torch.cuda.current_stream(self.device))     # (the buffer may be a recycled block still read upstream)
        dev.record_stream(cs)
        events = []
        with torch.cuda.stream(cs):
            for a in range(0, L, self.H2D_CHUNK):
                b = min(L, a + self.H2D_CHUNK)
                if stack is not None:
                    dev[a:b].copy_(stack[a:b], non_blocking=True)
                else:
                    for i in range(a, b):
                        dev[i].copy_(imgs[i], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(cs)
                events.append((b, ev))
        return dev, events

    def convert_surfaces(self, yuv, keep=False):
        """Decoder surfaces (preprocess.YuvFrames) -> uint8 [n, 3, height, width] on the model's device, visible to the current stream.
        Host planes go up as they are -- the rows the picture uses at their pitch: for NV12 at a tight pitch half an RGB upload -- on the copy
        stream; the current stream waits for them and converts (preprocess.yuv_to_rgb: one launch).  keep: -> (that tensor, the
        surfaces on the device -- what a surface overlay paints on --, whether an upload made them: else they are the caller's planes)."""
        from .preprocess import yuv_to_rgb
        if len(yuv) == 0:
            raise RuntimeError("MDQE: a video needs at least one frame")
        if self.device.type != "cuda":
            rgb = yuv_to_rgb(yuv).to(self.device)
            return (rgb, yuv, False) if keep else rgb
        uploaded = yuv.device != self.device
        if not yuv.y.is_cuda:
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(self.device)
            cs, cur = self._copy_stream, torch.cuda.current_stream(self.device)
            with torch.cuda.stream(cs):
                yuv = yuv.to(self.device, non_blocking=True)
            for t in (yuv.y, yuv.uv):                              # allocated under the copy stream, read by the kernel on this one
                t.record_stream(cur)
            cur.wait_stream(cs)
        elif yuv.device != self.device:
            yuv = yuv.to(self.device)
        return (yuv_to_rgb(yuv), yuv, uploaded) if keep else yuv_to_rgb(yuv)

    def to_device_frames(self, imgs):
        """All frames on the device, visible to the current stream."""
        dev, events = self.upload_frames(imgs)
        if events:
            torch.cuda.current_stream(self.device).wait_event(events[-1][1])
        return dev

    def _frames_for(self, video):
        """(frames on the device, upload events, original (h0, w0)) of one input dict; the optional device-side resize
        (the mapper's eval augmentation) needs the whole upload."""
        return self._frames_and_source(video)[:4]

    def _frames_and_source(self, video, surface=None):
        """`_frames_for` and, behind it, the frames as uploaded -- before the device-side resize, what an overlay is painted on -- with
        the event behind their upload (None: nothing was in flight) and whether an upload made them (else they may be the caller's tensor).
        surface (None: overlay_output == "surface"): the source of decoder surfaces is the surfaces themselves on the device, not the
        converted frames (those are then nobody's to keep once the per-frame stages have read them)."""
        from .preprocess import YuvFrames
        if surface is None:
            surface = self.overlay_output == "surface"
        if isinstance(video["image"], YuvFrames) and surface:
            frames_dev, src, uploaded = self.convert_surfaces(video["image"], keep=True)
            h2d = src_ready = None
        elif isinstance(video["image"], YuvFrames):
            # decoder surfaces: from here the converted tensor is what an uploaded uint8 RGB tensor would have been (and the model's own)
            frames_dev, h2d = self.convert_surfaces(video["image"]), None
            src, src_ready, uploaded = frames_dev, None, True
        else:
            frames_dev, h2d = self.upload_frames(video["image"])
            src, src_ready, uploaded = frames_dev, (h2d[-1][1] if h2d else None), bool(h2d)
        h0, w0 = int(frames_dev.shape[-2]), int(frames_dev.shape[-1])
        if self.resize_on_device and frames_dev.dtype == torch.uint8:
            from .preprocess import resize_shortest_edge
            if h2d:
                torch.cuda.current_stream(self.device).wait_event(h2d[-1][1])
                h2d = None
            frames_dev = resize_shortest_edge(frames_dev, self.cfg.min_size_test, self.cfg.max_size_test)
        return frames_dev, h2d, h0, w0, src, src_ready, uploaded

    @staticmethod
    def _ground_truth(video, out_size=None, n_frames=None):
        """The "ground_truth" of an input dict (a vis_score.GroundTruth; the video is then scored against it: res["pred_gt"]) or None,
        checked against the output size and the video's length where given."""
        gt = video.get("ground_truth")
        if gt is None:
            return None
        from .vis_score import GroundTruth
        if not isinstance(gt, GroundTruth):
            raise ValueError("ground_truth must be a vis_score.GroundTruth, got %s" % type(gt).__name__)
        if out_size is not None and tuple(gt.size) != (int(out_size[0]), int(out_size[1])):
            raise ValueError("ground_truth: its size %s is not the output size (height, width) = %s" % (tuple(gt.size), (int(out_size[0]), int(out_size[1]))))
        if n_frames is not None and gt.length != int(n_frames):
            raise ValueError("ground_truth: it holds %d frames, the video %d" % (gt.length, int(n_frames)))
        return gt

    def _frame_source(self, src, src_ready, out_size=None):
        """The whole video as the frame source of an overlay or of crops (merge.FrameStore), or None with both off.  overlay_output =
        "surface": refused here, before anything of the video runs, for RGB frames and for an output size that is not the surfaces'."""
        if not self.overlay_output and self.crop_output is None:
            return None
        store = merge.FrameStore()
        store.add(0, src, src_ready)
        if self.overlay_output == "surface":
            merge.surface_kind(store, out_size)
        return store

    def inference_vis(self, batched_inputs, trace=None):
        """mdqe/mdqe.py:291-366 with the compute-once schedule (same clips, same flush points)."""
        cfg = self.cfg
        video = batched_inputs[0]
        frames_dev, h2d, h0, w0, src, src_ready, _ = self._frames_and_source(video)
        L, h, w = frames_dev.shape[0], int(frames_dev.shape[-2]), int(frames_dev.shape[-1])
        out_size = (video.get("height", h0), video.get("width", w0))       # the mapper reports the ORIGINAL size as height/width
        geo = self.engine.geometry(h, w)
        ms = cfg.match_stride
        clips = self.clip_schedule(L, cfg.n_frames_test, cfg.clip_stride)
        gt = self._ground_truth(video, out_size, L)
        return self.merge_clips(self.iter_clip_results(frames_dev, clips, 0, trace, h2d=h2d), (h, w), out_size,
                                (geo.Hp // ms, geo.Wp // ms), n_frames=L, frame_source=self._frame_source(src, src_ready, out_size), ground_truth=gt)

    def forward_stream(self, batches):
        """An eval loop over videos: yields `forward(b)` for every b of the iterable `batches`, in order, bit-identical to
        separate calls -- but with one video of look-ahead: as soon as the last frame of video k is on the frame stream,
        the first pass of the per-frame stages of video k+1 is queued behind it, so it runs under video k's last decoder
        batch, tracker updates and mask read-back instead of after them (the chip is half idle there).  The reference's
        evaluator (`inference_on_dataset`) hands videos over one by one; this is that loop with the hand-over moved
        forward.  COCO image sets and CPU runs fall back to plain calls."""
        it = iter(batches)

        def start(b):
            """Frames to the device, geometry, clip schedule; queues the first pass (the generator is primed)."""
            if len(b) != 1:
                raise RuntimeError("MDQE eval takes exactly one video per call (mdqe/mdqe.py:292)")
            cfg = self.cfg
            video = b[0]
            frames_dev, h2d, h0, w0, src, src_ready, _ = self._frames_and_source(video)
            L, h, w = frames_dev.shape[0], int(frames_dev.shape[-2]), int(frames_dev.shape[-1])
            st = {"done_frames": False, "out_size": (video.get("height", h0), video.get("width", w0)), "hw": (h, w), "L": L}
            st["source"] = self._frame_source(src, src_ready, st["out_size"])
            st["gt"] = self._ground_truth(video, st["out_size"], L)
            geo = self.engine.geometry(h, w)
            st["mask_hw"] = (geo.Hp // cfg.match_stride, geo.Wp // cfg.match_stride)
            clips = self.clip_schedule(L, cfg.n_frames_test, cfg.clip_stride)

            def cb():
                st["done_frames"] = True
                look_ahead(st)
            st["gen"] = self.iter_clip_results(frames_dev, clips, 0, None, primed=True, on_frames_queued=cb, h2d=h2d, prime_all=False)
            next(st["gen"])
            return st

        state = {"cur": None, "next": None}

        def look_ahead(st):
            # only the video being consumed may pull the next one in (a short video whose frames are all queued by its own
            # start() must not cascade through the whole stream)
            if st is state["cur"] and state["next"] is None:
                b = next(it, None)
                if b is not None:
                    try:
                        state["next"] = start(b)
                    except Exception as e:                 # belongs to the NEXT video: raised when its turn comes
                        state["next"] = {"error": e}

        first = next(it, None)
        if first is None:
            return
        if self.cfg.is_coco or self.device.type != "cuda":
            yield self.forward(first)
            for b in it:
                yield self.forward(b)
            return

        def guarded(fn):                                   # no context manager is held across a yield
            with self._on_device(), torch.autocast(device_type="cuda", enabled=False), torch.no_grad(), self.work_stream():
                return fn()

        def step():
            st = state["cur"]
            if "error" in st:
                state["cur"] = None
                raise st["error"]
            if st["done_frames"]:
                look_ahead(st)
            out = self.merge_clips(st["gen"], st["hw"], st["out_size"], st["mask_hw"], n_frames=st["L"], frame_source=st["source"],
                                   ground_truth=st["gt"])
            if state["next"] is None:
                look_ahead(st)                             # (the generator ends only after its callback; belt and braces)
            state["cur"], state["next"] = state["next"], None
            return out

        state["cur"] = guarded(lambda: start(first))
        while state["cur"] is not None:
            yield guarded(step)

    def online_video(self, height=None, width=None, emit="masks", keep=False, geometry=False, style=None, ground_truth=None,
                     surface=False, surface_pitch_align=1, crops=None, paths=False, matte=None, polygons=None, occlusion=False):
        """An online session over ONE video whose frames arrive in pushes (a camera, a stream, a video too long to hold): push()
        returns each tracker window as soon as it is final, close() the rest, result() the video-level scores / labels / tracks.
        height / width: output mask size (default: the frame size); emit: "masks" (bool [n, F, H, W] per window), "rle" or "labels" (one
        uint8 [F, H, W] map per window: which track owns each pixel, `label_output`'s rule) or "overlay" (that map and, painted from it
        over the frames pushed, one uint8 [F, H, W, 3] picture per window in `style`, a render.Style; `overlay_output`'s picture); keep:
        result() also carries forward()'s "pred_masks" / "pred_rles" / "pred_label_map" / "pred_overlay", bit-identical; geometry: every
        window carries `boxes` / `areas` of its final masks and result() "pred_boxes" / "pred_areas" (with or without keep), equal to
        forward()'s with geometry_output; ground_truth (vis_score.GroundTruth): result() carries "pred_gt", forward()'s with the input's
        "ground_truth" (a push past its length raises); surface (with emit="overlay", pushes of preprocess.YuvFrames): `win.overlay` is
        a YuvFrames of painted surfaces of the pushed format instead of RGB pixels (surface_pitch_align: its row pitch in bytes is
        rounded up to a multiple of it); crops (render.Crops, beside any emit): every window carries `crops` / `crop_rects` /
        `crop_frames`, one fixed-size picture per track and taken frame (`crop_output`'s); paths (a bool, beside any emit): every
        window carries `centroids` / `moments` of its tracks' visible regions and, with keep, result() "pred_centroids" /
        "pred_moments" (`path_output`'s); matte (render.Matte, beside any emit): every window carries `matte`, uint8 [F, H, W], the soft
        matte of its tracks, and with keep result() "pred_matte" (`matte_output`'s); polygons (polygons.Polygons, beside any emit): every
        window carries `polygons`, a polygons.TrackPolygons of its tracks' outlines, and with keep result() "pred_polygons"
        (`polygon_output`'s); occlusion (a bool, beside any emit): every window carries `occlusion`, int32 [n, F, n], the pixels of each
        track's mask that every track owns, and with keep result() "pred_occlusion" (`occlusion_output`'s).  See online.py."""
        from .online import OnlineVideo
        return OnlineVideo(self, height=height, width=width, emit=emit, keep=keep, geometry=geometry, style=style, ground_truth=ground_truth,
                           surface=surface, surface_pitch_align=surface_pitch_align, crops=crops, paths=paths, matte=matte,
                           polygons=polygons, occlusion=occlusion)

    def inference_image(self, batched_inputs):
        """COCO single-image branch: MDQE.forward :213-236 -> mdqe.forward (models/mdqe.py:62-70) -> decoder
        eval branch `is_coco` (transformer_dec.py:247-255) -> MDQE.inference_image (mdqe/mdqe.py:486-556).  The pseudo clip
        (cfg.n_frames images) goes through the same per-frame stages and decoder as a video clip; the centre frame's masks
        are scored, box-IoU-suppressed and resized by two kernels that evaluate aligned_bilinear in closed form.
        Returns [{"instances": Instances(scores, pred_classes, pred_masks, pred_boxes)}]."""
        from . import ops
        from .d2_compat import Boxes, Instances
        cfg, eng = self.cfg, self.engine
        item = batched_inputs[0]
        if item.get("ground_truth") is not None:
            raise ValueError("ground_truth: the COCO image branch is not scored (video IoU and the YTVIS table are for videos)")
        if getattr(self, "overlay_output", False) == "surface":
            raise ValueError("overlay_output = 'surface': the COCO image branch has no overlay (painted surfaces are a video output: use a "
                             "video config, or set overlay_output = False)")
        if getattr(self, "crop_output", None) is not None:
            raise ValueError("crop_output: the COCO image branch has no crops (per-track crops are a video output: use a video config, or "
                             "set crop_output = None)")
        if getattr(self, "matte_output", None) is not None:
            raise ValueError("matte_output: the COCO image branch has no matte (the soft matte is a video output: use a video config, or "
                             "set matte_output = None)")
        if getattr(self, "path_output", False):
            raise ValueError("path_output: the COCO image branch has no paths (track centroids are a video output: use a video config, or "
                             "set path_output = False)")
        if getattr(self, "polygon_output", None) is not None:
            raise ValueError("polygon_output: the COCO image branch has no polygons (track outlines are a video output: use a video config, "
                             "or set polygon_output = None)")
        if getattr(self, "occlusion_output", False):
            raise ValueError("occlusion_output: the COCO image branch has no occlusion table (the relation between tracks is a video "
                             "output: use a video config, or set occlusion_output = False)")
        from .preprocess import YuvFrames
        if isinstance(item["image"], YuvFrames):
            raise ValueError("YuvFrames: the COCO image branch takes RGB tensors (decoder surfaces are a video input; convert one with "
                             "preprocess.yuv_to_rgb)")
        frames = self.to_device_frames(item["image"])
        T, h, w = int(frames.shape[0]), int(frames.shape[-2]), int(frames.shape[-1])
        geo = eng.geometry(h, w)
        cache = self._frame_cache(frames, geo)
        out = eng.decode_clips(cache, [0], T, geo)
        cls, coef = out["cls"][0], out["mask_coeff"][0]                      # [Q,K] (sigmoid), [Q,M] (tanh)
        thr = cfg.apply_cls_thres
        score = cls.max(-1)[0]
        idx = torch.nonzero(score >= torch.clamp(score.max(), max=thr)).reshape(-1)       # :504
        ct = int((cfg.n_frames - 1) / 2)
        mf = cache["mf"][ct]                                                 # [Hm,Wm,M] channels-last
        Hm, Wm, Md = mf.shape
        lg = ops.linear(coef[idx].contiguous(), mf.reshape(-1, Md)).view(-1, Hm, Wm)     # einsum 'qm,mhw->qhw' of the centre frame
        st = ops.image_mask_stats(lg, cfg.match_stride, h, w)
        mc = cls[idx] * (st[:, 0] / (st[:, 1] + 1e-6))[:, None]             # mask-quality rescoring :512-516
        n = int(idx.numel())
        order = torch.arange(n, device=self.device)
        if n > 0:                                                            # box-IoU NMS :519-531
            order = mc.max(-1)[0].sort(descending=True)[1]
            mc, sb = mc[order], st[order]
            empty = sb[:, 2] > sb[:, 4]
            bx = torch.stack([sb[:, 2], sb[:, 3], sb[:, 4] + 1, sb[:, 5] + 1], 1)
            bx = torch.where(empty[:, None], torch.zeros_like(bx), bx) / torch.tensor([w, h, w, h], device=self.device, dtype=torch.float32)
            area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
            lt = torch.max(bx[:, None, :2], bx[None, :, :2])
            rb = torch.min(bx[:, None, 2:], bx[None, :, 2:])
            inter = (rb - lt).clamp(min=0).prod(-1)
            iou = inter / (area[:, None] + area[None] - inter).clamp(min=1e-3)
            mc = mc * (1 - torch.triu(iou, diagonal=1).max(0)[0])[:, None]
        if cfg.multi_cls:                                                    # :534-540
            ls = torch.nonzero(mc > thr)
            ii, label = ls[:, 0], ls[:, 1]
            sc = mc[ii, label]
        else:
            sc, label = mc.max(-1)
            ii = torch.arange(n, device=self.device)
        Ho, Wo = int(item.get("height", h)), int(item.get("width", w))
        sel = order[ii].to(torch.int32).contiguous()                         # rows of lg, in output order
        pm = ops.image_final_masks(lg, sel, cfg.match_stride, h, w, Ho, Wo).view(torch.bool)
        # BitMasks(mask).get_bounding_boxes() of the final masks :554
        xa, ya = pm.any(1), pm.any(2)
        has = xa.any(1)
        ar_x, ar_y = torch.arange(Wo, device=self.device), torch.arange(Ho, device=self.device)
        x0 = torch.where(xa, ar_x, Wo).min(1)[0]; x1 = torch.where(xa, ar_x, -1).max(1)[0] + 1
        y0 = torch.where(ya, ar_y, Ho).min(1)[0]; y1 = torch.where(ya, ar_y, -1).max(1)[0] + 1
        boxes = torch.stack([x0, y0, x1, y1], 1).float() * has[:, None]
        res = Instances((Ho, Wo))
        res.scores, res.pred_classes, res.pred_masks, res.pred_boxes = sc, label, pm, Boxes(boxes)
        return [{"instances": res}]

    def select_tracks(self, cls_clips):
        """merge.select_tracks: (scores [k] host tensor, labels, track index of each output) of the video's top-k."""
        self.last_num_tracks = int(cls_clips[-1].shape[0])     # tracks of the video just merged (diagnostics; bench.py reports it)
        return merge.select_tracks(cls_clips, self.cfg.num_classes)

    track_geometry = staticmethod(merge.track_geometry)

    def inference_video(self, image_size, cls_clips, windows, frame_hw, n_frames, **kw):
        """mdqe/mdqe.py:430-471: the video's result from its flushed windows (merge.video_result, its keywords)."""
        return merge.video_result(self, image_size, cls_clips, windows, frame_hw, n_frames, **kw)


class MDQE_MI355X(MDQE):
    """The same model under a name of its own: `MODEL.META_ARCHITECTURE MDQE_MI355X` on the reference's command line selects this
    implementation whatever else is registered as "MDQE"."""


_REGISTRATION = {"state": "detectron2 not imported"}


def register_with_detectron2(registry=None, takeover=None):
    """Put this implementation into detectron2's `META_ARCH_REGISTRY` BESIDE the reference's `mdqe` package.

    The reference registers its own torch model under the name "MDQE" the moment `mdqe` is imported (`mdqe/__init__.py:3` ->
    `@META_ARCH_REGISTRY.register()` at `mdqe/mdqe.py:60-61`), and `train_net.py:40-43` / `demo/demo.py:16` import `mdqe` for
    `add_mdqe_config` and the data loaders; fvcore's `Registry` asserts on a second registration of a name.  So:

    * the alias `MDQE_MI355X` is always registered (no collision possible);
    * the name "MDQE" -- what every config of the reference selects (`configs/*.yaml: META_ARCHITECTURE: "MDQE"`) -- is TAKEN OVER
      (`takeover=True`, the default; `MDQE_MI355X_REGISTER=alias` in the environment turns it off): a reference model registered earlier
      is moved to "MDQE_REFERENCE" and this class takes its slot, with a warning in the log; a registration of another "MDQE" that
      comes LATER (this package imported before the reference's) is diverted to "MDQE_REFERENCE" instead of tripping fvcore's
      assertion.  Both import orders end with `build_model(cfg)` constructing this class and the reference's model still selectable.

    Returns a dict describing what was done (also kept in `registration_state()`).  A missing detectron2 is silent; a detectron2 that
    is installed but fails to import (ImportError / OSError) is a logged warning recorded in `registration_state()` -- the d2-free
    `MDQE(cfg)` keeps working -- unless `MDQE_MI355X_REGISTER=strict`; a failure of the registration itself propagates."""
    import logging
    log = logging.getLogger("mdqe_cvpr2023_amd")
    if registry is None:
        try:
            from detectron2.modeling import META_ARCH_REGISTRY as registry
        except (ImportError, OSError) as e:
            # ModuleNotFoundError of detectron2 itself: absent in this image, the d2-free entry points are all there is (silent).
            # Any other ImportError / OSError: a detectron2 that is installed but does not import here -- typically `from detectron2
            # import _C` on a ROCm box without its compiled ops.  That must not take the d2-free `MDQE(cfg)` entry point down with it:
            # warn, record, go on.  `MDQE_MI355X_REGISTER=strict` raises instead.  (A failure of the REGISTRATION below -- a registry
            # that misbehaves -- still propagates.)
            absent = isinstance(e, ModuleNotFoundError) and (e.name or "").split(".")[0] == "detectron2"
            if not absent:
                if os.environ.get("MDQE_MI355X_REGISTER", "") == "strict":
                    raise
                log.warning("detectron2 is installed but `detectron2.modeling` does not import (%s: %s): mdqe_cvpr2023_amd.MDQE is NOT in "
                            "META_ARCH_REGISTRY; the detectron2-free entry point MDQE(cfg) works (MDQE_MI355X_REGISTER=strict makes this "
                            "an error)", type(e).__name__, e)
            _REGISTRATION.clear()
            _REGISTRATION.update(state="detectron2 not importable" if absent else "detectron2 import failed",
                                 error=None if absent else "%s: %s" % (type(e).__name__, e))
            return dict(_REGISTRATION)
    if takeover is None:
        takeover = os.environ.get("MDQE_MI355X_REGISTER", "replace") != "alias"
    objs = registry._obj_map
    if objs.get("MDQE_MI355X") is not MDQE_MI355X:
        registry.register(MDQE_MI355X)            # (a foreign class of that name would assert here, as it should)
    done = {"state": "alias only", "alias": "MDQE_MI355X", "MDQE": None, "MDQE_REFERENCE": None}
    if takeover:
        prev = objs.get("MDQE")
        if prev is None:
            registry.register(MDQE)
        elif prev is not MDQE:
            objs["MDQE_REFERENCE"] = prev
            objs["MDQE"] = MDQE
            log.warning("META_ARCH_REGISTRY['MDQE'] now builds mdqe_cvpr2023_amd.meta_arch.MDQE (MI355X); the class registered before "
                        "(%s.%s) stays selectable as 'MDQE_REFERENCE'", getattr(prev, "__module__", "?"), getattr(prev, "__qualname__", "?"))
        if not getattr(registry, "_mdqe_mi355x_guard", False):
            inner = registry._do_register

            def _do_register(name, obj, _inner=inner, _objs=objs):
                if name == "MDQE" and _objs.get("MDQE") is MDQE and obj is not MDQE:
                    _objs["MDQE_REFERENCE"] = obj
                    log.warning("a second 'MDQE' (%s.%s) was registered after mdqe_cvpr2023_amd's: kept as 'MDQE_REFERENCE'; "
                                "'MDQE' keeps building the MI355X implementation", getattr(obj, "__module__", "?"), getattr(obj, "__qualname__", "?"))
                    return
                _inner(name, obj)
            registry._do_register = _do_register
            registry._mdqe_mi355x_guard = True
        done.update(state="MDQE taken over", MDQE="mdqe_cvpr2023_amd.meta_arch.MDQE")
    ref = objs.get("MDQE_REFERENCE")
    done["MDQE_REFERENCE"] = None if ref is None else "%s.%s" % (getattr(ref, "__module__", "?"), getattr(ref, "__qualname__", "?"))
    _REGISTRATION.clear()
    _REGISTRATION.update(done)
    return dict(done)


def registration_state():
    """What `register_with_detectron2` did at import (for logs and tests)."""
    return dict(_REGISTRATION)


def _register_backbone():
    """The Swin builder goes into BACKBONE_REGISTRY whenever the meta-architecture went into META_ARCH_REGISTRY (same policy)."""
    if _REGISTRATION.get("state") in ("MDQE taken over", "alias only"):
        from .backbone import register_backbone_with_detectron2
        try:
            from detectron2.modeling import BACKBONE_REGISTRY  # noqa: F401
        except (ImportError, OSError, AttributeError):
            return                                   # (a stand-in detectron2 without a backbone registry)
        register_backbone_with_detectron2()


register_with_detectron2()                        # silent without detectron2, a warning if it is there but does not import, loud otherwise
_register_backbone()
