"""Record what `MDQE.iter_clip_results` issues, in order, without a GPU: the golden trace of tests/test_schedule_plan_cpu.py.

    python tools/record_schedule_trace.py            # rewrites tests/golden/schedule_trace.json from the code as it stands

The generator runs on CPU tensors (its stream work is skipped) over a bare MDQE object whose seams are stand-ins that log their integer
arguments: `alloc_cache`, `_frame_cache`, `_cache_from_tokens`, the engine's `geometry` / `cache_shapes` / `decode_clips` /
`inference_clips`, a halo's `head` / `on_tail`, a carry's `head` / `on_tail` and `on_frames_queued`; every yield is logged too, the
`None` of a primed generator included.  The stand-in frame pass writes each frame's GLOBAL index into the cache rows it fills and the
stand-in decoder logs the values it finds at rows starts[k] .. starts[k]+T, so segment copies, carried heads and halo rows are checked
by content as well as by row number.  An exception ends a trace as ["error", type, text].
"""
import json
import os
import sys
import types

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "schedule_trace.json")

DEFAULTS = dict(L=23, T=4, stride=1, frame_batch=3, dec_batch=0, lookahead=2, cache_frames=0, cache_gb=None, taper=True, taper_tail=0,
                split_small=False, primed=False, prime_all=True, side_streams=True, kind="plain",
                offset=0, n_local=None, clips=None, carry_rows=0, tail_from=None, tail_sent=False)


def cfg(**kw):
    bad = set(kw) - set(DEFAULTS)
    assert not bad, bad
    return dict(DEFAULTS, **kw)


def configurations():
    """name -> configuration.  Together the traces hold every step kind and every integer-only error of the scheduler."""
    out = {}
    for L in (1, 3, 4, 5, 17, 23, 41, 120):
        out["len%d" % L] = cfg(L=L)
    out["len120_by_resolution"] = cfg(L=120, frame_batch=0)
    out["len120_fb40_db40"] = cfg(L=120, frame_batch=40, dec_batch=40)
    out["len41_fb6_db20"] = cfg(L=41, frame_batch=6, dec_batch=20)
    out["len41_fb2_db7_forced"] = cfg(L=41, frame_batch=2, dec_batch=7, cache_frames=1)
    out["len41_fb3_forced"] = cfg(L=41, frame_batch=3, cache_frames=1)
    out["len23_fb3_forced"] = cfg(L=23, frame_batch=3, cache_frames=1)
    out["len41_fb3_db1_forced_la1"] = cfg(L=41, frame_batch=3, dec_batch=1, cache_frames=1, lookahead=1)
    out["len41_fb6_forced_la3"] = cfg(L=41, frame_batch=6, cache_frames=1, lookahead=3)
    out["len41_fb3_cache_gb"] = cfg(L=41, frame_batch=3, cache_gb=60 * 12 / 2 ** 30)      # the budget in bytes: 60 frames, no segments
    out["len120_fb3_cache_gb"] = cfg(L=120, frame_batch=3, cache_gb=60 * 12 / 2 ** 30)    # ... and two buffers
    out["len23_la1"] = cfg(L=23, lookahead=1)
    out["len23_la3_db7"] = cfg(L=23, lookahead=3, dec_batch=7)
    out["len17_fb6_untapered"] = cfg(L=17, frame_batch=6, taper=False)
    out["len41_fb6_tail2"] = cfg(L=41, frame_batch=6, taper_tail=2)
    out["len23_fb40_split_small"] = cfg(L=23, frame_batch=40, split_small=True)
    out["len23_stride2"] = cfg(L=23, stride=2)
    out["len41_stride2_forced"] = cfg(L=41, stride=2, cache_frames=1)
    out["len23_T3_stride5"] = cfg(L=23, T=3, stride=5)
    out["len41_T3_stride5_fb2_forced"] = cfg(L=41, T=3, stride=5, frame_batch=2, cache_frames=1)
    out["len23_primed_all"] = cfg(L=23, primed=True)
    out["len23_primed_first"] = cfg(L=23, primed=True, prime_all=False)
    out["len3_primed_all"] = cfg(L=3, primed=True)
    out["len41_primed_all_forced"] = cfg(L=41, primed=True, cache_frames=1, side_streams=False)
    # ---- halo exchange: the chunk [offset, offset + n_local) of a longer video
    out["halo_first_chunk"] = cfg(kind="halo", L=40, offset=0, n_local=20, clips=[(s, s + 4, False) for s in range(0, 17)])
    out["halo_straddling"] = cfg(kind="halo", L=40, offset=20, n_local=20, clips=[(s, s + 4, False) for s in range(17, 37)] + [(37, 40, True)])
    out["halo_straddling_primed"] = cfg(kind="halo", L=40, offset=20, n_local=9, frame_batch=40, primed=True, side_streams=False,
                                        clips=[(s, s + 4, False) for s in range(17, 26)])
    out["halo_straddling_db7_split"] = cfg(kind="halo", L=60, offset=20, n_local=20, frame_batch=40, dec_batch=7, split_small=True,
                                           clips=[(s, s + 4, False) for s in range(17, 37)])
    out["halo_tail_sent"] = cfg(kind="halo", L=40, offset=20, n_local=20, tail_sent=True, clips=[(s, s + 4, False) for s in range(17, 37)])
    out["halo_no_full_group"] = cfg(kind="halo", L=23, offset=20, n_local=3, clips=[(s, s + 4, False) for s in (17, 18, 19)] + [(20, 23, True)])
    out["halo_no_whole_clip"] = cfg(kind="halo", L=23, offset=20, n_local=3, clips=[(s, s + 4, False) for s in (17, 18, 19)])
    out["halo_short_straddler"] = cfg(kind="halo", L=24, offset=20, n_local=4, clips=[(18, 21, False), (20, 24, False)])
    out["halo_too_long"] = cfg(kind="halo", L=80, offset=20, n_local=60, cache_frames=1, clips=[(s, s + 4, False) for s in range(17, 77)])
    # ---- online carry: pushes of a video in progress
    out["carry_first_push"] = cfg(kind="carry", offset=0, n_local=10, carry_rows=0, tail_from=7, clips=[(s, s + 4, False) for s in range(0, 7)])
    out["carry_rows3"] = cfg(kind="carry", offset=10, n_local=9, carry_rows=3, tail_from=16, clips=[(s, s + 4, False) for s in range(7, 16)])
    out["carry_one_frame_push"] = cfg(kind="carry", offset=19, n_local=1, carry_rows=3, tail_from=17, clips=[(16, 20, False)])
    out["carry_no_clip"] = cfg(kind="carry", offset=0, n_local=2, carry_rows=0, tail_from=0, clips=[])
    out["carry_close"] = cfg(kind="carry", offset=20, n_local=0, carry_rows=3, tail_from=20, clips=[(17, 20, True)])
    out["carry_tail_behind_last_clip"] = cfg(kind="carry", T=3, stride=5, offset=0, n_local=14, frame_batch=4, carry_rows=0, tail_from=15,
                                             clips=[(0, 3, False), (5, 8, False), (10, 13, False)])
    out["carry_tail_in_skipped_frames"] = cfg(kind="carry", T=3, stride=5, offset=0, n_local=12, frame_batch=4, carry_rows=0, tail_from=10,
                                              clips=[(0, 3, False), (5, 8, False)])
    out["carry_rows3_db7_la1"] = cfg(kind="carry", offset=10, n_local=30, carry_rows=3, tail_from=37, dec_batch=7, lookahead=1, frame_batch=6,
                                     clips=[(s, s + 4, False) for s in range(7, 37)])
    out["carry_tail_sent"] = cfg(kind="carry", offset=10, n_local=9, carry_rows=3, tail_from=16, tail_sent=True,
                                 clips=[(s, s + 4, False) for s in range(7, 16)])
    out["carry_outside"] = cfg(kind="carry", offset=10, n_local=9, carry_rows=2, tail_from=16, clips=[(s, s + 4, False) for s in range(7, 16)])
    out["carry_too_long"] = cfg(kind="carry", offset=10, n_local=60, carry_rows=3, tail_from=67, cache_frames=1,
                                clips=[(s, s + 4, False) for s in range(7, 67)])
    return out


class _Engine:
    """The engine's four seams.  A cache row is 3 floats (12 bytes) without the encoder tokens, 4 with them."""

    def __init__(self, rec):
        self.rec = rec

    def geometry(self, h, w):
        return types.SimpleNamespace(N=15300, h=h, w=w)                 # (N: 20 frames per pass "by resolution")

    def cache_shapes(self, geo, keep_enc=False):
        shapes = {"vals": (), "mf": (), "coords": ()}
        if keep_enc:
            shapes["enc"] = ()
        return shapes

    def decode_clips(self, cache, starts, T, geo, two_streams=True):
        mf = cache["mf"]
        self.rec.log("decode", self.rec.buffer_of(mf), int(mf.shape[0]), [int(s) for s in starts], int(T), bool(two_streams),
                     [[int(v) for v in mf[s:s + T].tolist()] for s in starts])
        return {"tok": torch.zeros(len(starts))}

    def inference_clips(self, outs, mf, starts, T):
        self.rec.log("inference", self.rec.buffer_of(mf), int(mf.shape[0]), [int(s) for s in starts], int(T), int(outs["tok"].shape[0]))
        return [{"row": torch.tensor(float(s))} for s in starts]


class _Halo:
    def __init__(self, rec, T, offset, tail_sent):
        self.rec, self.T, self.offset, self.tail_sent = rec, T, offset, tail_sent

    def head(self):
        self.rec.log("halo.head")
        v = torch.arange(self.offset - (self.T - 1), self.offset, dtype=torch.float32)
        return v.clone(), v.clone()

    def on_tail(self, enc_tail, mf_tail):
        self.tail_sent = True
        self.rec.log("halo.on_tail", [int(v) for v in enc_tail.tolist()], [int(v) for v in mf_tail.tolist()])


class _Carry:
    def __init__(self, rec, rows, offset, tail_from, tail_sent):
        self.rec, self.rows, self.offset, self.tail_from, self.tail_sent = rec, rows, offset, tail_from, tail_sent

    def head(self, ring, at):
        self.rec.log("carry.head", self.rec.buffer_of(ring["mf"]), int(at), int(self.rows))
        for v in ring.values():
            v[at:at + self.rows] = torch.arange(self.offset - self.rows, self.offset, dtype=torch.float32)

    def on_tail(self, views):
        self.tail_sent = True
        self.rec.log("carry.on_tail", sorted(views), [int(v) for v in views["mf"].tolist()],
                     all(torch.equal(v, views["mf"]) for v in views.values()))


class Recorder:
    def __init__(self):
        self.trace, self.buffers = [], []

    def log(self, *entry):
        self.trace.append(list(entry))

    def buffer_of(self, t):
        """Which allocation (in order) a cache tensor or a view of its first rows belongs to."""
        return self.buffers.index(t.data_ptr())

    def model(self, c):
        from mdqe_cvpr2023_amd.meta_arch import MDQE
        m = MDQE.__new__(MDQE)
        nn.Module.__init__(m)
        m.device = torch.device("cpu")
        m.cfg = types.SimpleNamespace(n_frames_test=c["T"], clip_stride=c["stride"])
        m._engine = _Engine(self)
        m.frame_batch, m.dec_batch, m.lookahead = c["frame_batch"], c["dec_batch"], c["lookahead"]
        m.taper_passes, m.taper_tail = c["taper"], c["taper_tail"]
        m.overlap_streams = m.early_decode = m.decode_ahead = True
        if c["cache_gb"] is not None:
            m.CACHE_GB = c["cache_gb"]
        alloc = m.alloc_cache
        rec = self

        def alloc_cache(frames, geo, keep_enc=False):
            ring = alloc(frames, geo, keep_enc)
            for v in ring.values():
                v.fill_(-1.0)
            rec.buffers.append(ring["mf"].data_ptr())
            rec._keep = getattr(rec, "_keep", []) + [ring]             # (an address is never reused within a trace)
            rec.log("alloc", int(frames), sorted(ring))
            return ring

        def frame_cache(frames, geo, ring=None, at=0, keep_enc=False, dec_ready=None):
            idx = frames[:, 0, 0, 0]
            n = int(idx.shape[0])
            rec.log("pass", int(idx[0]) if n else None, n, rec.buffer_of(ring["mf"]), int(at), int(ring["mf"].shape[0]))
            for v in ring.values():
                v[at:at + n] = idx

        def cache_from_tokens(enc, mf, geo, ring, at):
            rec.log("halo.rows", rec.buffer_of(ring["mf"]), int(at), [int(v) for v in enc.tolist()])
            for v in ring.values():
                v[at:at + enc.shape[0]] = enc

        m.alloc_cache, m._frame_cache, m._cache_from_tokens = alloc_cache, frame_cache, cache_from_tokens
        return m

    def run(self, c):
        from mdqe_cvpr2023_amd.meta_arch import MDQE
        env = os.environ.pop("MDQE_CACHE_FRAMES", None)
        if c["cache_frames"]:
            os.environ["MDQE_CACHE_FRAMES"] = str(c["cache_frames"])
        try:
            m = self.model(c)
            n_local = c["L"] if c["n_local"] is None else c["n_local"]
            clips = MDQE.clip_schedule(c["L"], c["T"], c["stride"]) if c["clips"] is None else [tuple(x) for x in c["clips"]]
            frames = torch.arange(c["offset"], c["offset"] + n_local, dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 1, 2, 2)
            kw = {}
            if c["kind"] == "halo":
                kw["halo"] = _Halo(self, c["T"], c["offset"], c["tail_sent"])
            elif c["kind"] == "carry":
                kw["carry"] = _Carry(self, c["carry_rows"], c["offset"], c["tail_from"], c["tail_sent"])
            gen = m.iter_clip_results(frames, clips, c["offset"], primed=c["primed"], prime_all=c["prime_all"],
                                      side_streams=c["side_streams"], split_small=c["split_small"],
                                      on_frames_queued=lambda: self.log("frames_queued"), **kw)
            for item in gen:
                if item is None:
                    self.log("yield", None)
                else:
                    s, e, last, res = item
                    self.log("yield", int(s), int(e), bool(last), int(res["row"]), res["ready"], bool(res["batch_end"]))
        except Exception as exc:                                       # the scheduler's own refusals are part of the trace
            self.log("error", type(exc).__name__, str(exc))
        finally:
            os.environ.pop("MDQE_CACHE_FRAMES", None)
            if env is not None:
                os.environ["MDQE_CACHE_FRAMES"] = env
        return self.trace


def record_all():
    return {name: {"config": c, "trace": Recorder().run(c)} for name, c in configurations().items()}


def dumps(traces):
    lines = []
    for name, t in traces.items():
        body = ",\n".join("   " + json.dumps(e) for e in t["trace"])
        lines.append(' %s: {"config": %s,\n  "trace": [\n%s]}' % (json.dumps(name), json.dumps(t["config"]), body))
    return "{\n" + ",\n".join(lines) + "\n}\n"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    text = dumps(record_all())
    with open(out, "w") as f:
        f.write(text)
    print("%s: %d configurations, %d bytes" % (out, len(json.loads(text)), len(text)))
