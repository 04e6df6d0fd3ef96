"""The clip scheduler's PLAN: which frame passes, cache rows, decoder groups and hand-overs a chunk of a video needs, and in which order.

Pure Python over integers -- no torch stream, event or device tensor -- so every scheduling decision can be walked and checked without a
GPU (tests/test_schedule_plan_cpu.py).  `MDQE.iter_clip_results` (meta_arch.py) resolves its parameters into a `Chunk`, pulls
`plan_steps(chunk)` one step at a time and issues the work each step stands for; nothing here depends on what the GPU computes.
"""
import os
from collections import deque
from typing import NamedTuple


def pass_bounds(n_frames, fbatch, taper=True, tail=0, split_small=False):
    """End frames of the passes of the per-frame stages over a chunk of `n_frames`: uniform passes of `fbatch` frames, or
    (taper) a half-size first pass -- the clip stream starts after half a pass instead of a whole one -- and a last pass of
    at most `tail` frames (0: half a pass) -- the tail that runs with an idle frame stream (last decoder batch, tracker,
    mask read-back) is shorter.  Measured: 20/40/40/20 at 360p +0.2-1.1 %; shorter tails lose to the extra pass."""
    bounds = list(range(fbatch, n_frames, fbatch)) + [n_frames]
    if split_small and taper and 16 <= n_frames <= fbatch:
        # a chunk of a sharded video that fits ONE pass goes in two: a round's clip work trails its frames by about the pass queued
        # behind them (the next round's first), and the round is gathered -- and its tracker replay can start on rank 0 -- only then
        return [n_frames // 2, n_frames]
    if taper and n_frames > fbatch:
        h = max(fbatch // 2, 1)
        t = max(min(tail, h), 1) if tail > 0 else h
        bounds = [h] + list(range(h + fbatch, n_frames, fbatch)) + [n_frames]
        if len(bounds) >= 2 and bounds[-1] - bounds[-2] > t and n_frames - t - bounds[-2] >= 4:
            bounds.insert(-1, n_frames - t)
        if len(bounds) >= 3 and bounds[-1] - bounds[-2] < max(min(t, h) // 2, 1):
            # a last pass of a handful of frames (a 60-frame chunk + its 3-frame halo: 20 / 40 / 3) runs every GEMM of the
            # per-frame stages on a sliver: split what lies behind the first pass evenly instead (20 / 22 / 21)
            r = n_frames - h
            k = -(-r // fbatch)
            bounds = [h] + [h + (r * (i + 1)) // k for i in range(k)]
    return bounds


def clip_schedule(L, T, stride):
    """Clip list of mdqe/mdqe.py:308-312: (start, end, is_last); the loop ends at the first clip that
    reaches past the video (it is clamped and may be shorter than T)."""
    clips = []
    for start in range(0, L, stride):
        end = start + T
        last = end > L
        clips.append((start, min(end, L), last))
        if last:
            break
    return clips


# ---- cache capacity ------------------------------------------------------------------------------------------------------------------
def cache_budget_frames(per_frame_bytes, cache_gb):
    """Frames ONE frame-cache buffer may hold: `cache_gb` GB of `per_frame_bytes` rows, or MDQE_CACHE_FRAMES (tests / A-B: force short
    segments; read at call time)."""
    forced = int(os.environ.get("MDQE_CACHE_FRAMES", "0"))
    return forced if forced > 0 else int(cache_gb * 2 ** 30 // max(per_frame_bytes, 1))


def cache_capacity(n_local, lead, fbatch, dec_batch, Tmax, NR, budget, owner=None):
    """(capf, single): rows of one cache buffer for a chunk of `n_local` frames behind `lead` rows -- the whole chunk if `budget` allows
    (single), else segments in two alternating buffers of at least what the groups in flight need.  owner ("halo exchange" / "online
    carry"): a chunk whose rows are exchanged must fit one buffer."""
    gframes = max(fbatch, dec_batch) + Tmax - 1 + fbatch                    # frames one group can span, passes rounded up
    floor = lead + (NR + 1) * gframes                                       # what the groups in flight need at the very least
    want = n_local + lead
    capf = min(want, max(budget, floor))
    single = capf >= want
    if single:
        capf = -(-capf // 8) * 8              # (rounded: videos of similar length reuse the allocator's blocks)
    elif owner is not None:
        raise RuntimeError("%s: a chunk (%d frames) must fit one frame-cache buffer (%d frames; MDQE_CACHE_GB)" % (owner, n_local, capf))
    return capf, single


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
class Chunk(NamedTuple):
    """One call's resolved integers (`resolve`).  Row of local frame f in the first buffer: f + lead."""
    clips: tuple            # the clips that start in this chunk, global frame indices
    strad: tuple            # (halo) the clips that start in the LEFT neighbour's last T-1 frames; they join the last full-length group
    frame_offset: int
    n_local: int
    Tn: int
    bounds: tuple           # pass_bounds of the chunk
    dec_batch: int
    NR: int                 # groups planned (their frame passes queued) ahead of the one being decoded + 1
    capf: int
    lead: int
    halo: bool
    halo_tail_sent: bool
    carry: bool
    carry_tail_from: int
    carry_tail_sent: bool


class Switch(NamedTuple):
    """Continue in the other buffer, whose row 0 becomes local frame `first` (the first frame a clip not yet planned reads): rows
    [src_row, src_row + keep) of the current buffer are copied over once."""
    buffer: int
    first: int
    keep: int
    src_row: int


class Pass(NamedTuple):
    """Local frames [n0, n1) through the per-frame stages, stored at rows [row, row + n1 - n0) of `buffer`."""
    n0: int
    n1: int
    buffer: int
    row: int


class HaloTail(NamedTuple):
    """(halo) The chunk's last frame is queued: rows [row0, row1) hold its last T-1 frames, complete behind the last pass (`new_pass`)
    or behind all that is queued so far."""
    buffer: int
    row0: int
    row1: int
    new_pass: bool


class Group(NamedTuple):
    """Clips [i, j), all of `T` frames, decoded as one batch from rows [0, rows) of `buffer` (row of local frame f: f - base + lead);
    `starts`: the first row of each clip.  new_frames: frames queued for this group -- it waits for the last of those passes, or with 0
    for all that is queued so far.  frames_queued: the chunk's last frame is now queued (announced once)."""
    i: int
    j: int
    T: int
    buffer: int
    base: int
    lead: int
    rows: int
    new_frames: int
    starts: tuple
    frames_queued: bool


class CarryTail(NamedTuple):
    """(carry) Every clip is planned and the frames from local frame `t0` on are queued: rows [row0, row1) of the first buffer are
    handed over."""
    t0: int
    row0: int
    row1: int


class Consume(NamedTuple):
    """Decoder + inference_clips of the oldest planned group.  send_tail: the halo's tail goes out first.  straddlers: the halo's
    straddling clips join this group (their rows close `starts`, behind the group's own).  ahead: the group planned next if it needs no
    new frame pass and no straddlers are pending -- a decode-ahead candidate -- or None."""
    group: Group
    send_tail: bool
    straddlers: tuple
    starts: tuple
    ahead: Group


def resolve(clips, frame_offset, n_local, Tn, fbatch, dec_batch, lookahead, taper, taper_tail, split_small, per_frame_bytes, cache_gb,
            halo=False, halo_tail_sent=False, carry=False, carry_rows=0, carry_tail_from=0, carry_tail_sent=False):
    """The `Chunk` of one call; raises what can be refused before any work is issued."""
    Tmax = max((c[1] - c[0] for c in clips), default=1)
    # halo exchange (sharded videos, sharding._Halo): `clips` may START up to T-1 frames before this chunk; those clips read
    # the LEFT neighbour's last T-1 frames, which arrive as encoder tokens + mask features and get their cache entries in the
    # `lead` rows IN FRONT of this chunk's first frame (so a straddling clip's frames are consecutive rows); in return the tokens
    # of this chunk's last T-1 frames are handed to `halo.on_tail` as soon as the last pass is queued.
    strad, lead = [], 0
    if halo:
        strad = [c for c in clips if c[0] < frame_offset]
        clips = [c for c in clips if c[0] >= frame_offset]
        if any(c[1] - c[0] != Tn or c[0] < frame_offset - (Tn - 1) for c in strad) or not clips:
            raise RuntimeError("halo exchange: a chunk must hold at least one whole clip and its straddling clips T frames")
        lead = Tn - 1 if strad else 0
    elif carry:
        lead = carry_rows
        if any(c[0] < frame_offset - lead or c[1] > frame_offset + n_local for c in clips):
            raise RuntimeError("online carry: a clip reads frames outside the carried rows and the chunk")
    dec_batch = max(0, int(dec_batch))        # clips per decoder batch the planner waits for (0: whatever one frame pass completes)
    NR = max(2, lookahead + 1)
    capf, _ = cache_capacity(n_local, lead, fbatch, dec_batch, Tmax, NR, cache_budget_frames(per_frame_bytes, cache_gb),
                             "halo exchange" if halo else "online carry" if carry else None)
    return Chunk(tuple(clips), tuple(strad), frame_offset, n_local, Tn, tuple(pass_bounds(n_local, fbatch, taper, taper_tail, split_small)),
                 dec_batch, NR, capf, lead, halo, halo_tail_sent, carry, carry_tail_from, carry_tail_sent)


def plan_steps(ch):
    """The steps of a chunk's schedule, lazily and in issue order: up to `NR` groups are planned -- each behind the segment switch and
    the frame passes it still needs -- then the oldest is consumed, and so on.

    A group starts at the first clip not yet planned; the planner queues passes until `dec_batch` clips (at least one) are complete,
    and every further clip of the same length whose frames are then cached joins the batch -- clips are independent through the
    decoder, so they run as ONE pass (M = clips*T*Q rows)."""
    clips, off, n_local, Tn, bounds = ch.clips, ch.frame_offset, ch.n_local, ch.Tn, ch.bounds
    strad = ch.strad
    b, base, lead = 0, 0, ch.lead             # row of local frame f in buffer b: f - base + lead
    nxt = 0                                   # local frames [0, nxt) have been through the per-frame stages
    ci = 0                                    # clips [0, ci) are planned
    planned = deque()                         # groups planned and not yet consumed, in clip order
    tail_ready, halo_sent, carry_sent, announced = False, ch.halo_tail_sent, ch.carry_tail_sent, False
    while True:
        while len(planned) < ch.NR:
            if ci >= len(clips):
                if ch.carry and not carry_sent:
                    t0 = min(max(ch.carry_tail_from - off, -ch.lead), n_local)
                    nxt = max(nxt, t0)            # frames no clip reads (CLIP_STRIDE > clip length)
                    while nxt < n_local:
                        c1 = next(e for e in bounds if e > nxt)
                        yield Pass(nxt, c1, b, nxt - base + lead)
                        nxt = c1
                    yield CarryTail(t0, t0 + ch.lead, nxt + ch.lead)
                    carry_sent = True
                break
            T = clips[ci][1] - clips[ci][0]
            ls = clips[ci][0] - off
            nxt = max(nxt, ls)                    # CLIP_STRIDE > clip length: the frames between two clips are never read
            k = ci
            while k + 1 < len(clips) and k + 1 - ci < max(ch.dec_batch, 1) and clips[k + 1][1] - clips[k + 1][0] == T:
                k += 1
            target = clips[k][1] - off
            end = nxt
            while end < target:
                end = next(e for e in bounds if e > end)
            if end - base + lead > ch.capf:
                if any(g.buffer == 1 - b for g in planned):
                    raise RuntimeError("frame cache: a buffer is needed again while a group still reads it (capacity %d frames)" % ch.capf)
                yield Switch(1 - b, ls, nxt - ls, ls - base + lead)
                b, base, lead = 1 - b, ls, 0
            first_new = nxt
            while nxt < end:
                c1 = next(e for e in bounds if e > nxt)
                yield Pass(nxt, c1, b, nxt - base + lead)
                nxt = c1
            rows = nxt - base + lead
            if ch.halo and nxt >= n_local and not tail_ready and not halo_sent:
                yield HaloTail(b, rows - min(Tn - 1, n_local), rows, nxt > first_new)
                tail_ready = True
            j = ci
            while j < len(clips) and clips[j][1] - off <= nxt and clips[j][1] - clips[j][0] == T:
                j += 1
            queued = nxt >= n_local and not announced
            announced = announced or queued
            group = Group(ci, j, T, b, base, lead, rows, nxt - first_new, tuple(c[0] - off - base + lead for c in clips[ci:j]), queued)
            planned.append(group)
            ci = j
            yield group
        if not planned:
            break
        send_tail = tail_ready and not halo_sent
        halo_sent = halo_sent or send_tail
        cur = planned.popleft()
        joining = ()
        if strad and cur.T == Tn and (cur.j >= len(clips) or clips[cur.j][1] - clips[cur.j][0] != Tn):
            # the last full-length group of the chunk: the straddling clips join it.  Cache rows [0, T-1) = the left neighbour's
            # last T-1 frames, directly in front of this chunk's first frame
            joining, strad = strad, ()
        starts = cur.starts + tuple(c[0] - off - cur.base + cur.lead for c in joining)
        ahead = planned[0] if planned and planned[0].new_frames == 0 and not strad else None
        yield Consume(cur, send_tail, joining, starts, ahead)
    if strad:
        raise RuntimeError("halo exchange: the chunk has no full-length group for its straddling clips (chunk_plan(..., halo_exchange=True) "
                           "merges a short last chunk into its neighbour)")
