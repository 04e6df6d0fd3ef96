"""The online schedule (mdqe_cvpr2023_amd.online) as pure bookkeeping: same clips and flushes as the offline schedule, every clip at
the first push that holds its frames, every window at the push that first makes its flush clip runnable.  No GPU."""
import dataclasses
import os
import random
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mdqe_cvpr2023_amd import online as O  # noqa: E402
from mdqe_cvpr2023_amd.config import PRESETS  # noqa: E402
from mdqe_cvpr2023_amd.meta_arch import MDQE, ClipMerger  # noqa: E402


def _cases(n=300, seed=0):
    rng = random.Random(seed)
    for _ in range(n):
        L = rng.randint(1, 90)
        T, stride, win = rng.randint(1, 4), rng.choice([1, 2, 5]), rng.choice([1, 3, 6, 10, 30])
        mode = rng.randrange(4)
        if mode == 0:
            sizes = [L]
        elif mode == 1:
            sizes = [1] * L
        else:
            sizes, left = [], L
            while left:
                k = min(left, rng.randint(1, 13 if mode == 2 else 40))
                sizes.append(k)
                left -= k
        yield L, T, stride, win, sizes


def _feed_many_flushes(clips, T, stride, win):
    """The windows ClipMerger.feed_many flushes (the product's own rule, its tracker work stubbed out), clip by clip."""
    m = ClipMerger.__new__(ClipMerger)
    m.model = types.SimpleNamespace(cfg=dataclasses.replace(PRESETS["R50_ovis_360"], n_frames_test=T, clip_stride=stride,
                                                            n_frames_window_test=win))
    m.saved, m.done = 0, False
    flushed = []

    def consume(run, flush, last):
        if flush:
            flushed.append((run[-1][0], m.saved))
            m.saved += 1
        m.done = m.done or bool(last)
    m._consume = consume
    for s, e, last in clips:
        m.feed_many([(s, e, last, {})])
    return flushed


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_online_clips_are_the_offline_schedule_each_at_the_first_push_that_holds_its_frames(seed):
    for L, T, stride, win, sizes in _cases(seed=seed):
        steps = O.plan(sizes, T, stride, win)
        run = [c for st in steps for c in st["clips"]]
        assert run == MDQE.clip_schedule(L, T, stride), (L, T, stride, sizes)
        cum = [st["received"] for st in steps[:-1]]
        for p, st in enumerate(steps):
            for s, e, last in st["clips"]:
                if last:
                    assert p == len(steps) - 1                         # the clamped last clip: only at close()
                else:
                    assert p == next(i for i, r in enumerate(cum) if r >= e)
        assert all(not c[2] for st in steps[:-1] for c in st["clips"])


@pytest.mark.parametrize("seed", [3, 4])
def test_online_flushes_follow_feed_many_and_the_latency_rule(seed):
    for L, T, stride, win, sizes in _cases(seed=seed):
        steps = O.plan(sizes, T, stride, win)
        sched = MDQE.clip_schedule(L, T, stride)
        ref = _feed_many_flushes(sched, T, stride, win)
        got = []
        saved = 0
        for st in steps:
            for s, e, last in st["clips"]:
                if O.is_flush(s, last, saved, stride, win):
                    got.append((s, saved))
                    saved += 1
        assert got == ref, (L, T, stride, win, sizes)
        assert [k for st in steps for k in st["windows"]] == list(range(len(ref)))
        # window k's flush clip: the first scheduled clip after window k-1's with s + stride >= win * (k+1), or the last one (one
        # window per clip: with stride > win a clip satisfies the test for several windows and flushes the next one only); it
        # arrives with the push whose frame count first reaches s + T, or at close()
        cum = [st["received"] for st in steps[:-1]]
        flush_clip, ci = [], 0
        for k in range(len(ref)):
            while not (sched[ci][2] or sched[ci][0] + stride >= win * (k + 1)):
                ci += 1
            flush_clip.append(sched[ci])
            ci += 1
        for p, st in enumerate(steps):
            for k in st["windows"]:
                fl = flush_clip[k]
                want = len(steps) - 1 if fl[2] else next(i for i, r in enumerate(cum) if r >= fl[0] + T)
                assert p == want, (L, T, stride, win, sizes, k)


def test_carry_is_at_most_T_minus_1_frames_and_covers_the_next_clip():
    for L, T, stride, win, sizes in _cases(seed=5):
        nxt, received = 0, 0
        for n in sizes:
            received += n
            _, nxt = O.push_clips(nxt, received, T, stride)
            c0 = O.carry_from(nxt, received)
            assert 0 <= received - c0 <= T - 1
            assert c0 == nxt or nxt >= received


def test_misuse_raises_without_touching_a_device():
    cfg = PRESETS["R50_ovis_360"]
    cpu = types.SimpleNamespace(cfg=cfg, device=torch.device("cpu"))
    with pytest.raises(RuntimeError):
        MDQE.online_video(cpu)
    coco = types.SimpleNamespace(cfg=dataclasses.replace(cfg, is_coco=True), device=torch.device("cuda", 0))
    with pytest.raises(RuntimeError):
        MDQE.online_video(coco)
    ok = types.SimpleNamespace(cfg=cfg, device=torch.device("cuda", 0))
    with pytest.raises(ValueError):
        MDQE.online_video(ok, emit="png")
    ov = MDQE.online_video(ok)
    assert ov.push(torch.empty(0, 3, 8, 8, dtype=torch.uint8)) == []      # n == 0: no-op
    with pytest.raises(RuntimeError):
        ov.close()                                                       # no frames pushed
    with pytest.raises(RuntimeError):
        ov.result()                                                      # before close()
