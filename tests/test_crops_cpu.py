"""Per-track crops without a GPU: the numpy restatement of the rule (tests/_crops_ref.py) against hand-derived cases, render.Crops,
the frame selection of `every` across windows and store pieces, the ABI of the two entries, and the refusals of the wrappers, the
session and the model.  Integers only: every comparison is exact."""
import dataclasses
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _crops_ref as REF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402


def _frames(seed, F, h0, w0):
    return np.random.default_rng(seed).integers(0, 256, size=(F, 3, h0, w0)).astype(np.uint8)


def _run(frames, labels, geom, n, size, **kw):
    return REF.crops(REF.rgb_source(frames), frames.shape[2], frames.shape[3], labels, geom, n, size, **kw)


# ---- the reference against hand-derived cases ------------------------------------------------------------------------------------------
def test_whole_picture_at_its_own_size_is_the_picture():
    Ho, Wo = 7, 9
    fr = _frames(1, 2, Ho, Wo)
    lab = np.ones((2, Ho, Wo), dtype=np.uint8)
    geom = np.array([[Ho * Wo, 0, 0, Wo - 1, Ho - 1]] * 2, dtype=np.int32)
    chips, rects = _run(fr, lab, geom, 1, (Ho, Wo))
    assert np.array_equal(chips[0], np.moveaxis(fr, 1, -1))             # chip[i, j, c] == frames[c, i, j]
    assert rects.tolist() == [[[0, 0, Wo - 1, Ho - 1]] * 2]


def test_integer_upscale_replicates_and_exact_downscale_is_the_rounded_mean():
    fr = _frames(2, 1, 4, 6)
    lab = np.ones((1, 4, 6), dtype=np.uint8)
    geom = np.array([[24, 0, 0, 5, 3]], dtype=np.int32)
    up, _ = _run(fr, lab, geom, 1, (12, 12))                            # x3 rows, x2 columns
    pic = np.moveaxis(fr[0], 0, -1)
    assert np.array_equal(up[0, 0], pic.repeat(3, 0).repeat(2, 1))
    down, _ = _run(fr, lab, geom, 1, (2, 3))
    s = pic.astype(np.int64).reshape(2, 2, 3, 2, 3).sum((1, 3))
    assert np.array_equal(down[0, 0], (s + 2) // 4)
    # a box inside the picture: the same, from its own corner
    geom = np.array([[4, 2, 1, 3, 2]], dtype=np.int32)
    sub, rects = _run(fr, lab, geom, 1, (4, 4))
    assert np.array_equal(sub[0, 0], pic[1:3, 2:4].repeat(2, 0).repeat(2, 1)) and rects[0, 0].tolist() == [2, 1, 3, 2]


def test_a_constant_frame_gives_a_constant_chip_at_every_size():
    fr = np.empty((1, 3, 11, 13), dtype=np.uint8)
    fr[0, 0], fr[0, 1], fr[0, 2] = 7, 200, 255
    lab = np.ones((1, 11, 13), dtype=np.uint8)
    geom = np.array([[50, 1, 2, 11, 9]], dtype=np.int32)
    for size in ((1, 1), (3, 5), (11, 13), (20, 17)):
        chips, _ = _run(fr, lab, geom, 1, size, pad256=40)
        assert (chips[0, 0] == np.array([7, 200, 255], dtype=np.uint8)).all(), size


def test_float_frames_round_half_to_even_clamp_and_nan():
    fr = np.zeros((1, 3, 1, 6), dtype=np.float32)
    fr[0, :, 0] = np.array([0.5, 1.5, 2.5, 254.5, 300.0, np.nan], dtype=np.float32)
    fr[0, 1, 0, 0] = -3.0
    lab = np.ones((1, 1, 6), dtype=np.uint8)
    chips, _ = _run(fr, lab, np.array([[6, 0, 0, 5, 0]], dtype=np.int32), 1, (1, 6))
    assert chips[0, 0, 0, :, 0].tolist() == [0, 2, 2, 254, 255, 0] and chips[0, 0, 0, 0, 1] == 0


def test_cutout_counts_owned_pixels_only_and_fills_where_there_are_none():
    fr = _frames(3, 1, 4, 4)
    lab = np.zeros((1, 4, 4), dtype=np.uint8)
    lab[0, 0, 0] = lab[0, 1, 1] = 1                                     # the top-left 2 x 2 block owns two pixels, the others none
    lab[0, 3, 3] = 2
    geom = np.array([[2, 0, 0, 3, 3]], dtype=np.int32)                  # (a box wider than the region: the table is taken as it is)
    chips, _ = _run(fr, lab, geom, 1, (2, 2), cutout=True, fill=(9, 8, 7))
    pic = np.moveaxis(fr[0], 0, -1).astype(np.int64)
    assert np.array_equal(chips[0, 0, 0, 0], (pic[0, 0] + pic[1, 1] + 1) // 2)
    for i, j in ((0, 1), (1, 0), (1, 1)):                                # (label 2's pixel is not label 1's)
        assert chips[0, 0, i, j].tolist() == [9, 8, 7]
    plain, _ = _run(fr, lab, geom, 1, (2, 2))
    assert np.array_equal(plain[0, 0, 1, 1], (pic[2:, 2:].reshape(4, 3).sum(0) + 2) // 4)


def test_pad_grows_the_box_and_clamps_at_all_four_borders():
    Ho, Wo = 20, 30
    assert REF.rect_of((1, 10, 8, 19, 11), Ho, Wo, 0) == (10, 8, 19, 11)
    assert REF.rect_of((1, 10, 8, 19, 11), Ho, Wo, 64) == (7, 7, 22, 12)            # (10*64+128)>>8 = 3, (4*64+128)>>8 = 1
    assert REF.rect_of((1, 10, 8, 19, 11), Ho, Wo, 256) == (0, 4, 29, 15)           # a full width per side: both x borders
    assert REF.rect_of((1, 1, 1, 12, 9), Ho, Wo, 128) == (0, 0, 18, 14)             # left and top
    assert REF.rect_of((1, 20, 12, 28, 18), Ho, Wo, 128) == (15, 8, 29, 19)         # right and bottom: (9*128+128)>>8 = 5, (7*128+128)>>8 = 4
    assert REF.rect_of((1, 5, 5, 5, 5), Ho, Wo, 127) == (5, 5, 5, 5)                # (127 + 128) >> 8 = 0
    assert REF.rect_of((1, 5, 5, 5, 5), Ho, Wo, 128) == (4, 4, 6, 6)


def test_min_area_and_dead_rows_give_fill_and_the_dead_rect():
    Ho, Wo = 6, 8
    fr = _frames(4, 1, Ho, Wo)
    lab = np.ones((1, Ho, Wo), dtype=np.uint8)
    rows = [(0, Wo, Ho, -1, -1), (5, 1, 1, 3, 3), (5, 3, 1, 1, 3), (5, 0, 0, Wo, 1), (5, 0, -1, 1, 1), (5, 0, 0, 1, Ho), (-4, 0, 0, 1, 1),
            (6, 1, 1, 3, 3)]
    geom = np.array(rows, dtype=np.int32)
    chips, rects = _run(fr, np.repeat(lab, 1, 0), geom, len(rows), (3, 2), min_area=6, fill=(1, 2, 3))
    for k in range(len(rows) - 1):
        assert rects[k, 0].tolist() == [0, 0, -1, -1] and (chips[k, 0] == np.array([1, 2, 3], dtype=np.uint8)).all(), rows[k]
    assert rects[-1, 0].tolist() == [1, 1, 3, 3]                        # area == min_area is live
    assert REF.live((1, 0, 0, 0, 0), Ho, Wo, 0) and not REF.live((0, 0, 0, 0, 0), Ho, Wo, 0)      # min_area 0 still needs one pixel


def test_footprints_are_never_empty_never_leave_the_rect_and_cover_it():
    for ch in range(1, 71):
        for S in range(1, 41):
            spans = [REF.span(i, ch, S, 5) for i in range(S)]
            assert all(a < b <= 5 + ch for a, b in spans), (ch, S)      # Ya < Yb <= Y1 + 1
            assert spans[0][0] == 5 and spans[-1][1] == 5 + ch
            assert all(nxt[0] <= cur[1] for cur, nxt in zip(spans, spans[1:])), (ch, S)      # no source row is skipped


def test_the_fast_form_and_the_surface_source_equal_the_loops():
    rng = np.random.default_rng(7)
    h0, w0, Ho, Wo, F, n = 9, 14, 12, 10, 3, 3
    lab = rng.integers(0, 4, size=(F, Ho, Wo)).astype(np.uint8)
    geom = np.array([REF.box_of(lab[f] == k + 1) for k in range(n) for f in range(F)], dtype=np.int32)
    geom[4] = (0, Wo, Ho, -1, -1)
    kw = dict(first=1, step=1, pad256=32, min_area=2, cutout=True, fill=(3, 2, 1))
    fr = _frames(8, F, h0, w0)
    a = _run(fr, lab, geom, n, (5, 7), **kw)
    b = REF.crops_fast(REF.expand_rgb(fr, Ho, Wo), lab, geom, n, (5, 7), **kw)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].shape == (n, 2, 5, 7, 3)
    for fmt in ("nv12", "p010"):
        ys, cs = YREF.make_content(5, F, h0, w0, fmt)
        for order in ("rgb", "bgr"):
            c = REF.crops(REF.yuv_source(ys, cs, fmt, "bt601", True, order), h0, w0, lab, geom, n, (5, 7), **kw)
            d = REF.crops_fast(REF.expand_yuv(ys, cs, h0, w0, fmt, "bt601", True, order, Ho, Wo), lab, geom, n, (5, 7), **kw)
            assert np.array_equal(c[0], d[0]) and np.array_equal(c[1], d[1]), (fmt, order)


# ---- render.Crops ----------------------------------------------------------------------------------------------------------------------
def test_crops_validation_names_the_field():
    from mdqe_cvpr2023_amd.render import Crops
    c = Crops()
    assert (c.size, c.pad, c.cutout, c.fill, c.min_area, c.every, c.pad256) == ((128, 64), 0.0, False, (0, 0, 0), 0, 1, 0)
    c = Crops(size=[1, 512], pad=0.125, cutout=True, fill=[255, 0, 7], min_area=9, every=3)
    assert c.size == (1, 512) and c.fill == (255, 0, 7) and c.pad256 == 32 and Crops(pad=1).pad256 == 256
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.every = 2
    bad = {"size": [(0, 8), (8, 513), (8,), 8, (8.0, 8), "ab", (True, 8), None], "pad": [-0.1, 1.5, "0", True, None],
           "cutout": [1, 0, None, "yes"], "fill": [(0, 0), (0, 0, 256), (-1, 0, 0), (0.0, 0, 0), 7, None], "min_area": [-1, 1.0, True, 2 ** 31],
           "every": [0, -1, 1.0, True, None]}
    for field, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match="crops: %s must" % field):
                Crops(**{field: v})


def test_every_takes_the_same_frames_whatever_the_windows_and_pieces_are():
    from mdqe_cvpr2023_amd.render import Crops
    for every in (1, 2, 3, 5, 7):
        c = Crops(every=every)
        L = 23
        want = [f for f in range(L) if f % every == 0]
        assert c.taken(0, L) == want and c.count(L) == len(want)
        for win in (1, 4, 6, 7):
            got, at = [], 0
            for f0 in range(0, L, win):
                f1 = min(L, f0 + win)
                assert c.first_in(f0) == (-f0) % every
                assert c.count(f0) == at                                 # the window's chips start where the earlier windows' end
                piece = c.taken(f0, f1)
                assert piece == [f0 + q for q in range(c.first_in(f0), f1 - f0, every)]
                got += piece
                at += len(piece)
            assert got == want, (every, win)


def test_crop_frames_slices_the_table_and_adjusts_first_per_store_piece(monkeypatch):
    """Stand-in launches: a window of 6 frames from video frame 6 whose frames lie in the pushes [5, 10) and [10, 15), every = 4."""
    from mdqe_cvpr2023_amd import merge, ops
    from mdqe_cvpr2023_amd.render import Crops
    store = merge.FrameStore()
    for first in (0, 5, 10):
        store.add(first, torch.full((5, 3, 2, 2), first, dtype=torch.uint8))
    calls = []
    monkeypatch.setattr(ops, "track_crops", lambda lab, fr, g, n, size, out, c_off, rects, first, step, *a: calls.append(
        (tuple(lab.shape), int(fr[0, 0, 0, 0]), len(fr), g[:, :, 0].tolist(), n, c_off, first, step, a)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    labels = torch.zeros(8, 2, 2, dtype=torch.uint8)
    geom = torch.arange(2 * 6, dtype=torch.int32).view(2, 6, 1).repeat(1, 1, 5)
    spec = Crops(size=(4, 4), every=4, pad=0.25, min_area=3, cutout=True, fill=(1, 2, 3))
    done = merge.crop_frames(2, 6, labels, 1, geom, store, 6, spec, "out", "rects", 2)
    assert done == 1 and spec.taken(6, 12) == [8]
    # piece [6, 10): frames 6..9 of push 5, the frame taken is 8 = its frame 2; piece [10, 12) takes nothing and launches nothing
    assert calls == [((4, 2, 2), 5, 4, [[0, 1, 2, 3], [6, 7, 8, 9]], 2, 2, 2, 4, (64, 3, True, (1, 2, 3)))]
    del calls[:]
    assert merge.crop_frames(2, 6, labels, 1, geom, store, 6, Crops(every=2), "out", "rects", 3) == 3
    assert [(c[1], c[2], c[3], c[5], c[6]) for c in calls] == [(5, 4, [[0, 1, 2, 3], [6, 7, 8, 9]], 3, 0), (10, 2, [[4, 5], [10, 11]], 5, 0)]
    del calls[:]
    assert merge.crop_frames(0, 6, labels, 1, geom[:0], store, 6, Crops(every=2), "out", "rects", 3) == 3 and calls == []


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_both_entries_and_they_refuse_bad_arguments():
    from mdqe_cvpr2023_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    for name, n_args in (("mdqe_track_crops_u8", 25), ("mdqe_track_crops_yuv420sp", 32)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
        assert hasattr(h, name) and name in _lib.SIGNATURES
        proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == n_args
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # new entries only
    EINVAL, ENULL = 1, 3
    base = dict(F=3, Ho=8, Wo=8, n=2, f_first=0, f_step=1, Sh=4, Sw=4, pad256=0, min_area=0, cutout=0, fill=0, ors=1 << 20, c_off=0, rrs=1 << 10)

    def tail(q):
        return (None, q["F"], q["Ho"], q["Wo"], None, q["n"], q["f_first"], q["f_step"], q["Sh"], q["Sw"], q["pad256"], q["min_area"],
                q["cutout"], q["fill"], None, q["ors"], q["c_off"], None, q["rrs"], None)

    def rgb(is_u8=1, frame_stride=3 * 64, h0=8, w0=8, **kw):
        return h.mdqe_track_crops_u8(None, is_u8, frame_stride, h0, w0, *tail(dict(base, **kw)))

    def yuv(yp=8, ys=64, cp=8, cs=32, H=8, W=8, fmt=0, matrix=0, **kw):
        return h.mdqe_track_crops_yuv420sp(None, yp, ys, None, cp, cs, H, W, fmt, matrix, 0, 0, *tail(dict(base, **kw)))
    bad = [{"Sh": 0}, {"Sh": 513}, {"Sw": 0}, {"Sw": 513}, {"pad256": -1}, {"pad256": 257}, {"min_area": -1}, {"cutout": 2}, {"cutout": -1},
           {"fill": -1}, {"fill": 1 << 24}, {"n": -1}, {"n": 256}, {"F": -1}, {"Ho": 0}, {"Wo": 0}, {"Ho": 4096, "Wo": 4096}, {"f_first": -1},
           {"f_step": 0}, {"c_off": -1}, {"Sh": 512, "Sw": 512, "c_off": 2800}, {"ors": 3 * 48 - 1}, {"rrs": 11}]
    for call in (rgb, yuv):
        for kw in bad:
            assert call(**kw) == EINVAL, (call.__name__, kw)
            if not {"F", "n", "ors", "rrs"} & set(kw):                   # ... whatever F and n say (the strides are held to the chips of the call)
                assert call(**dict(kw, F=0)) == EINVAL and call(**dict(kw, n=0)) == EINVAL, (call.__name__, kw)
        assert call(F=0) == 0 and call(n=0) == 0 and call(f_first=3) == 0 and call(f_first=7, f_step=2) == 0   # nothing to do: OK, no launch
        assert call(ors=3 * 48, rrs=12) == ENULL and call(n=1, ors=0, rrs=0) == ENULL and call() == ENULL
        assert call(Ho=4095, Wo=4096, Sh=512, Sw=512, pad256=256, cutout=1, fill=0xFFFFFF, n=255, f_first=2, f_step=9) == ENULL
    for kw in ({"h0": 0}, {"w0": 0}, {"is_u8": 2}, {"frame_stride": 3 * 64 - 1}, {"h0": 1 << 20, "Ho": 1 << 12, "Wo": 1}):
        assert rgb(**kw) == EINVAL, kw
    assert rgb(frame_stride=0, F=1) == ENULL                             # (one frame has no stride)
    for kw in ({"H": 0}, {"W": 0}, {"fmt": 2}, {"matrix": 2}, {"yp": 7}, {"cp": 7}, {"ys": -1}, {"cs": -1}, {"fmt": 1, "yp": 17, "cp": 16},
               {"fmt": 1, "yp": 16, "cp": 16, "ys": 129}, {"W": 9, "yp": 9, "cp": 9}):
        assert yuv(**kw) == EINVAL, kw
    assert yuv(W=9, yp=9, cp=10) == ENULL and yuv(fmt=1, yp=16, cp=16, ys=128) == ENULL


# ---- the wrappers' refusals ------------------------------------------------------------------------------------------------------------
def test_wrapper_argument_checks():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    lab = torch.zeros(2, 6, 9, dtype=torch.uint8)
    fr = torch.zeros(2, 3, 6, 9, dtype=torch.uint8)
    geom = torch.zeros(3 * 2, 5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="frames must be uint8 or float32"):
        ops.track_crops(lab, fr.double(), geom, 3, (4, 4))
    with pytest.raises(RuntimeError, match="every frame must be contiguous"):
        ops.track_crops(lab, torch.zeros(2, 3, 6, 18, dtype=torch.uint8)[:, :, :, ::2], geom, 3, (4, 4))
    for bad in (lab.float(), lab[:, :, :8], torch.zeros(2, 6, 9, 1, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match="labels must be contiguous uint8"):
            ops.track_crops(bad, fr, geom, 3, (4, 4))
    with pytest.raises(RuntimeError, match="labels hold F = 1 frames, the frames handed in 2"):
        ops.track_crops(lab[:1], fr, geom, 3, (4, 4))
    with pytest.raises(RuntimeError, match=r"Ho\*Wo < 2\^24"):
        ops.track_crops(torch.zeros(1, 4096, 4096, dtype=torch.uint8), fr[:1], geom, 3, (4, 4))
    for n in (-1, 256, 3.0, True):
        with pytest.raises(RuntimeError, match="n must be an int in 0..255"):
            ops.track_crops(lab, fr, geom, n, (4, 4))
    for size in ((0, 4), (4, 513), (4,), 4, (4.0, 4), None):
        with pytest.raises(RuntimeError, match="size must be"):
            ops.track_crops(lab, fr, geom, 3, size)
    for kw, what in (({"pad256": 257}, "pad256"), ({"pad256": 0.5}, "pad256"), ({"min_area": -1}, "min_area"), ({"c_off": -1}, "c_off"),
                     ({"first": -1}, "first"), ({"step": 0}, "step"), ({"step": True}, "step")):
        with pytest.raises(RuntimeError, match="%s must be an int" % what):
            ops.track_crops(lab, fr, geom, 3, (4, 4), **kw)
    with pytest.raises(RuntimeError, match="cutout must be a bool"):
        ops.track_crops(lab, fr, geom, 3, (4, 4), cutout=2)
    for fill in ((0, 0), (0, 0, 256), 7, (0.0, 0, 0)):
        with pytest.raises(RuntimeError, match="fill must be three ints"):
            ops.track_crops(lab, fr, geom, 3, (4, 4), fill=fill)
    for bad in (geom.float(), geom[:5], geom.view(2, 3, 5), torch.zeros(6, 10, dtype=torch.int32)[:, ::2]):
        with pytest.raises(RuntimeError, match="geom must be contiguous int32"):
            ops.track_crops(lab, fr, bad, 3, (4, 4))
    for out in (torch.zeros(3, 2, 4, 4, 3), torch.zeros(2, 2, 4, 4, 3, dtype=torch.uint8), torch.zeros(3, 1, 4, 4, 3, dtype=torch.uint8),
                torch.zeros(3, 2, 4, 5, 3, dtype=torch.uint8), torch.zeros(3, 2, 4, 4, 6, dtype=torch.uint8)[..., ::2]):
        with pytest.raises(RuntimeError, match="out must be uint8"):
            ops.track_crops(lab, fr, geom, 3, (4, 4), out=out)
    with pytest.raises(RuntimeError, match="out must be uint8"):          # c_off moves the chips past the buffer's end
        ops.track_crops(lab, fr, geom, 3, (4, 4), out=torch.zeros(3, 2, 4, 4, 3, dtype=torch.uint8), c_off=1)
    for rects in (torch.zeros(3, 2, 4), torch.zeros(3, 1, 4, dtype=torch.int32), torch.zeros(3, 2, 5, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="rects must be int32"):
            ops.track_crops(lab, fr, geom, 3, (4, 4), out=torch.zeros(3, 2, 4, 4, 3, dtype=torch.uint8), rects=rects)
    # shapes and dtypes first, devices after (a host without a GPU gets as far as the device check)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor on the frames' device"):
        ops.track_crops(lab, fr, geom, 3, (4, 4), out=torch.zeros(3, 2, 4, 4, 3, dtype=torch.uint8), rects=torch.zeros(3, 2, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="yuv must be a preprocess.YuvFrames"):
        ops.track_crops_yuv(lab, fr, geom, 3, (4, 4))
    with pytest.raises(RuntimeError, match="must be on a HIP device"):
        ops.track_crops_yuv(lab, YuvFrames.empty(2, 6, 9), geom, 3, (4, 4))


# ---- the session's and the model's refusals, on stand-ins ------------------------------------------------------------------------------
def _standin(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)

    def check():
        from mdqe_cvpr2023_amd.meta_arch import MDQE
        MDQE.check_label_capacity(types.SimpleNamespace(cfg=cfg))
    return types.SimpleNamespace(cfg=cfg, device=torch.device("cuda", 0), check_label_capacity=check)


def _cpu_model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    return MDQE(dataclasses.replace(PRESETS["R50_ovis_360"], **kw), seed=1)


def test_online_session_takes_crops_beside_every_emit_and_refuses_what_it_cannot_do():
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.merge import Forms, FrameStore
    from mdqe_cvpr2023_amd.online import Window
    from mdqe_cvpr2023_amd.render import Crops
    spec = Crops(size=(8, 4), every=2)
    for emit in ("masks", "rle", "labels", "overlay"):
        ov = MDQE.online_video(_standin(), emit=emit, crops=spec)
        assert ov.crops is spec and ov.frames_held == 0
        f = Forms.of_emit(emit, crops=True)
        assert f.crops and f == dataclasses.replace(Forms.of_emit(emit), crops=True)
    assert MDQE.online_video(_standin(), emit="masks").crops is None and not Forms.of_emit("masks").crops
    for bad in ((8, 4), "crops", True, {"size": (8, 4)}):
        with pytest.raises(ValueError, match="crops must be a render.Crops"):
            MDQE.online_video(_standin(), emit="masks", crops=bad)
    with pytest.raises(ValueError, match="COCO image config.*video config"):
        MDQE.online_video(_standin(is_coco=True), emit="masks", crops=spec)
    with pytest.raises(ValueError, match="n_max_inst.*exceeds 255"):    # more tracks than the label map has rows for
        MDQE.online_video(_standin(n_max_inst=256), emit="masks", crops=spec)
    MDQE.online_video(_standin(n_max_inst=256), emit="masks")           # (without crops a dense session has no such limit)
    # the window's pseudo-fields: init-only, the dataclass's own fields are what they were
    assert [f.name for f in dataclasses.fields(Window)] == ["frames", "track_ids", "cls_probs", "masks", "rles", "boxes", "areas"]
    w = Window(frames=(0, 2), track_ids=[0], cls_probs=torch.zeros(1, 2), crops="c", crop_rects="r", crop_frames=[0])
    assert (w.crops, w.crop_rects, w.crop_frames, w.labels, w.overlay) == ("c", "r", [0], None, None)
    w = Window(frames=(0, 2), track_ids=[0], cls_probs=torch.zeros(1, 2))
    assert w.crops is None and w.crop_rects is None and w.crop_frames is None
    assert FrameStore().frames_held == 0


def test_model_crop_output_round_trips_resolves_into_the_forms_and_is_refused_where_it_cannot_run():
    from mdqe_cvpr2023_amd import merge, sharding
    from mdqe_cvpr2023_amd.merge import Forms
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.render import Crops
    m = _cpu_model()
    assert m.crop_output is None and not Forms.of_model(m).crops and Forms.of_model(m) == Forms(planes="dense")
    assert m._frame_source(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), None) is None
    spec = Crops(size=(8, 4))
    m.crop_output = spec
    assert m.crop_output is spec
    for attrs, planes, labels in (({}, "dense", False), ({"rle_output": True}, "rle", False), ({"label_output": True}, "dense", True),
                                  ({"label_output": "only"}, None, True)):
        for k, v in attrs.items():
            setattr(m, k, v)
        f = Forms.of_model(m)
        assert f.crops and f.planes == planes and f.labels == labels and not f.overlay
        assert not Forms.of_model(m, emit_masks=False).crops
        for k in attrs:
            setattr(m, k, False)
    store = m._frame_source(torch.zeros(4, 3, 8, 8, dtype=torch.uint8), None)
    assert store.frames_held == 4 and store.surface is None
    for bad in ((8, 4), True, "crops", 0):
        with pytest.raises(ValueError, match="crop_output must be None or a render.Crops"):
            m.crop_output = bad
    m.crop_output = None
    assert m.crop_output is None and Forms.of_model(m) == Forms(planes="dense")
    with pytest.raises(ValueError, match="n_max_inst.*exceeds 255"):
        _cpu_model(n_max_inst=256).crop_output = spec
    # a merger without the video's frames
    with pytest.raises(ValueError, match="crop output needs the frames of the whole video"):
        merge.ClipMerger(types.SimpleNamespace(cfg=m.cfg, crop_output=spec, device=torch.device("cpu"), merge_on_cpu=None), (8, 8), (8, 8), (2, 2))
    # a COCO image config
    coco = types.SimpleNamespace(cfg=dataclasses.replace(m.cfg, is_coco=True), engine=None, device=torch.device("cpu"), crop_output=spec)
    with pytest.raises(ValueError, match="COCO image branch has no crops.*video config"):
        MDQE.inference_image(coco, [{"image": torch.zeros(3, 3, 8, 8)}])
    # the sharded driver
    geo = types.SimpleNamespace(Hp=8, Wp=8, N=4)
    model = types.SimpleNamespace(cfg=m.cfg, device=torch.device("cpu"), engine=types.SimpleNamespace(geometry=lambda h, w: geo), crop_output=spec)
    with pytest.raises(ValueError, match="crop_output is not offered by the sharded driver.*one device"):
        sharding.run_round_robin(model, {0: torch.zeros(4, 3, 8, 8)}, [(0, 0, 4)], 0, 1, None, (8, 8))
