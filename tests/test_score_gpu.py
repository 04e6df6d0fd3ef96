"""Scoring against ground truth on the device: ops.final_masks_overlap (csrc/score_ops.hip) against numpy counts on the bits of the
UNTOUCHED dense kernel (ops.final_masks) -- exact integer equality throughout, no tolerance anywhere -- and "pred_gt" of the video paths
(early, late, RLE, label map only, online) against numpy on the dense masks the model returns."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [(24, 40, 90, 150, 90, 150), (24, 40, 96, 160, 135, 225), (24, 40, 90, 150, 61, 97), (16, 24, 60, 90, 120, 180)]   # (Hm, Wm, h, w, Ho, Wo)
FACTOR = 4
POISON = -7


def _int_logits(n, Fw, Hm, Wm, seed):
    """Background -1 / -2 / -3, 0-3 rectangles of +1 / +2 / +3 per (track, frame); map (0, 0) all negative, map (n-1, Fw-1) all positive
    (the construction of the label-map tests)."""
    rng = np.random.default_rng(seed)
    lg = -rng.integers(1, 4, size=(n, Fw, Hm, Wm)).astype(np.float32)
    for i in range(n):
        for f in range(Fw):
            if (i, f) == (0, 0):
                continue
            for _ in range(int(rng.integers(0, 4))):
                y0, x0 = int(rng.integers(0, Hm)), int(rng.integers(0, Wm))
                y1, x1 = y0 + int(rng.integers(1, Hm // 2 + 1)), x0 + int(rng.integers(1, Wm // 2 + 1))
                blk = lg[i, f, y0:y1, x0:x1]
                blk[...] = rng.integers(1, 4, size=blk.shape).astype(np.float32)
    lg[n - 1, Fw - 1] = rng.integers(1, 4, size=(Hm, Wm)).astype(np.float32)
    return torch.from_numpy(lg)


def _gt_planes(G, frames, Ho, Wo, seed, full=None):
    """uint8 [G, frames, Ho, Wo]: 1-2 random rectangles per (track, frame), large enough to overlap one another; track 1 is absent on the
    odd frames; track G-1 (bit 31 when G = 32) is all-set on frame `full`."""
    rng = np.random.default_rng(seed)
    m = np.zeros((G, frames, Ho, Wo), dtype=np.uint8)
    for g in range(G):
        for f in range(frames):
            for _ in range(int(rng.integers(1, 3))):
                y0, x0 = int(rng.integers(0, Ho - 1)), int(rng.integers(0, Wo - 1))
                m[g, f, y0:y0 + int(rng.integers(1, Ho)), x0:x0 + int(rng.integers(1, Wo))] = 1
    if G > 1:
        m[1, 1::2] = 0
    if full is not None:
        m[G - 1, full] = 1
    return m


def _pack(planes):
    """[G <= 32, frames, Ho, Wo] -> the packed words [frames, Ho, Wo] on the device, as int32 (the same bits; `.view(torch.uint32)`)."""
    w = np.zeros(planes.shape[1:], dtype=np.uint32)
    for g in range(planes.shape[0]):
        w |= planes[g].astype(np.uint32) << np.uint32(g)
    return torch.from_numpy(w.view(np.int32)).cuda()


def _dense_bits(dev, idx, shape):
    """The expected bits: the untouched dense kernel, read back -> uint8 [n_sel, Fw, Ho, Wo] (numpy)."""
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    out = torch.full((int(idx.numel()), int(dev.shape[1]), Ho, Wo), 9, dtype=torch.uint8, device="cuda")
    ops.final_masks(dev, idx, FACTOR, h, w, Ho, Wo, out, 0)
    bits = out.cpu().numpy()
    assert bits.max(initial=0) <= 1
    return bits


def _counts(bits, planes):
    """numpy on bits [k, Fw, Ho, Wo] and the window's planes [G, Fw, Ho, Wo] -> (inter int64 [k, G], area int64 [k, Fw])."""
    k, G = bits.shape[0], planes.shape[0]
    inter = (bits.reshape(k, -1).astype(np.float64) @ planes.reshape(G, -1).astype(np.float64).T).astype(np.int64)   # (exact: counts < 2^53)
    return inter, bits.reshape(k, bits.shape[1], -1).sum(2).astype(np.int64)


def _run_case(lg, rows, shape, G, f_off, tail=1, seed=0):
    """One window through the kernel with everything around it poisoned: frames of gt_bits outside the window are all-ones words, inter
    has 3 padding columns and random starting values, one of them 2^32 - 5 in an entry that receives counts, area starts poisoned."""
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    n, Fw = int(lg.shape[0]), int(lg.shape[1])
    dev = lg.cuda()
    idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
    k = len(rows)
    planes = _gt_planes(G, Fw, Ho, Wo, seed + 1, full=Fw - 1)
    words = torch.full((f_off + Fw + tail, Ho, Wo), -1, dtype=torch.int32, device="cuda")
    words[f_off:f_off + Fw] = _pack(planes)
    words = words.view(torch.uint32)
    bits = _dense_bits(dev, idx, shape)
    want_inter, want_area = _counts(bits, planes)
    rng = np.random.default_rng(seed + 2)
    start = rng.integers(0, 1000, size=(k, G + 3)).astype(np.int64)
    hot = np.unravel_index(int(np.argmax(want_inter)), want_inter.shape)
    assert want_inter[hot] > 5                                           # the carry out of the low 32 bits really happens
    start[hot] = 2 ** 32 - 5
    inter = torch.from_numpy(start).cuda()
    area = torch.full((k * Fw,), POISON, dtype=torch.int32, device="cuda")
    got_inter, got_area = ops.final_masks_overlap(dev, idx, FACTOR, h, w, Ho, Wo, words, G, f_off, inter, area)
    assert got_inter is inter and got_area is area
    torch.cuda.synchronize()
    gi, ga = inter.cpu().numpy(), area.cpu().numpy().reshape(k, Fw)
    assert np.array_equal(gi[:, G:], start[:, G:])                       # padding columns unchanged
    assert np.array_equal(gi[:, :G] - start[:, :G], want_inter), np.abs(gi[:, :G] - start[:, :G] - want_inter).max()
    assert int(gi[hot]) == 2 ** 32 - 5 + int(want_inter[hot]) and int(gi[hot]) > 2 ** 32
    assert np.array_equal(ga, want_area)
    # area is column 0 of the geometry table of the same rows
    geom = ops.final_masks_geom(dev, idx, FACTOR, h, w, Ho, Wo, torch.empty(k, Fw, Ho, Wo, dtype=torch.uint8, device="cuda"), 0)[1]
    assert torch.equal(geom.view(k * Fw, 5)[:, 0], area)
    # a second call adds the same counts again and overwrites the areas with the same values; area=None allocates
    _, area2 = ops.final_masks_overlap(dev, idx, FACTOR, h, w, Ho, Wo, words, G, f_off, inter)
    assert np.array_equal(inter.cpu().numpy()[:, :G] - start[:, :G], 2 * want_inter) and torch.equal(area2, area)
    # run to run: the same bits from the same start
    again = torch.from_numpy(start).cuda()
    ops.final_masks_overlap(dev, idx, FACTOR, h, w, Ho, Wo, words, G, f_off, again, torch.full_like(area, POISON))
    assert np.array_equal(again.cpu().numpy(), gi)
    return want_inter, want_area


@pytest.mark.parametrize("G,Fw,f_off", [(5, 3, 2), (32, 3, 0)])
@pytest.mark.parametrize("shape", SHAPES)
def test_overlap_counts_against_the_dense_kernels_bits(shape, G, Fw, f_off):
    Hm, Wm = shape[:2]
    lg = _int_logits(4, Fw, Hm, Wm, seed=Hm + G)
    # not the identity, a repeated row, the all-negative map (0, 0) and the all-positive map (3, Fw - 1): with the all-set ground-truth
    # track of frame Fw - 1 the largest count a block can meet
    inter, area = _run_case(lg, [2, 0, 3, 2], shape, G, f_off, seed=Hm)
    assert area[1, 0] == 0 and area[2, Fw - 1] == shape[4] * shape[5] and inter[2, G - 1] >= shape[4] * shape[5]
    assert np.array_equal(inter[0], inter[3]) and np.array_equal(area[0], area[3])


@pytest.mark.parametrize("G,Fw,f_off", [(1, 1, 0), (32, 1, 2)])
def test_one_track_one_frame_and_bit_31_on_the_odd_shape(G, Fw, f_off):
    shape = SHAPES[2]                                                    # odd Wo: bands and waves do not align
    _run_case(_int_logits(3, Fw, shape[0], shape[1], seed=G), [2, 0], shape, G, f_off, seed=G)


@pytest.mark.parametrize("n_sel,Fw,shape", [(70, 2, (16, 24, 60, 90, 60, 90)), (255, 1, (8, 12, 32, 48, 32, 48)), (3, 1, (16, 24, 60, 90, 60, 90)),
                                            (1, 1, (16, 24, 60, 90, 60, 90))])
def test_many_rows(n_sel, Fw, shape):
    lg = _int_logits(n_sel, Fw, shape[0], shape[1], seed=n_sel)
    _run_case(lg, list(range(n_sel)), shape, 32 if n_sel != 3 else 5, 1, seed=n_sel)


def test_more_rows_than_one_block_holds():
    """300 selected rows (over 5 maps): the rows go in chunks of 256 per block, the second chunk holds 44."""
    shape = (8, 12, 32, 48, 32, 48)
    _run_case(_int_logits(5, 2, shape[0], shape[1], seed=300), [i % 5 for i in range(300)], shape, 32, 0, seed=300)


def test_nothing_to_do_launches_nothing_and_bad_sizes_are_refused():
    from mdqe_cvpr2023_amd import _lib, ops
    shape = (16, 24, 60, 90, 60, 90)
    Hm, Wm, h, w, Ho, Wo = shape
    words = _pack(_gt_planes(5, 4, Ho, Wo, 0)).view(torch.uint32)
    start = torch.arange(4 * 8, dtype=torch.int64, device="cuda").view(4, 8)
    inter = start.clone()
    # n_sel == 0 (with rows to choose from) and Fw == 0
    lg = _int_logits(4, 2, Hm, Wm, 0).cuda()
    _, area = ops.final_masks_overlap(lg, torch.zeros(0, dtype=torch.int32, device="cuda"), FACTOR, h, w, Ho, Wo, words, 5, 0, inter)
    assert area.numel() == 0
    area = torch.full((0,), POISON, dtype=torch.int32, device="cuda")
    ops.final_masks_overlap(lg[:, :0].contiguous(), torch.arange(4, dtype=torch.int32, device="cuda"), FACTOR, h, w, Ho, Wo, words, 5, 4, inter, area)
    torch.cuda.synchronize()
    assert torch.equal(inter, start)
    # bad sizes come back as MDQE_EINVAL through check, without a launch
    idx = torch.arange(4, dtype=torch.int32, device="cuda")
    area = torch.full((8,), POISON, dtype=torch.int32, device="cuda")
    wide = torch.zeros(4, 40, dtype=torch.int64, device="cuda")
    for G in (0, 33):
        with pytest.raises(_lib.MdqeError, match="final_masks_overlap"):
            ops.final_masks_overlap(lg, idx, FACTOR, h, w, Ho, Wo, words, G, 0, wide, area)
    with pytest.raises(_lib.MdqeError, match="code 1"):
        _lib.check(_lib.lib.mdqe_final_masks_overlap(lg.data_ptr(), 4, idx.data_ptr(), 2, Hm, Wm, FACTOR, h, w, Ho, Wo, words.data_ptr(), 5, 0,
                                                     inter.data_ptr(), 4, area.data_ptr(), _lib.cur_stream()), "stride")
    torch.cuda.synchronize()
    assert torch.equal(inter, start) and int(wide.abs().sum()) == 0 and bool((area == POISON).all())
    # the binding refuses a gt_bits that is too short for f_off + Fw
    with pytest.raises(RuntimeError, match="gt_bits holds 4 frames, the window needs f_off \\+ Fw = 5"):
        ops.final_masks_overlap(lg, idx, FACTOR, h, w, Ho, Wo, words, 5, 3, inter, area)
    assert torch.equal(inter, start)


@pytest.mark.parametrize("shape", SHAPES)
def test_float_logits_against_the_dense_kernels_bits(shape):
    """randn * 3: the bits are the dense kernel's own (one device expression on both sides), so this is exact too."""
    g = torch.Generator().manual_seed(shape[4])
    lg = torch.randn(5, 2, shape[0], shape[1], generator=g) * 3
    _run_case(lg, [4, 1, 0, 3, 2], shape, 8, 1, seed=shape[5])


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)
    return cfg, MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()


@pytest.fixture(scope="module", params=[None, 1e-6], ids=["thr_default", "thr_1e-6"])
def scored(request):
    """One 17-frame video (tracker windows of 6, 6, 5 frames) without ground truth, then against a ground truth made of its own masks
    rolled by a few pixels -- one track without frames 4..8, one extra all-background track, and with the lowered class threshold (many
    tracks) padded with further rolls to G >= 33, so that two word groups run -- on every path, once."""
    from bench import synth_video
    from mdqe_cvpr2023_amd.vis_score import GroundTruth
    cfg, model = _model(n_frames_window_test=6) if request.param is None else _model(n_frames_window_test=6, apply_cls_thres=request.param)
    L, (Ho, Wo) = 17, (90, 150)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    inp = {"image": frames, "height": Ho, "width": Wo}
    off = model([inp])
    pm = torch.stack(off["pred_masks"]).numpy().astype(np.uint8)                      # [n_out, L, Ho, Wo]
    tracks = [np.roll(pm[j], (2 + j % 3, 3 + j % 5), axis=(1, 2)) for j in range(pm.shape[0])]
    j = 0
    while request.param is not None and len(tracks) < 33:
        tracks.append(np.roll(pm[j % pm.shape[0]], (-1 - j % 4, 7 + j), axis=(1, 2)))
        j += 1
    tracks[0] = tracks[0].copy()
    tracks[0][4:9] = 0                                                               # "None" on frames 4..8
    tracks.append(np.zeros_like(tracks[0]))                                          # a track that is background throughout
    gm = np.stack(tracks)
    cats = [off["pred_labels"][g % pm.shape[0]] for g in range(gm.shape[0])]
    gt = GroundTruth(masks=torch.from_numpy(gm), category_ids=cats)
    saved = model.early_masks
    runs = {"off": off}
    try:
        runs["early"] = model([dict(inp, ground_truth=gt)])
        model.early_masks = False
        runs["late"] = model([dict(inp, ground_truth=gt)])
        model.early_masks = saved
        model.rle_output = True
        runs["rle"] = model([dict(inp, ground_truth=gt)])
        model.rle_output = False
        model.label_output = "only"
        runs["only"] = model([dict(inp, ground_truth=gt)])
        runs["only_off"] = model([inp])
        model.label_output = False
        runs["off2"] = model([inp])
    finally:
        model.label_output, model.rle_output, model.early_masks = False, False, saved
    return model, frames, inp, gt, gm, runs


def _same_pred_gt(a, b):
    assert set(a) == set(b) == {"inter", "pred_area", "gt_area", "iou"}
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_pred_gt_equals_numpy_on_the_returned_masks(scored):
    model, frames, inp, gt, gm, runs = scored
    off, on = runs["off"], runs["early"]
    pm = torch.stack(off["pred_masks"]).numpy().astype(np.uint8)
    n_out, L = pm.shape[:2]
    G = gm.shape[0]
    print("outputs %d, tracks %d, ground-truth tracks %d (%d word groups)" % (n_out, model.last_num_tracks, G, len(gt.words)))
    assert (G >= 33 and len(gt.words) == 2) or len(gt.words) == 1
    pg = on["pred_gt"]
    want_inter, want_area = _counts(pm, gm)
    assert pg["inter"].dtype == pg["pred_area"].dtype == pg["gt_area"].dtype == torch.int64 and pg["iou"].dtype == torch.float64
    assert tuple(pg["inter"].shape) == (n_out, G) and tuple(pg["pred_area"].shape) == (n_out, L) and tuple(pg["gt_area"].shape) == (G, L)
    assert np.array_equal(pg["inter"].numpy(), want_inter) and int(want_inter.sum()) > 0
    assert np.array_equal(pg["pred_area"].numpy(), want_area)
    assert np.array_equal(pg["gt_area"].numpy(), gm.reshape(G, L, -1).sum(2))
    assert not pg["gt_area"][0, 4:9].any() and not pg["gt_area"][G - 1].any() and not pg["inter"][:, G - 1].any()
    union = want_area.sum(1)[:, None] + gm.reshape(G, -1).sum(1)[None].astype(np.int64) - want_inter
    want_iou = np.where(union > 0, want_inter.astype(np.float64) / np.maximum(union, 1).astype(np.float64), 0.0)
    assert np.array_equal(pg["iou"].numpy(), want_iou) and 0 < want_iou.max() <= 1
    # every other key is what it was without ground truth
    assert set(on) == set(off) | {"pred_gt", "pred_track_ids"} and set(runs["off2"]) == set(off)
    assert len(on["pred_track_ids"]) == n_out
    for r in ("early", "late", "off2"):
        assert runs[r]["image_size"] == off["image_size"] and runs[r]["pred_scores"] == off["pred_scores"] and runs[r]["pred_labels"] == off["pred_labels"]
        assert len(runs[r]["pred_masks"]) == n_out and all(torch.equal(x, y) for x, y in zip(runs[r]["pred_masks"], off["pred_masks"]))


def test_every_path_gives_the_same_pred_gt(scored):
    from mdqe_cvpr2023_amd import rle as R
    from mdqe_cvpr2023_amd.vis_score import YTVISScorer
    model, frames, inp, gt, gm, runs = scored
    ref = runs["early"]["pred_gt"]
    for r in ("late", "rle", "only"):
        _same_pred_gt(runs[r]["pred_gt"], ref)
        assert runs[r]["pred_track_ids"] == runs["early"]["pred_track_ids"] and runs[r]["pred_scores"] == runs["off"]["pred_scores"]
    assert "pred_masks" not in runs["rle"] and runs["only"]["pred_masks"] == []
    # the label map of the scored run is the unscored run's, bit for bit, and so is every other key
    only, only_off = runs["only"], runs["only_off"]
    assert set(only) == set(only_off) | {"pred_gt"} and only["pred_track_ids"] == only_off["pred_track_ids"]
    assert only["pred_label_map"].dtype == torch.uint8 and bool(only["pred_label_map"].any())
    assert torch.equal(only["pred_label_map"], only_off["pred_label_map"])
    assert only["pred_scores"] == only_off["pred_scores"] and only["pred_labels"] == only_off["pred_labels"]
    # (the RLE path's masks are the dense ones: its pred_gt describes what it returned)
    dec = np.stack([np.stack([R.decode_dense(s) for s in track]) for track in runs["rle"]["pred_rles"]])
    assert np.array_equal(dec, torch.stack(runs["off"]["pred_masks"]).numpy().astype(np.uint8))
    L = int(frames.shape[0])
    for sizes in ([L], [5, 1, 7, 4], [1] * L):
        ov = model.online_video(height=inp["height"], width=inp["width"], emit="masks", ground_truth=gt)
        a = 0
        for n in sizes:
            ov.push(frames[a:a + n])
            a += n
        ov.close()
        res = ov.result()
        _same_pred_gt(res["pred_gt"], ref)
        assert res["pred_track_ids"] == runs["early"]["pred_track_ids"]
    ov = model.online_video(height=inp["height"], width=inp["width"])          # no ground truth: no key
    ov.push(frames)
    ov.close()
    assert "pred_gt" not in ov.result()
    # and the scorer takes the result as it is
    sc = YTVISScorer()
    sc.add("video", runs["early"], gt)
    out = sc.evaluate()
    assert out["stats"].shape == (12,) and -1 <= out["AP"] <= 1 and out["AR100"] >= 0


def test_the_video_paths_refuse_a_ground_truth_that_does_not_fit(scored):
    from mdqe_cvpr2023_amd.vis_score import GroundTruth
    model, frames, inp, gt, gm, runs = scored
    L = int(frames.shape[0])
    with pytest.raises(ValueError, match="size"):
        model([dict(inp, ground_truth=GroundTruth(masks=gm[:1, :, :-1], category_ids=[1]))])
    with pytest.raises(ValueError, match="frames"):
        model([dict(inp, ground_truth=GroundTruth(masks=gm[:1, :-1], category_ids=[1]))])
    with pytest.raises(ValueError, match="GroundTruth"):
        model([dict(inp, ground_truth=gm)])
    short = GroundTruth(masks=gm[:1, :10], category_ids=[1])
    ov = model.online_video(height=inp["height"], width=inp["width"], ground_truth=short)
    ov.push(frames[:6])
    ov.push(frames[6:10])
    with pytest.raises(RuntimeError, match="ground truth holds 10"):
        ov.push(frames[10:11])
    ov = model.online_video(height=inp["height"] + 1, width=inp["width"], ground_truth=gt)
    with pytest.raises(ValueError, match="size"):
        ov.push(frames[:L])
