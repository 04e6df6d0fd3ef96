"""Per-frame track boxes and areas from the final-mask kernels (ops.final_masks_geom / final_masks_rle_geom) and the surfaces above
them (model.geometry_output, online_video(geometry=True)).  Every comparison is exact: integers, bools, byte strings.

Kernel against the oracle on logits that take only the values +-1, +-2, +-3: with factor 4 every interpolation weight is a multiple of
1/4, every up-sampled value an exact multiple of 1/16 in fp32, so a pixel is exactly 0 (not set, in the kernel and in the oracle alike)
or at least 1/16 away from the threshold -- no rounding can flip a bit.

Wall time of this file on one MI355X (pytest's own figure, model construction included): 4.2 s for its 20 tests; the model tests stay
on the small R50_ovis_360 at 96 x 160.
"""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = [(24, 40, 90, 150, 90, 150), (24, 40, 96, 160, 135, 225), (24, 40, 90, 150, 61, 97), (16, 24, 60, 90, 120, 180),
          (90, 160, 360, 640, 360, 640)]                      # (Hm, Wm, h, w, Ho, Wo)
FACTOR = 4


def _int_logits(n, Fw, Hm, Wm, seed):
    """Background -1 / -2 / -3, 0-3 rectangles of +1 / +2 / +3 per (track, frame); map (0, 0) all negative, map (n-1, Fw-1) all positive."""
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


def _oracle_masks(lg, h, w, Ho, Wo):
    """mdqe/mdqe.py:357-358 + 458-462 on the CPU: x4 aligned bilinear, sigmoid, crop, nearest resize, > 0.5 -> bool [n, Fw, Ho, Wo]."""
    import mdqe_oracle as O
    up = O.aligned_bilinear(lg, FACTOR).sigmoid()[..., :h, :w]
    return F.interpolate(up, size=(Ho, Wo), mode="nearest") > 0.5


def _oracle_geom(masks):
    """(areas int64 [...], boxes float32 [..., 4]) of bool [..., H, W] by a plain pixel count and oracle.mask_bounding_boxes."""
    import mdqe_oracle as O
    flat = masks.reshape(-1, masks.shape[-2], masks.shape[-1])
    return flat.flatten(1).sum(1).view(masks.shape[:-2]), O.mask_bounding_boxes(flat).view(*masks.shape[:-2], 4)


def _rle_strings(pos, n_pos, total):
    from mdqe_cvpr2023_amd import rle as R
    mx = max(int(n_pos.max()), 1)
    counts, lengths = R.positions_to_counts(pos[:, :mx].cpu().numpy(), n_pos.cpu().numpy(), total)
    return R.counts_to_strings(counts, lengths)


def _check_geom(geom, masks_kf, Ho, Wo):
    """geom int32 [k*Fw, 5] against the oracle's masks [k, Fw, Ho, Wo]: raw rows and the d2 form."""
    from mdqe_cvpr2023_amd import rle as R
    areas, boxes = _oracle_geom(masks_kf)
    g = geom.cpu().view(*masks_kf.shape[:2], 5)
    assert g.dtype == torch.int32
    bx, ar = R.geom_to_boxes(g)
    assert torch.equal(ar, areas) and torch.equal(bx, boxes)
    empty = areas == 0
    assert torch.equal(g[empty], torch.tensor([0, Wo, Ho, -1, -1], dtype=torch.int32).expand(int(empty.sum()), 5))
    ne = g[~empty].long()
    assert torch.equal(torch.stack([ne[:, 1], ne[:, 2], ne[:, 3] + 1, ne[:, 4] + 1], 1).float(), boxes[~empty])
    return int(empty.sum()), int((areas == Ho * Wo).sum())


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_against_the_oracle_bit_certain(shape):
    import rle_oracle as RO
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    n, Fw = 5, 3
    lg = _int_logits(n, Fw, Hm, Wm, seed=Hm + Wo)
    want = _oracle_masks(lg, h, w, Ho, Wo)
    assert not bool(want[0, 0].any()) and bool(want[n - 1, Fw - 1].all())
    dev = lg.cuda()
    for rows in ([0, 1, 2, 3, 4], [3, 0, 4, 1]):                  # every row; a strict subset in another order
        idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
        k, f_off, L = len(rows), 2, Fw + 3                         # frames 0-1 and L-1 are guards
        out = torch.full((k + 1, L, Ho, Wo), 0xAB, dtype=torch.uint8, device="cuda")     # (row k is a guard too)
        geom = torch.full((k * Fw, 5), -12345, dtype=torch.int32, device="cuda")          # garbage: must be fully overwritten
        out2, geom2 = ops.final_masks_geom(dev, idx, FACTOR, h, w, Ho, Wo, out, f_off, geom=geom)
        assert out2 is out and geom2 is geom
        torch.cuda.synchronize()
        o = out.cpu()
        assert torch.equal(o[:k, f_off:f_off + Fw].view(torch.bool), want[rows])
        assert bool((o[:k, :f_off] == 0xAB).all()) and bool((o[:k, f_off + Fw:] == 0xAB).all()) and bool((o[k] == 0xAB).all())
        n_empty, n_full = _check_geom(geom, want[rows], Ho, Wo)
        assert n_empty >= 1 and n_full >= 1

        cap = 8 * (Ho + Wo) + 64
        rgeom = torch.full((k * Fw, 5), 777, dtype=torch.int32, device="cuda")
        pos, n_pos, rgeom2 = ops.final_masks_rle_geom(dev, idx, FACTOR, h, w, Ho, Wo, cap, geom=rgeom)
        assert rgeom2 is rgeom and int(n_pos.max()) <= cap
        assert torch.equal(rgeom.cpu(), geom.cpu())
        strs = _rle_strings(pos, n_pos, Ho * Wo)
        for j, (i, f) in enumerate((i, f) for i in rows for f in range(Fw)):
            assert strs[j] == RO.encode(want[i, f].numpy())["counts"], (i, f)
        # a buffer the wrapper allocates itself gives the same rows
        _, g3 = ops.final_masks_geom(dev, idx, FACTOR, h, w, Ho, Wo, out, f_off)
        assert torch.equal(g3, geom)

    # n_sel = 0: MDQE_OK, nothing touched
    idx0 = torch.zeros(0, dtype=torch.int32, device="cuda")
    out = torch.full((1, Fw, Ho, Wo), 0xAB, dtype=torch.uint8, device="cuda")
    _, g0 = ops.final_masks_geom(dev, idx0, FACTOR, h, w, Ho, Wo, out, 0)
    pos, n_pos, g1 = ops.final_masks_rle_geom(dev, idx0, FACTOR, h, w, Ho, Wo, 64)
    torch.cuda.synchronize()
    assert tuple(g0.shape) == (0, 5) and tuple(g1.shape) == (0, 5) and tuple(n_pos.shape) == (0,) and bool((out == 0xAB).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_same_bits_as_the_existing_entry_points(shape):
    """Ordinary float logits: the untouched kernels (ops.final_masks / final_masks_rle) are the yardstick."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd import rle as R
    Hm, Wm, h, w, Ho, Wo = shape
    n, Fw = 6, 4
    g = torch.Generator().manual_seed(Hm * 7 + Ho)
    dev = (torch.randn(n, Fw, Hm, Wm, generator=g) * 2).cuda()
    idx = torch.tensor([5, 2, 0, 3, 1], dtype=torch.int32, device="cuda")
    k = int(idx.numel())
    ref = ops.final_masks(dev, idx, FACTOR, h, w, Ho, Wo, torch.zeros(k, Fw + 1, Ho, Wo, dtype=torch.uint8, device="cuda"), 1)
    out, geom = ops.final_masks_geom(dev, idx, FACTOR, h, w, Ho, Wo, torch.zeros(k, Fw + 1, Ho, Wo, dtype=torch.uint8, device="cuda"), 1)
    assert torch.equal(out, ref)
    want = R.geometry_dense(ref[:, 1:].view(torch.bool))           # [k, Fw, 5] from the parent kernel's masks (device reduction)
    assert torch.equal(geom.view(k, Fw, 5), want)
    assert int(geom[:, 0].min()) > 0                               # (random logits: no mask is empty here)
    cap = Ho * Wo + 1
    pos0, n0 = ops.final_masks_rle(dev, idx, FACTOR, h, w, Ho, Wo, cap)
    pos1, n1, rgeom = ops.final_masks_rle_geom(dev, idx, FACTOR, h, w, Ho, Wo, cap)
    assert torch.equal(n1, n0)
    col = torch.arange(cap, device="cuda")[None] < n0[:, None]
    assert torch.equal(pos1[col], pos0[col])
    assert torch.equal(rgeom.view(k, Fw, 5), want)
    # identical from run to run (integer atomics: no dependence on the order in which blocks arrive)
    for _ in range(2):
        _, again = ops.final_masks_geom(dev, idx, FACTOR, h, w, Ho, Wo, torch.zeros_like(out), 1)
        assert torch.equal(again, geom)
    _, _, again = ops.final_masks_rle_geom(dev, idx, FACTOR, h, w, Ho, Wo, cap)
    assert torch.equal(again, rgeom)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)
    return cfg, MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()


def _video(L, h=96, w=160, n_obj=4):
    from bench import synth_video
    return synth_video(0, L, seed=1, h=h, w=w, n_obj=n_obj)


@pytest.fixture(scope="module")
def small():
    return _model(n_frames_window_test=6)


def _decode(rles):
    import rle_oracle as RO
    return torch.from_numpy(np.stack([RO.rle_decode(RO.rle_from_string(r["counts"].encode()), r["size"][0], r["size"][1]) for r in rles]))


def _check_result_geometry(res, L, Ho, Wo):
    """pred_boxes / pred_areas of a result against the geometry of its own masks (dense, or the decoded RLE strings)."""
    from mdqe_cvpr2023_amd import rle as R
    n_out = len(res["pred_scores"])
    assert len(res["pred_boxes"]) == n_out and len(res["pred_areas"]) == n_out
    non_empty = 0
    for j in range(n_out):
        m = res["pred_masks"][j] if "pred_masks" in res else _decode(res["pred_rles"][j])
        assert tuple(m.shape) == (L, Ho, Wo)
        bx, ar = R.geom_to_boxes(R.geometry_dense(m))
        b, a = res["pred_boxes"][j], res["pred_areas"][j]
        assert b.dtype == torch.float32 and tuple(b.shape) == (L, 4) and a.dtype == torch.int64 and tuple(a.shape) == (L,)
        assert torch.equal(b, bx) and torch.equal(a, ar), j
        non_empty += int((a > 0).sum())
    assert non_empty > 0                                            # not a test on empty data
    return non_empty


def _equal_results(a, b, keys):
    assert set(a) == set(b) == keys
    assert a["image_size"] == b["image_size"] and a["pred_labels"] == b["pred_labels"] and a["pred_scores"] == b["pred_scores"]
    if "pred_masks" in keys:
        assert len(a["pred_masks"]) == len(b["pred_masks"])
        assert all(torch.equal(x, y) for x, y in zip(a["pred_masks"], b["pred_masks"]))
    if "pred_rles" in keys:
        assert a["pred_rles"] == b["pred_rles"]
    for kk in ("pred_boxes", "pred_areas"):
        if kk in keys:
            assert len(a[kk]) == len(b[kk]) and all(torch.equal(x, y) for x, y in zip(a[kk], b[kk]))


BASE = {"image_size", "pred_scores", "pred_labels"}
GEO = {"pred_boxes", "pred_areas"}


@pytest.mark.parametrize("early", [True, False])
@pytest.mark.parametrize("size", [(96, 160), (90, 150)])
def test_forward_geometry_output(small, early, size):
    cfg, model = small
    L, (Ho, Wo) = 17, size
    frames = _video(L).cuda()
    inp = [{"image": frames, "height": Ho, "width": Wo}]
    assert model.geometry_output is False
    saved = model.early_masks
    model.early_masks = early
    try:
        off = model(inp)                                             # the flag as constructed: what the parent returns
        model.geometry_output = True
        on = model(inp)
        model.rle_output = True
        on_rle = model(inp)
        model.geometry_output = False
        off_rle = model(inp)
        model.rle_output = False
        off2 = model(inp)
    finally:
        model.geometry_output, model.rle_output, model.early_masks = False, False, saved
    _equal_results(off, off2, BASE | {"pred_masks"})
    assert set(on) == BASE | GEO | {"pred_masks"} and set(on_rle) == BASE | GEO | {"pred_rles"}
    _equal_results({k: v for k, v in on.items() if k not in GEO}, off, BASE | {"pred_masks"})         # masks unchanged
    _equal_results({k: v for k, v in on_rle.items() if k not in GEO}, off_rle, BASE | {"pred_rles"})   # RLEs unchanged
    _check_result_geometry(on, L, Ho, Wo)
    _check_result_geometry(on_rle, L, Ho, Wo)
    assert all(torch.equal(x, y) for x, y in zip(on["pred_boxes"], on_rle["pred_boxes"]))
    assert all(torch.equal(x, y) for x, y in zip(on["pred_areas"], on_rle["pred_areas"]))


# ---- zeros before a track's first window: hand-made window logits whose track count grows ------------------------------------------------
def _hand_windows(model, frame_hw):
    cfg = model.cfg
    geo = model.engine.geometry(*frame_hw)
    Hm, Wm = geo.Hp // cfg.match_stride, geo.Wp // cfg.match_stride
    wins, f_off = [], 0
    for wi, (n, nf) in enumerate(((2, 6), (4, 6), (5, 3))):
        lg = _int_logits(n, nf, Hm, Wm, seed=100 + wi)
        c = torch.zeros(n, cfg.num_classes)
        c[torch.arange(n), torch.arange(n) % cfg.num_classes] = 0.9 - 0.1 * torch.arange(n)
        wins.append((f_off, nf, n, lg, c))
        f_off += nf
    return wins, (Hm, Wm), f_off


def _expect_hand(wins, track, frame_hw, Ho, Wo):
    parts = []
    for f_off, nf, n, lg, c in wins:
        parts.append(_oracle_masks(lg[track:track + 1], frame_hw[0], frame_hw[1], Ho, Wo)[0] if track < n
                     else torch.zeros(nf, Ho, Wo, dtype=torch.bool))
    return torch.cat(parts)


def _check_hand(res, wins, frame_hw, Ho, Wo, inst):
    L = sum(w[1] for w in wins)
    late = 0
    for j, i in enumerate(inst):
        want = _expect_hand(wins, i, frame_hw, Ho, Wo)
        got = res["pred_masks"][j] if "pred_masks" in res else _decode(res["pred_rles"][j])
        assert torch.equal(got, want), (j, i)
        areas, boxes = _oracle_geom(want)
        assert torch.equal(res["pred_areas"][j], areas) and torch.equal(res["pred_boxes"][j], boxes), (j, i)
        first = next(w[0] for w in wins if i < w[2])                 # the track's first window starts here
        assert not bool(got[:first].any()) and not bool(res["pred_areas"][j][:first].any()) and not bool(res["pred_boxes"][j][:first].any())
        if first > 0:
            late += 1
            assert int(res["pred_areas"][j][first:].sum()) > 0
    assert late >= 3 and len(res["pred_areas"][0]) == L


@pytest.mark.parametrize("rle", [False, True])
def test_zeros_before_a_tracks_first_window_late_and_early_paths(small, rle):
    from mdqe_cvpr2023_amd.meta_arch import ClipMerger
    cfg, model = small
    frame_hw, (Ho, Wo) = (96, 160), (90, 150)
    wins, mask_hw, L = _hand_windows(model, frame_hw)
    model.geometry_output, model.rle_output = True, rle
    try:
        with model._on_device(), torch.no_grad():
            cls_clips = [w[4] for w in wins]
            _, _, inst = model.select_tracks(cls_clips)
            assert set(inst) == {0, 1, 2, 3, 4}
            # late path: merge.video_result's loop over the windows with f_off
            late = model.inference_video((Ho, Wo), cls_clips, [(w[0], w[3].cuda()) for w in wins], frame_hw, L)
            _check_hand(late, wins, frame_hw, Ho, Wo, inst)
            # early path: ClipMerger._early_masks per flushed window, finish() selects
            mg = ClipMerger(model, frame_hw, (Ho, Wo), mask_hw, n_frames=L)
            assert mg.geometry is True
            for f_off, nf, n, lg, c in wins:
                m = lg.cuda()
                mg.side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(mg.side):
                    mg._early_masks(m)
                m.record_stream(mg.side)
                mg.cls_clips.append(c)
                mg.f_off += nf
            early = mg.finish()
            assert mg.early is not None and len(mg.early.geom) == len(wins)
            _check_hand(early, wins, frame_hw, Ho, Wo, inst)
            _equal_results(early, late, BASE | GEO | {"pred_rles" if rle else "pred_masks"})
    finally:
        model.geometry_output, model.rle_output = False, False


@pytest.mark.parametrize("emit", ["masks", "rle"])
def test_online_window_records_carry_the_windows_geometry(small, emit):
    from mdqe_cvpr2023_amd.meta_arch import ClipMerger
    cfg, model = small
    frame_hw, (Ho, Wo) = (96, 160), (90, 150)
    wins, mask_hw, L = _hand_windows(model, frame_hw)
    with model._on_device(), torch.no_grad():
        mg = ClipMerger(model, frame_hw, (Ho, Wo), mask_hw, n_frames=None, online=emit, geometry=True)
        plain = ClipMerger(model, frame_hw, (Ho, Wo), mask_hw, n_frames=None, online=emit)
        assert plain.geometry is False
        for f_off, nf, n, lg, c in wins:
            m = lg.cuda()
            recs = []
            for g in (mg, plain):
                g.side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(g.side):
                    recs.append(g._online_window(c, m))
                m.record_stream(g.side)
                g.f_off += nf
            rec, rec0 = recs
            for r in recs:
                if r["ready"] is not None:
                    r["ready"].synchronize()
            assert "geom" not in rec0 and rec["frames"] == (f_off, f_off + nf)
            want = _oracle_masks(lg, frame_hw[0], frame_hw[1], Ho, Wo)
            if emit == "masks":
                assert torch.equal(rec["masks"], want) and torch.equal(rec0["masks"], want)
            else:
                assert rec["rles"] == rec0["rles"]
                assert all(torch.equal(_decode(rec["rles"][i]), want[i]) for i in range(n))
            assert tuple(rec["geom"].shape) == (n, nf, 5)
            _check_geom(rec["geom"].reshape(-1, 5), want, Ho, Wo)


# ---- online sessions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emit", ["masks", "rle"])
def test_online_geometry(small, emit):
    from mdqe_cvpr2023_amd import rle as R
    cfg, model = small
    L, (Ho, Wo) = 17, (90, 150)
    frames = _video(L).cuda()
    model.geometry_output, model.rle_output = True, emit == "rle"
    try:
        ref = model([{"image": frames, "height": Ho, "width": Wo}])
    finally:
        model.geometry_output, model.rle_output = False, False
    _check_result_geometry(ref, L, Ho, Wo)
    for sizes in ([L], [1] * L, [min(5, L - a) for a in range(0, L, 5)]):
        for keep in (False, True):
            ov = model.online_video(height=Ho, width=Wo, emit=emit, keep=keep, geometry=True)
            wins, a = [], 0
            for n in sizes:
                wins += ov.push(frames[a:a + n])
                a += n
            wins += ov.close()
            res = ov.result()
            assert len(wins) == 3 and wins[0].frames[0] == 0 and wins[-1].frames[1] == L
            assert all(x.frames[1] == y.frames[0] for x, y in zip(wins, wins[1:]))
            seen = 0
            for w in wins:
                n, nf = w.cls_probs.shape[0], w.frames[1] - w.frames[0]
                assert w.boxes.dtype == torch.float32 and tuple(w.boxes.shape) == (n, nf, 4)
                assert w.areas.dtype == torch.int64 and tuple(w.areas.shape) == (n, nf)
                if n == 0:
                    continue
                m = w.masks if emit == "masks" else torch.stack([_decode(r) for r in w.rles])
                bx, ar = R.geom_to_boxes(R.geometry_dense(m))
                assert torch.equal(w.boxes, bx) and torch.equal(w.areas, ar)
                seen += int((ar > 0).sum())
            assert seen > 0
            # result(): forward()'s geometry, with or without keep
            assert res["pred_labels"] == ref["pred_labels"] and res["pred_scores"] == ref["pred_scores"]
            assert len(res["pred_boxes"]) == len(ref["pred_boxes"])
            assert all(torch.equal(x, y) for x, y in zip(res["pred_boxes"], ref["pred_boxes"]))
            assert all(torch.equal(x, y) for x, y in zip(res["pred_areas"], ref["pred_areas"]))
            key = "pred_rles" if emit == "rle" else "pred_masks"
            assert (key in res) == keep
    # geometry=False: windows carry None, result() no geometry
    ov = model.online_video(height=Ho, width=Wo, emit=emit)
    wins = ov.push(frames) + ov.close()
    assert wins and all(w.boxes is None and w.areas is None for w in wins)
    assert not (GEO & set(ov.result()))
