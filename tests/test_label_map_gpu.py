"""Per-frame track label maps (ops.final_label_map) and the surfaces above them (model.label_output, online_video(emit="labels")).

One definition: among the selected rows whose final-mask bit is set at a pixel the row with the largest up-sampled logit owns it, the
first such row on an exact tie; label = track row + 1, 0 where no bit is set.

Kernel against the oracle on logits that take only the values +-1, +-2, +-3: with factor 4 every interpolation weight is a multiple of
1/4 and every up-sampled value an exact multiple of 1/16 in fp32, whatever the order and fusing of the four products -- so values, bits
and exact ties are the same on the device and on the CPU, and every comparison is exact.  Float logits: the untouched dense kernel
gives the bits (exact), a float64 recomputation from the same fp32 logits the argmax.  There a pixel whose two best set rows lie closer
than 1e-5 in float64 is left out: the fp32 blend of four logits of |v| <~ 10 with weights in [0, 1] carries at most a few ulp(10) ~ 1e-6
of rounding, so 1e-5 cannot hide a wrong winner, and the share of such pixels is a condition of its own (<= 0.1 %, measured 0 to 4.3e-5
for these seeds).

Both kernel forms run on every kernel case: the shipped cache-read one and the LDS-staged one (MDQE_LABEL_MAP_STAGE=1, taken wherever
the selected maps' source rows fit its budget: every case but n_sel = 255).

Wall time of this file on one MI355X (pytest's own figure, two model constructions included): 3.1 s for its 30 tests.  The model cases:
1 track per window with the preset's class threshold, 43 with it lowered to 1e-6.
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

SHAPES = [(24, 40, 90, 150, 90, 150), (24, 40, 96, 160, 135, 225), (24, 40, 90, 150, 61, 97), (16, 24, 60, 90, 120, 180)]   # (Hm, Wm, h, w, Ho, Wo)
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


def _oracle_values(lg, h, w, Ho, Wo):
    """mdqe/mdqe.py:357-358 + 458-462 on the CPU: x4 aligned bilinear, crop, nearest resize -> (values [n, Fw, Ho, Wo], bits as
    sigmoid(value) > 0.5, the rule of the dense masks)."""
    import mdqe_oracle as O
    up = O.aligned_bilinear(lg, FACTOR)[..., :h, :w]
    return F.interpolate(up, size=(Ho, Wo), mode="nearest"), F.interpolate(up.sigmoid(), size=(Ho, Wo), mode="nearest") > 0.5


def _oracle_labels(lg, rows, h, w, Ho, Wo):
    """-> (label map uint8 [Fw, Ho, Wo], number of pixels whose winner is tied with another set row)."""
    v, bits = _oracle_values(lg[rows], h, w, Ho, Wo)
    score = torch.where(bits, v, torch.full_like(v, float("-inf")))
    k = score.argmax(0)                                             # torch: the FIRST maximum -- the tie rule
    ids = torch.tensor(rows, dtype=torch.int64) + 1
    want = torch.where(bits.any(0), ids[k], torch.zeros_like(k)).to(torch.uint8)
    tied = ((score == score.max(0)[0][None]) & bits).sum(0) >= 2
    return want, int(tied.sum())


def _label_geom(want, rows, Ho, Wo):
    """int32 [len(rows) * Fw, 5]: pixel count and tight box of want[f] == rows[k] + 1, empty = (0, Wo, Ho, -1, -1)."""
    out = []
    for r in rows:
        for f in range(want.shape[0]):
            ys, xs = np.nonzero(want[f].numpy() == r + 1)
            out.append([len(ys), xs.min(), ys.min(), xs.max(), ys.max()] if len(ys) else [0, Wo, Ho, -1, -1])
    return torch.tensor(out, dtype=torch.int32).view(-1, 5)


@pytest.fixture(params=["cached", "staged"])
def form(request, monkeypatch):
    """Every kernel case in both forms: the shipped one (map rows read through the caches) and LDS staging switched on (the entry
    point reads the variable at every call; it stages wherever the rows fit its budget)."""
    if request.param == "staged":
        monkeypatch.setenv("MDQE_LABEL_MAP_STAGE", "1")
    else:
        monkeypatch.delenv("MDQE_LABEL_MAP_STAGE", raising=False)
    return request.param


def _run_int_case(lg, rows, shape, f_off=2, tail=1):
    """The kernel on integer logits against the oracle: map, guard frames, geometry.  -> (want, tied pixels, geom)."""
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    Fw, k = int(lg.shape[1]), len(rows)
    want, tied = _oracle_labels(lg, rows, h, w, Ho, Wo)
    dev = lg.cuda()
    idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
    out = torch.full((f_off + Fw + tail, Ho, Wo), 0xAB, dtype=torch.uint8, device="cuda")
    geom = torch.full((k * Fw, 5), -12345, dtype=torch.int32, device="cuda")             # garbage: must be fully overwritten
    out2, geom2 = ops.final_label_map(dev, idx, FACTOR, h, w, Ho, Wo, out, f_off, geom=geom)
    assert out2 is out and geom2 is geom
    torch.cuda.synchronize()
    o = out.cpu()
    assert torch.equal(o[f_off:f_off + Fw], want)
    assert bool((o[:f_off] == 0xAB).all()) and bool((o[f_off + Fw:] == 0xAB).all())
    g = geom.cpu()
    assert torch.equal(g, _label_geom(want, rows, Ho, Wo))
    # without geometry, and with a table the wrapper allocates: the same map, the same rows
    out3 = torch.full_like(out, 0xCD)
    _, none = ops.final_label_map(dev, idx, FACTOR, h, w, Ho, Wo, out3, f_off)
    _, g4 = ops.final_label_map(dev, idx, FACTOR, h, w, Ho, Wo, torch.empty_like(out), f_off, geom=True)
    assert none is None and torch.equal(out3[f_off:f_off + Fw].cpu(), want) and torch.equal(g4.cpu(), g)
    return want, tied, g


@pytest.mark.parametrize("shape", SHAPES)
def test_label_map_against_the_oracle_bit_certain(shape, form):
    Hm, Wm, h, w, Ho, Wo = shape
    n, Fw = 5, 3
    lg = _int_logits(n, Fw, Hm, Wm, seed=Hm + Wo)
    for rows in ([0, 1, 2, 3, 4], [3, 0, 4, 1]):                  # every row; a strict subset in another order
        want, tied, g = _run_int_case(lg, rows, shape)
        assert tied >= 1 and int((want == 0).sum()) >= 1 and int((g[:, 0] == 0).sum()) >= 1
        assert set(want.unique().tolist()) <= {0} | {r + 1 for r in rows}


@pytest.mark.parametrize("n_sel,Fw,shape", [(70, 2, (16, 24, 60, 90, 60, 90)), (255, 1, (8, 12, 32, 48, 32, 48)), (1, 1, (16, 24, 60, 90, 60, 90))])
def test_many_tracks_and_the_edges_of_the_table(n_sel, Fw, shape, form):
    Hm, Wm = shape[:2]
    lg = _int_logits(n_sel, Fw, Hm, Wm, seed=n_sel)
    rows = torch.randperm(n_sel, generator=torch.Generator().manual_seed(n_sel)).tolist()
    want, tied, g = _run_int_case(lg, rows, shape)
    assert int(want.max()) <= n_sel and int((want != 0).sum()) > 0
    if n_sel > 64:
        assert len(want.unique()) > 8 and tied >= 1              # (many labels really win pixels)


def test_no_tracks_is_all_background(form):
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = 16, 24, 60, 90, 60, 90
    Fw = 2
    dev = torch.zeros(0, Fw, Hm, Wm, device="cuda")
    idx = torch.zeros(0, dtype=torch.int32, device="cuda")
    out = torch.full((Fw + 2, Ho, Wo), 0xAB, dtype=torch.uint8, device="cuda")
    _, g = ops.final_label_map(dev, idx, FACTOR, h, w, Ho, Wo, out, 1, geom=True)
    torch.cuda.synchronize()
    o = out.cpu()
    assert tuple(g.shape) == (0, 5) and g.dtype == torch.int32
    assert bool((o[1:1 + Fw] == 0).all()) and bool((o[0] == 0xAB).all()) and bool((o[-1] == 0xAB).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_float_logits_against_the_untouched_kernels(shape, form):
    import mdqe_oracle as O
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    n, Fw = 6, 4
    gen = torch.Generator().manual_seed(Hm * 7 + Ho)
    lg = torch.randn(n, Fw, Hm, Wm, generator=gen) * 2
    dev = lg.cuda()
    rows = [5, 2, 0, 3, 1, 4]
    idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
    masks = ops.final_masks(dev, idx, FACTOR, h, w, Ho, Wo, torch.zeros(n, Fw, Ho, Wo, dtype=torch.uint8, device="cuda"), 0).view(torch.bool)
    out, geom = ops.final_label_map(dev, idx, FACTOR, h, w, Ho, Wo, torch.full((Fw + 1, Ho, Wo), 0xAB, dtype=torch.uint8, device="cuda"), 1, geom=True)
    lab = out[1:].long()
    # exact: the union, the labelled row's own mask, the areas
    assert torch.equal(lab != 0, masks.any(0))
    row_of = torch.zeros(256, dtype=torch.int64, device="cuda")
    row_of[idx.long() + 1] = torch.arange(n, device="cuda")
    own = masks.gather(0, row_of[lab][None])[0]                     # the dense bit of the row the label names
    assert bool(own[lab != 0].all())
    areas = torch.stack([(lab == r + 1).flatten(1).sum(1) for r in rows])          # [k, Fw]
    assert torch.equal(geom.view(n, Fw, 5)[..., 0].long(), areas)
    from mdqe_cvpr2023_amd import rle as R
    assert torch.equal(geom.view(n, Fw, 5), R.geometry_dense(torch.stack([lab == r + 1 for r in rows])))
    # argmax against float64 from the same fp32 logits
    v64 = F.interpolate(O.aligned_bilinear(lg[rows].double(), FACTOR)[..., :h, :w], size=(Ho, Wo), mode="nearest")
    m = masks.cpu()
    score = torch.where(m, v64, torch.full_like(v64, float("-inf")))
    top = score.topk(2, dim=0)
    decided = m.any(0) & ~((top.values[0] - top.values[1]) < 1e-5)  # (one set row: gap = inf)
    left_out = float((m.any(0) & ~decided).sum()) / float(m.any(0).numel())
    print("shape %s form %s: left out of the argmax comparison %.3g of all pixels" % (shape, form, left_out))
    assert left_out <= 1e-3
    want = (torch.tensor(rows)[top.indices[0]] + 1)
    got = lab.cpu()
    assert torch.equal(got[decided], want[decided])
    # identical from run to run (integer atomics only)
    for _ in range(2):
        out2, geom2 = ops.final_label_map(dev, idx, FACTOR, h, w, Ho, Wo, torch.empty_like(out), 1, geom=True)
        assert torch.equal(out2[1:], out[1:]) and torch.equal(geom2, geom)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)
    return cfg, MDQE(cfg, state_dict=random_state(cfg, seed=3)).eval()


@pytest.fixture(scope="module")
def small():
    return _model(n_frames_window_test=6)


BASE = {"image_size", "pred_scores", "pred_labels"}
LAB = {"pred_label_map", "pred_track_ids"}


def _same_head(a, b):
    assert a["image_size"] == b["image_size"] and a["pred_labels"] == b["pred_labels"] and a["pred_scores"] == b["pred_scores"]


def _region_geometry(lm, track_ids):
    from mdqe_cvpr2023_amd import rle as R
    return R.geom_to_boxes(R.geometry_dense(R.labels_to_masks(lm, track_ids)))


@pytest.fixture(scope="module", params=[None, 1e-6], ids=["thr_default", "thr_1e-6"])
def model_video(request, small):
    """One 17-frame video (three tracker windows of 6, 6, 5 frames) through forward() with the feature off and in every setting, once.
    The random weights score every query far below the preset's class threshold, which leaves the tracker ONE track; the second case
    lowers APPLY_CLS_THRES so that more queries become tracks.  What the tests assert holds for any number of tracks (the windows in
    which the count GROWS, from none, are the hand-made ones below); test_online_labels_equal_forward prints the counts."""
    from bench import synth_video
    cfg, model = small if request.param is None else _model(n_frames_window_test=6, apply_cls_thres=request.param)
    L, (Ho, Wo) = 17, (90, 150)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    inp = [{"image": frames, "height": Ho, "width": Wo}]
    assert model.label_output is False
    saved = model.early_masks
    runs = {}
    try:
        runs["off"] = model(inp)
        model.label_output = True
        runs["early"] = model(inp)
        model.early_masks = False
        runs["late"] = model(inp)
        model.early_masks = saved
        model.label_output = "only"
        runs["only"] = model(inp)
        model.early_masks = False
        runs["only_late"] = model(inp)
        model.early_masks = saved
        model.label_output, model.geometry_output = True, True
        runs["geo"] = model(inp)
        model.rle_output = True
        runs["geo_rle"] = model(inp)
        model.label_output, model.geometry_output, model.rle_output = False, False, False
        runs["off2"] = model(inp)
    finally:
        model.label_output, model.geometry_output, model.rle_output, model.early_masks = False, False, False, saved
    return model, frames, L, (Ho, Wo), runs


def test_model_label_output_leaves_the_other_outputs_alone(model_video):
    model, frames, L, (Ho, Wo), runs = model_video
    off, on = runs["off"], runs["early"]
    assert set(off) == set(runs["off2"]) == BASE | {"pred_masks"} and set(on) == BASE | LAB | {"pred_masks"}
    for r in ("early", "late", "geo", "off2"):
        _same_head(runs[r], off)
        assert len(runs[r]["pred_masks"]) == len(off["pred_masks"])
        assert all(torch.equal(x, y) for x, y in zip(runs[r]["pred_masks"], off["pred_masks"]))
    lm = on["pred_label_map"]
    assert lm.dtype == torch.uint8 and tuple(lm.shape) == (L, Ho, Wo) and not lm.is_cuda
    assert len(on["pred_track_ids"]) == len(on["pred_scores"]) and int(lm.max()) > 0
    # the same map from the early path, the late path and "only" (either path), with geometry and with RLE output
    for r in ("late", "only", "only_late", "geo", "geo_rle"):
        assert torch.equal(runs[r]["pred_label_map"], lm), r
        assert runs[r]["pred_track_ids"] == on["pred_track_ids"]
    for r in ("only", "only_late"):
        _same_head(runs[r], off)
        assert set(runs[r]) == BASE | LAB | {"pred_masks"} and runs[r]["pred_masks"] == []
    assert set(runs["geo_rle"]) == BASE | LAB | {"pred_rles", "pred_boxes", "pred_areas", "pred_label_boxes", "pred_label_areas"}
    # output j's dense mask covers its exclusive region
    seen = 0
    for j, t in enumerate(on["pred_track_ids"]):
        region = lm == t + 1
        assert not bool((region & ~on["pred_masks"][j]).any()), j
        seen += int(region.sum())
    assert seen > 0
    # geometry of the regions; pred_boxes / pred_areas keep meaning the full masks
    geo = runs["geo"]
    bx, ar = _region_geometry(lm, geo["pred_track_ids"])
    assert all(torch.equal(geo["pred_label_boxes"][j], bx[j]) and torch.equal(geo["pred_label_areas"][j], ar[j]) for j in range(len(ar)))
    from mdqe_cvpr2023_amd import rle as R
    fb, fa = R.geom_to_boxes(R.geometry_dense(torch.stack(geo["pred_masks"])))
    assert all(torch.equal(geo["pred_boxes"][j], fb[j]) and torch.equal(geo["pred_areas"][j], fa[j]) for j in range(len(fa)))
    assert all(torch.equal(x, y) for x, y in zip(runs["geo_rle"]["pred_label_areas"], geo["pred_label_areas"]))


def test_online_labels_equal_forward(model_video):
    from mdqe_cvpr2023_amd import rle as R
    model, frames, L, (Ho, Wo), runs = model_video
    ref = runs["early"]
    lm = ref["pred_label_map"]
    # every track's dense masks per window: what the map's union must be
    ov = model.online_video(height=Ho, width=Wo, emit="masks")
    dense = ov.push(frames) + ov.close()
    counts = [len(w.track_ids) for w in dense]
    print("tracks per window:", counts)
    assert len(dense) == 3 and min(counts) > 0 and counts == sorted(counts)       # (tracker rows only ever grow)
    for sizes in ([L], [1] * L, [min(5, L - a) for a in range(0, L, 5)]):
        ov = model.online_video(height=Ho, width=Wo, emit="labels", keep=True, geometry=True)
        wins, a = [], 0
        for n in sizes:
            wins += ov.push(frames[a:a + n])
            a += n
        wins += ov.close()
        res = ov.result()
        assert [w.frames for w in wins] == [w.frames for w in dense]
        for w, d in zip(wins, dense):
            nf = w.frames[1] - w.frames[0]
            assert w.masks is None and w.rles is None and w.track_ids == d.track_ids
            assert w.labels.dtype == torch.uint8 and tuple(w.labels.shape) == (nf, Ho, Wo)
            assert torch.equal(w.labels != 0, d.masks.any(0))                         # the union of ALL tracks' masks
            assert torch.equal(R.labels_to_masks(w.labels, w.track_ids).any(0), d.masks.any(0))
            own = R.labels_to_masks(w.labels, w.track_ids)
            assert not bool((own & ~d.masks).any())                                    # a label names a track whose mask holds the pixel
            bx, ar = _region_geometry(w.labels, w.track_ids)
            assert torch.equal(w.boxes, bx) and torch.equal(w.areas, ar)
        assert torch.equal(torch.cat([w.labels for w in wins]), lm)                    # window records concatenate to forward()'s map
        assert torch.equal(res["pred_label_map"], lm) and res["pred_track_ids"] == ref["pred_track_ids"]
        _same_head(res, ref)
        assert all(torch.equal(x, y) for x, y in zip(res["pred_label_areas"], runs["geo"]["pred_label_areas"]))
        assert all(torch.equal(x, y) for x, y in zip(res["pred_label_boxes"], runs["geo"]["pred_label_boxes"]))
        assert "pred_masks" not in res and "pred_boxes" not in res
    ov = model.online_video(height=Ho, width=Wo, emit="labels")                       # keep=False: the windows only
    wins = ov.push(frames) + ov.close()
    assert torch.equal(torch.cat([w.labels for w in wins]), lm) and all(w.boxes is None for w in wins)
    assert "pred_label_map" not in ov.result()


# ---- hand-made windows whose track count grows from none: every path against the oracle ----------------------------------------------
def _hand_windows(model, frame_hw):
    cfg = model.cfg
    geo = model.engine.geometry(*frame_hw)
    Hm, Wm = geo.Hp // cfg.match_stride, geo.Wp // cfg.match_stride
    wins, f_off = [], 0
    for wi, (n, nf) in enumerate(((0, 3), (2, 6), (4, 6), (5, 3))):
        lg = _int_logits(n, nf, Hm, Wm, seed=200 + wi) if n else torch.zeros(0, nf, Hm, Wm)
        c = torch.zeros(n, cfg.num_classes)
        c[torch.arange(n), torch.arange(n) % cfg.num_classes] = 0.9 - 0.1 * torch.arange(n)
        wins.append((f_off, nf, n, lg, c))
        f_off += nf
    return wins, (Hm, Wm), f_off


@pytest.mark.parametrize("mode", [True, "only"])
def test_hand_made_windows_early_late_and_online_paths(small, mode):
    from mdqe_cvpr2023_amd.meta_arch import ClipMerger
    cfg, model = small
    frame_hw, (Ho, Wo) = (96, 160), (90, 150)
    wins, mask_hw, L = _hand_windows(model, frame_hw)
    want = torch.cat([_oracle_labels(lg, list(range(n)), frame_hw[0], frame_hw[1], Ho, Wo)[0] if n
                      else torch.zeros(nf, Ho, Wo, dtype=torch.uint8) for _, nf, n, lg, _ in wins])
    assert not bool(want[:3].any()) and set(want.unique().tolist()) == {0, 1, 2, 3, 4, 5}
    model.label_output, model.geometry_output = mode, True
    try:
        with model._on_device(), torch.no_grad():
            cls_clips = [w[4] for w in wins]
            late = model.inference_video((Ho, Wo), cls_clips, [(w[0], w[3].cuda()) for w in wins], frame_hw, L)
            pool = model.pinned_mask_buffer((L, Ho, Wo))
            pool.fill_(0xEE)                                          # the pooled buffer the early path is about to be handed: not zeros
            del pool
            mg = ClipMerger(model, frame_hw, (Ho, Wo), mask_hw, n_frames=L)
            assert mg.labels == mode
            for f_off, nf, n, lg, c in wins:
                m = lg.cuda()
                mg.side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(mg.side):
                    mg._early_masks(m)
                m.record_stream(mg.side)
                mg.cls_clips.append(c)
                mg.f_off += nf
            early = mg.finish()
            assert mg.early.labels is not None and len(mg.early.label_geom) == len(wins)
            assert len(mg.early.hosts) == (0 if mode == "only" else 5)
            on = ClipMerger(model, frame_hw, (Ho, Wo), mask_hw, n_frames=None, online="labels", geometry=True)
            recs = []
            for f_off, nf, n, lg, c in wins:
                m = lg.cuda()
                on.side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(on.side):
                    recs.append(on._online_window(c, m))
                m.record_stream(on.side)
                on.f_off += nf
    finally:
        model.label_output, model.geometry_output = False, False
    for res in (late, early):
        assert torch.equal(res["pred_label_map"], want)
        bx, ar = _region_geometry(want, res["pred_track_ids"])
        assert all(torch.equal(res["pred_label_boxes"][j], bx[j]) and torch.equal(res["pred_label_areas"][j], ar[j]) for j in range(len(ar)))
        assert (res["pred_masks"] == []) == (mode == "only")
    for r, (f_off, nf, n, lg, c) in zip(recs, wins):
        r["ready"].synchronize()
        assert torch.equal(r["labels"], want[f_off:f_off + nf]) and tuple(r["geom"].shape) == (n, nf, 5)
        assert torch.equal(r["geom"].reshape(-1, 5), _label_geom(want[f_off:f_off + nf], list(range(n)), Ho, Wo))
