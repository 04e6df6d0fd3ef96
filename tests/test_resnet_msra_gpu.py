"""GPU: MSRA ResNets (MODEL.RESNETS.STRIDE_IN_1X1 True: a downsampling block's stride on the 1x1 conv1; configs/R101_coco.yaml,
R101_ytvis19.yaml) on the product, against the tests' restatement (tests/_resnet_msra.py, pinned to transformers.ResNetModel in
tests/test_resnet_msra_cpu.py) run by the CPU oracle through its `backbone_fn` hook.

  * mdqe_gemm_nt_pix_f32 (the strided 1x1 product of an MSRA conv1) against F.conv2d(stride=s) in fp64;
  * engine.backbone with stride_in_1x1 for R50 and R101 at full size (two 360x640 frames), bar 1e-3 of the activation scale;
  * the R101_ytvis19 preset end to end on 6 frames of 360x640: MDQE.forward against oracle.inference_vis -- every clip's heads,
    then the video's labels, scores and boolean masks;
  * stride_in_1x1 False leaves the R50 backbone bit for bit as the unmodified preset builds it."""
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

import mdqe_oracle as O
from _golden import maxdiff, record_margin
from _resnet_msra import resnet_msra

pytestmark = pytest.mark.gpu
BP = "detr.backbone.0.backbone"
TIE_BAND = 2e-6                     # as tests/test_fullsize_gpu.py: an fp32 near-tie of a query cell's arg-max


def _m(group, stage, got, want, tol, scale=1.0):
    d = record_margin(group, stage, maxdiff(got, want), scale, tol)
    assert d < tol * scale, (group, stage, d, tol * scale)


# ---- the strided 1x1 product -------------------------------------------------------------------------------------------------------
# the three MSRA conv1 shapes (res3.0, res4.0, res5.0 read res2, res3, res4 at stride 2) at 360p (384x640) and 640p (640x1152), then
# odd maps, 1..3 images, a K that is a multiple of 16 but not of 32, a ragged N and stride 3
@pytest.mark.parametrize("NI,H,W,K,N,stride,act", [
    (2, 96, 160, 256, 128, 2, "relu"), (2, 48, 80, 512, 256, 2, "relu"), (2, 24, 40, 1024, 512, 2, "relu"),
    (2, 160, 288, 256, 128, 2, "relu"), (2, 80, 144, 512, 256, 2, "relu"), (2, 40, 72, 1024, 512, 2, "relu"),
    (1, 13, 21, 256, 128, 2, None), (2, 7, 9, 512, 256, 2, "relu"), (3, 25, 41, 1024, 512, 2, None), (3, 11, 17, 48, 40, 3, None),
    (1, 1, 1, 64, 64, 2, "relu")])
def test_strided_1x1_product_against_fp64_conv(NI, H, W, K, N, stride, act):
    from mdqe_cvpr2023_amd import ops
    g = torch.Generator().manual_seed(H * W + K + N)
    x = torch.randn(NI, H, W, K, generator=g)
    w, b = torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)
    out = ops.linear_pix(x.cuda(), stride, w.cuda(), b.cuda(), act=act)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().view(N, K, 1, 1), b.double(), stride).permute(0, 2, 3, 1)
    if act == "relu":
        ref = torch.relu(ref)
    assert out.shape == ref.shape == (NI, (H - 1) // stride + 1, (W - 1) // stride + 1, N)
    scale = float(ref.abs().max())
    assert float((out.cpu().double() - ref).abs().max()) < 3e-6 * scale                 # the k16 kernels' bar against fp64


def test_strided_1x1_product_refuses_a_k_off_the_k_step():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import MdqeError
    x, w = torch.randn(1, 8, 8, 40, device="cuda"), torch.randn(32, 40, device="cuda")
    with pytest.raises(MdqeError):
        ops.linear_pix(x, 2, w, None)


# ---- the backbone at full size -------------------------------------------------------------------------------------------------------
def _hyper(cfg):
    return O.Hyper(**{f.name: getattr(cfg, f.name) for f in dataclasses.fields(O.Hyper)})


@functools.lru_cache(maxsize=None)
def _frames(n, h=360, w=640):
    from bench import synth_video
    return list(synth_video(0, n, seed=0, h=h, w=w))


@functools.lru_cache(maxsize=None)
def _backbone_case(kind):
    """(cfg, weights, oracle res3/res4/res5 NHWC) for two 360x640 frames; the oracle on the MSRA restatement."""
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.params import random_state
    cfg = dataclasses.replace(PRESETS["R101_ytvis19"], backbone=kind)
    sd = random_state(cfg, seed=1)
    with torch.no_grad():
        x, _ = O.pad_frames(O.preprocess(_hyper(cfg), _frames(2)), 32)
        ref = [r.permute(0, 2, 3, 1).contiguous() for r in resnet_msra(sd, BP, x, int(kind[1:]))]
    return cfg, sd, ref


def _run_backbone(cfg, sd, precision="f32"):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.engine import Engine
    eng = Engine(cfg, sd, only_backbone=True)
    geo = eng.geometry(360, 640)
    ops.set_gemm_precision(precision)
    try:
        with torch.no_grad():
            outs = [o.cpu() for o in eng.backbone(torch.stack(_frames(2)).cuda(), geo)]
    finally:
        ops.set_gemm_precision("f32")
    return outs


@pytest.mark.parametrize("kind,precision", [("R50", "f32"), ("R101", "f32"), ("R101", "f16x3")])
def test_msra_backbone_full_size(kind, precision):
    """res3 / res4 / res5 of engine.backbone with stride_in_1x1 against the restatement, 1e-3 of the activation scale (exact fp32: the
    strided conv1 through mdqe_gemm_nt_pix_f32; f16x3: through conv2d_nhwc with stride 2)."""
    cfg, sd, ref = _backbone_case(kind)
    outs = _run_backbone(cfg, sd, precision)
    group = "%s MSRA backbone 2x360x640 %s" % (kind, precision)
    for lvl, o, r in zip(("res3", "res4", "res5"), outs, ref):
        assert o.shape == r.shape, (lvl, o.shape, r.shape)
        _m(group, lvl, o, r, 1e-3, float(r.abs().max()))


def test_stride_in_1x1_false_is_bit_identical_to_the_preset():
    """The 3x3 placement is untouched: a config that states stride_in_1x1=False builds the very backbone of the unmodified preset, and
    the MSRA placement on the same weights is a different network."""
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.params import random_state
    base = PRESETS["R50_ovis_360"]
    sd = random_state(base, seed=1)
    want = _run_backbone(base, sd)
    got = _run_backbone(dataclasses.replace(base, stride_in_1x1=False), sd)
    for o, r in zip(got, want):
        assert torch.equal(o, r)
    msra = _run_backbone(dataclasses.replace(base, stride_in_1x1=True), sd)
    assert msra[0].shape == want[0].shape and float((msra[0] - want[0]).abs().max()) > 1e-2 * float(want[0].abs().max())


# ---- R101_ytvis19 end to end ------------------------------------------------------------------------------------------------------------
def _check_clip(group, res, rc, lscale):
    """tests/test_fullsize_gpu.py's bars on one clip's heads."""
    assert res["pred_masks"].shape == rc["pred_masks"].shape, (res["pred_masks"].shape, rc["pred_masks"].shape)
    assert res["pred_classes"].tolist() == rc["pred_classes"].tolist()
    if rc["pred_masks"].numel():
        _m(group, "clip mask logits", res["pred_masks"].cpu(), rc["pred_masks"], 1e-3, lscale)
        _m(group, "clip scores", res["scores"].cpu(), rc["scores"], 1e-3)
        _m(group, "clip cls_probs", res["cls_probs"].cpu(), rc["cls_probs"], 1e-3)
        _m(group, "clip query_embeds", res["query_embeds"].cpu(), rc["query_embeds"], 1e-3, max(1.0, float(rc["query_embeds"].abs().max())))


def _near_tie_frames(group, sd, hp, feats, model, frames, clips):
    """Frames of `clips` whose product query cells differ from the oracle's; asserts each such pick is within 10 x TIE_BAND of the
    oracle's maximum on the oracle's own score map (the band tests/test_fullsize_gpu.py allows on the product's own encoder tokens)."""
    enc_o, mask_o, shapes, _ = feats
    eng = model.engine
    geo = eng.geometry(*frames[0].shape[-2:])
    with torch.no_grad():
        enc = eng.encode(eng.backbone(torch.stack(frames).cuda(), geo), geo)
        coords = eng.frame_queries(enc, geo)[0].cpu()
    tied = set()
    for idx in clips:
        dbg = {}
        with torch.no_grad():
            O.transformer_dec(sd, hp, enc_o[idx], mask_o[idx], shapes, dbg=dbg)
        for t, f in enumerate(idx):
            co_o = dbg["coords0"][t]
            su = dbg["score_up"][t].reshape(dbg["score_up"].shape[-2:])
            Hu, Wu = su.shape
            for q in ((coords[f] - co_o).abs().amax(-1) > 1e-6).nonzero().flatten().tolist():
                col, row = int(round(float(coords[f, q, 0]) * Wu)), int(float(coords[f, q, 1]) * Hu + 1e-4)
                co, ro = int(round(float(co_o[q, 0]) * Wu)), int(float(co_o[q, 1]) * Hu + 1e-4)
                gap = float(su[ro, co] - su[row, col])
                assert 0.0 <= gap < 10 * TIE_BAND, ("query cell decided differently without a near-tie", f, q, gap)
                record_margin(group, "a11 query cell picked at an fp32 near-tie: oracle score gap", gap, 1.0, 10 * TIE_BAND)
                tied.add(f)
    return tied


def test_r101_ytvis19_end_to_end(monkeypatch):
    """The R101_ytvis19 preset (MSRA R101, 40 classes, 4-frame clips, 30-frame window: one flush at the end) with seeded synthetic
    weights (zero-init trap removed, class bias calibrated as bench.py does) on 6 frames of 360x640: MDQE.forward against the oracle's
    inference_vis with the MSRA restatement as its backbone."""
    from bench import calibrate_synthetic_scores
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.params import random_state
    cfg = PRESETS["R101_ytvis19"]
    fh, fw = 360, 640
    sd = random_state(cfg, seed=0)
    model = MDQE(cfg, state_dict=sd).eval()
    calibrate_synthetic_scores(model, sd, cfg, fh, fw)               # shifts the class bias in sd and in the model alike
    frames = _frames(6)
    hp = _hyper(cfg)
    feats = {}
    frame_features = O.frame_features

    def keep(*a, **k):                                               # the oracle's encoder tokens, for the near-tie check below
        feats["v"] = frame_features(*a, **k)
        return feats["v"]
    monkeypatch.setattr(O, "frame_features", keep)
    trace_o = []
    with torch.no_grad():
        video_o = O.inference_vis(sd, hp, frames, lambda im: resnet_msra(sd, BP, im, 101), trace=trace_o)
    monkeypatch.undo()

    batch = [{"image": frames, "height": fh, "width": fw}]
    out = model(batch)
    trace = []
    with torch.no_grad():
        model.inference_vis(batch, trace=trace)
    group = "R101_ytvis19 6x360x640 f32 direct"
    assert len(trace) == len(trace_o) and sum(int(c["scores"].numel()) for c in trace_o) > len(trace_o)   # >1 instance per clip
    lscale = max(1.0, max(float(c["pred_masks"].abs().max()) for c in trace_o if c["pred_masks"].numel()))
    failed = []
    for res, rc in zip(trace, trace_o):
        try:
            _check_clip(group, res, rc, lscale)
        except AssertionError:
            failed.append(rc["frame_idx"])
    tied = _near_tie_frames(group, sd, hp, feats["v"], model, frames, failed) if failed else set()
    for idx in failed:                                               # a clip off its bars must hold a near-tie cell (as test_fullsize_gpu)
        assert any(f in tied for f in idx), ("clip off the bars without a near-tie", idx)
    record_margin(group, "clips not held to the oracle (a near-tie query cell)", float(len(failed)), 1.0, float(len(trace_o)))
    assert len(failed) <= 1, failed
    assert len(out["pred_masks"]) == len(out["pred_scores"]) == len(out["pred_labels"]) >= 1
    assert out["pred_masks"][0].shape == (len(frames), fh, fw)
    if failed:                                                       # the tracker's inputs differ in that clip: form only
        return
    assert out["pred_labels"] == video_o["pred_labels"]
    _m(group, "video scores", torch.tensor(out["pred_scores"]), torch.tensor(video_o["pred_scores"]), 1e-3)
    got, want = torch.stack(out["pred_masks"]), torch.stack(video_o["pred_masks"])
    assert got.shape == want.shape and got.dtype == torch.bool
    mis = record_margin(group, "final masks: mismatching pixel fraction", float((got != want).float().mean()), 1.0, 1e-3)
    assert mis < 1e-3
