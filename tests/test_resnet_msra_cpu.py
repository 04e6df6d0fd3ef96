"""CPU: MSRA ResNets (detectron2 MODEL.RESNETS.STRIDE_IN_1X1 True -- a downsampling block's stride on the 1x1 conv1) and the R101
configs that use them (configs/R101_coco.yaml, R101_ytvis19.yaml).

  * from_d2_cfg reads STRIDE_IN_1X1 (absent: False, as before) and refuses the RESNETS options the backbone does not implement;
  * the R101_ytvis19 preset carries the values of its yaml chain;
  * the tests' MSRA restatement (tests/_resnet_msra.py) equals an independent implementation of the same published architecture,
    transformers' ResNetModel with downsample_in_bottleneck=True, within 1e-5 of the activation scale -- R50 and R101."""
import dataclasses
from types import SimpleNamespace as NS

import pytest
import torch

from _resnet_msra import resnet_msra
from mdqe_cvpr2023_amd.config import PRESETS, MDQEConfig, from_d2_cfg
from mdqe_cvpr2023_amd.params import resnet_manifest
from synth import synth_tensor


def _cfg(**resnets):
    """An attribute tree with the keys from_d2_cfg reads (values of configs/R50_ytvis21.yaml); MODEL.RESNETS from the arguments."""
    m = NS(NUM_CLASSES=40, MASK_STRIDE=4, MATCH_STRIDE=4, HIDDEN_DIM=256, NUM_OBJECT_QUERIES=200, WINDOW_INTER_FRAME_ASSOCIATION=7,
           QUERY_EMBED_DIM=64, NHEADS=8, ENC_LAYERS=6, DEC_LAYERS=6, NUM_FEATURE_LEVELS=4, DEC_NUM_POINTS=4, ENC_NUM_POINTS=4,
           DEC_TEMPORAL=True, MLP_RATIO=4, CLIP_STRIDE=1, MERGE_ON_CPU=False, MULTI_CLS_ON=True, APPLY_CLS_THRES=0.1,
           SAMPLING_FRAME_NUM_TEST=4, WINDOW_FRAME_NUM_TEST=30, MAX_NUM_INSTANCES=70)
    return NS(INPUT=NS(SAMPLING_FRAME_NUM=4, MIN_SIZE_TEST=360), DATASETS=NS(TEST=("ytvis_2019_val",)), TEST=NS(DETECTIONS_PER_IMAGE=10),
              MODEL=NS(DEVICE="cuda", PIXEL_MEAN=[123.675, 116.280, 103.530], PIXEL_STD=[58.395, 57.120, 57.375], MDQE=m,
                       RESNETS=NS(**resnets), BACKBONE=NS(NAME="build_resnet_backbone")))


def test_stride_in_1x1_is_read():
    c = from_d2_cfg(_cfg(DEPTH=101, STRIDE_IN_1X1=True))
    assert c.backbone == "R101" and c.stride_in_1x1 is True
    c = from_d2_cfg(_cfg(DEPTH=50, STRIDE_IN_1X1=False))
    assert c.backbone == "R50" and c.stride_in_1x1 is False


def test_absent_stride_in_1x1_keeps_the_old_meaning():
    assert from_d2_cfg(_cfg(DEPTH=50)).stride_in_1x1 is False
    assert from_d2_cfg(_cfg(DEPTH=101)).stride_in_1x1 is False
    assert MDQEConfig().stride_in_1x1 is False


def test_detectron2_defaults_pass():
    """detectron2's own defaults of the refused keys (get_cfg(): MODEL.RESNETS.*) are exactly what the backbone implements."""
    c = from_d2_cfg(_cfg(DEPTH=101, STRIDE_IN_1X1=True, NUM_GROUPS=1, WIDTH_PER_GROUP=64, RES5_DILATION=1, NORM="FrozenBN",
                         STEM_OUT_CHANNELS=64, RES2_OUT_CHANNELS=256, DEFORM_ON_PER_STAGE=[False, False, False, False]))
    assert c.backbone == "R101" and c.stride_in_1x1 is True


@pytest.mark.parametrize("key,value", [("DEPTH", 18), ("DEPTH", 152), ("NUM_GROUPS", 32), ("WIDTH_PER_GROUP", 8), ("RES5_DILATION", 2),
                                       ("DEFORM_ON_PER_STAGE", [False, True, True, True]), ("NORM", "SyncBN"), ("NORM", "BN"),
                                       ("STEM_OUT_CHANNELS", 128), ("RES2_OUT_CHANNELS", 64)])
def test_unimplemented_resnet_options_are_refused(key, value):
    rn = {"DEPTH": 50, key: value}
    with pytest.raises(ValueError, match="RESNETS.%s" % key):
        from_d2_cfg(_cfg(**rn))


def test_swin_configs_skip_the_resnet_check():
    cfg = _cfg(DEPTH=18, NORM="BN")                                       # a ResNet tree a Swin config carries but does not use
    cfg.MODEL.BACKBONE = NS(NAME="build_swinv2_backbone")
    cfg.MODEL.SWIN = NS(EMBED_DIM=192, DEPTHS=[2, 2, 18, 2], NUM_HEADS=[6, 12, 24, 48], WINDOW_SIZE=12, MLP_RATIO=4.0)
    c = from_d2_cfg(cfg)
    assert c.backbone == "SwinV2" and c.stride_in_1x1 is False


def test_r101_ytvis19_preset_matches_its_yaml_chain():
    """configs/R101_ytvis19.yaml -> R50_ytvis19.yaml -> R50_ytvis21.yaml -> R50_coco.yaml, read through from_d2_cfg, field by field."""
    c = from_d2_cfg(_cfg(DEPTH=101, STRIDE_IN_1X1=True))
    p = PRESETS["R101_ytvis19"]
    diff = {f.name: (getattr(c, f.name), getattr(p, f.name)) for f in dataclasses.fields(p) if getattr(c, f.name) != getattr(p, f.name)}
    assert not diff, diff
    assert (p.backbone, p.stride_in_1x1, p.num_classes, p.window_inter_frame_asso, p.n_max_inst) == ("R101", True, 40, 7, 70)
    assert (p.n_frames_test, p.n_frames_window_test, p.apply_cls_thres, p.min_size_test, p.detections_per_image) == (4, 30, 0.1, 360, 10)
    assert p.is_coco is False and p.merge_on_cpu is False


def test_existing_presets_keep_the_stride_on_the_3x3():
    for name in ("R50_ovis_360", "R50_ovis_720", "swinl_ovis"):
        assert PRESETS[name].stride_in_1x1 is False


def _hf_state(sd, p):
    """detectron2 names -> transformers names."""
    out = {}

    def unit(src, dst):
        out[dst + ".convolution.weight"] = sd[src + ".weight"]
        for a in ("weight", "bias", "running_mean", "running_var"):
            out[dst + ".normalization." + a] = sd[src + ".norm." + a]
        out[dst + ".normalization.num_batches_tracked"] = torch.tensor(0)
    unit(p + ".stem.conv1", "embedder.embedder")
    for k in sd:
        if k.startswith(p + ".res") and k.endswith(".weight") and ".norm." not in k:
            parts = k[len(p) + 1:].split(".")                                  # resS.B.convN|shortcut.weight
            s, b, name = int(parts[0][3:]) - 2, int(parts[1]), parts[2]
            dst = f"encoder.stages.{s}.layers.{b}." + ("shortcut" if name == "shortcut" else f"layer.{int(name[4:]) - 1}")
            unit(k[:-len(".weight")], dst)
    return out


@pytest.mark.parametrize("kind,depths", [("R50", [3, 4, 6, 3]), ("R101", [3, 4, 23, 3])])
def test_msra_restatement_equals_an_independent_implementation(kind, depths):
    transformers = pytest.importorskip("transformers")
    p = "detr.backbone.0.backbone"
    sd = {k: synth_tensor(k, s, 3) for k, s in resnet_manifest(kind, p).items()}
    cfg = transformers.ResNetConfig(num_channels=3, embedding_size=64, hidden_sizes=[256, 512, 1024, 2048], depths=depths,
                                    layer_type="bottleneck", hidden_act="relu", downsample_in_first_stage=False,
                                    downsample_in_bottleneck=True)
    hf = transformers.ResNetModel(cfg).eval()
    res = hf.load_state_dict(_hf_state(sd, p), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 96, 160, generator=g)
    with torch.no_grad():
        ours = resnet_msra(sd, p, x, int(kind[1:]))
        hs = hf(x, output_hidden_states=True).hidden_states                    # (stem, res2, res3, res4, res5)
    for o, r in zip(ours, hs[2:]):
        assert o.shape == r.shape
        assert float((o - r).abs().max()) <= 1e-5 * float(r.abs().max()), (kind, float((o - r).abs().max()), float(r.abs().max()))
