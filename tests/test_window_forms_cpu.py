"""merge.Forms: which output forms a video produces, resolved once.  The table of the offline flags and the online `emit`, row by row,
on stand-in models (one of them without the newer attributes), and the merger's refusals with their messages."""
import itertools
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mdqe_cvpr2023_amd import merge  # noqa: E402
from mdqe_cvpr2023_amd.merge import Forms  # noqa: E402


def _row(f):
    return (f.planes, f.labels, f.overlay, f.plane_geometry, f.label_geometry)


def _model(**kw):
    return types.SimpleNamespace(**kw)


def test_offline_rows():
    for rle, ov, geo in itertools.product((False, True), repeat=3):
        flags = dict(rle_output=rle, overlay_output=ov, geometry_output=geo)
        planes = "rle" if rle else "dense"
        assert _row(Forms.of_model(_model(label_output=True, **flags), emit_masks=False)) == (None, False, False, False, False)
        assert _row(Forms.of_model(_model(label_output=False, **flags))) == (planes, False, ov, geo, False)
        assert _row(Forms.of_model(_model(label_output=True, **flags))) == (planes, True, ov, geo, geo)
        assert _row(Forms.of_model(_model(label_output="only", **flags))) == (None, True, ov, False, geo)
        # rle_output takes the early path whatever early_masks says, with or without planes: the path choice of before
        assert all(Forms.of_model(_model(label_output=lab, **flags)).early_always is rle for lab in (False, True, "only"))
    assert Forms.of_model(_model(rle_output=True), emit_masks=False).early_always is False


def test_online_rows():
    for geo in (False, True):
        assert _row(Forms.of_emit("masks", geo)) == ("dense", False, False, geo, False)
        assert _row(Forms.of_emit("rle", geo)) == ("rle", False, False, geo, False)
        assert _row(Forms.of_emit("labels", geo)) == (None, True, False, False, geo)
        assert _row(Forms.of_emit("overlay", geo)) == (None, True, True, False, geo)
        # geometry=None: the model's flag, for either constructor; a value given wins over it
        model = _model(geometry_output=geo)
        assert _row(Forms.of_emit("labels", None, model)) == (None, True, False, False, geo)
        assert Forms.of_model(model, geometry=not geo).plane_geometry is (not geo)
    with pytest.raises(KeyError):
        Forms.of_emit("pictures")


def test_a_model_without_the_newer_attributes_and_a_frozen_record():
    bare = _model()
    assert _row(Forms.of_model(bare)) == ("dense", False, False, False, False)
    assert _row(Forms.of_model(_model(rle_output=True))) == ("rle", False, False, False, False)
    assert _row(Forms.of_emit("masks", None, bare)) == ("dense", False, False, False, False)
    with pytest.raises(Exception):
        Forms.of_model(bare).labels = True
    assert Forms.of_model(bare) == Forms(planes="dense")


def test_the_merger_reads_its_forms_and_keeps_its_refusals():
    from mdqe_cvpr2023_amd.vis_score import GroundTruth
    gt = GroundTruth(masks=torch.zeros(1, 4, 8, 8, dtype=torch.bool), category_ids=[1])
    args = ((8, 8), (8, 8), (2, 2))
    with pytest.raises(ValueError, match="overlay output needs the frames of the whole video on this device; this path does not hold them"):
        merge.ClipMerger(_model(overlay_output=True), *args, n_frames=4)
    with pytest.raises(ValueError, match="overlay output needs the frames"):
        merge.ClipMerger(_model(), *args, online="overlay")
    with pytest.raises(ValueError, match="ground_truth: it holds 4 frames, the video 5"):
        merge.ClipMerger(_model(), *args, n_frames=5, ground_truth=gt)
    with pytest.raises(ValueError, match="ground_truth: a merger that emits no masks cannot score them"):
        merge.ClipMerger(_model(), *args, n_frames=4, emit_masks=False, ground_truth=gt)
    with pytest.raises(ValueError, match="ground_truth: the overlap counts are a device kernel's; the model is on cpu"):
        merge.ClipMerger(_model(device=torch.device("cpu")), *args, n_frames=4, ground_truth=gt)


def test_a_result_that_asks_for_nothing_touches_no_device():
    """emit_masks=False (ranks > 0 of a sharded video): the head and an empty mask list, no stream, no synchronise -- a stand-in model
    without a device, on a host without a GPU."""
    model = _model(select_tracks=lambda cls_clips: (torch.tensor([0.9, 0.2]), [3, 1], [1, 0]), rle_output=True, label_output=True)
    res = merge.video_result(model, (8, 9), [torch.zeros(2, 4)], [], (8, 8), 4, emit_masks=False)
    assert res == {"image_size": (8, 9), "pred_scores": [pytest.approx(0.9), pytest.approx(0.2)], "pred_labels": [3, 1], "pred_masks": []}
    assert merge.video_result(model, (8, 9), [torch.zeros(2, 4)], [], (8, 8), 4, forms=Forms()) == res
