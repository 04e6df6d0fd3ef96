"""Decoder surfaces as video input on the device: the conversion kernel (mdqe_yuv420sp_to_rgb_u8 through preprocess.yuv_to_rgb) against
the numpy oracle (tests/_yuv_ref.py), and the model's surfaces above it -- forward() and the online session on a YuvFrames against the
same call on the converted tensor.  Integers only: every comparison is torch.equal, there is no tolerance.

Kernel cases: per (shape, format) ONE content and its 8 references (matrix x range x order); the content is packed into 14 layouts -- the
tight pitch, a 256-aligned one and an unaligned one (odd for NV12: 39 bytes for W = 37), the chroma plane right behind the luma rows
and at the height rounded up to 32, surfaces back to back and 5 rows apart, and the allocation entered 1 (NV12) and 4 bytes late, so
that the 16-byte, the 4-byte and the per-sample form are each chosen and each refused by some launch.  NI = 3 everywhere.  The output
lies between guard frames of 0xAB; the input allocation, padding included, must be unchanged.
"""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import _yuv_ref as REF  # noqa: E402

SHAPES = [(1, 1), (2, 2), (1, 33), (19, 37), (32, 64), (33, 131), (64, 1040)]
NI = 3


def _layouts(H, W, fmt):
    """(pitch, chroma_row, extra_rows, lead) of every packing of one content."""
    tight = REF.tight_pitch(W, fmt)
    pitches = (tight, (tight + 255) // 256 * 256, tight + (1 if fmt == "nv12" else 2))
    crows = (H, (H + 31) // 32 * 32)
    out = [(p, c, e, 0) for p in pitches for c in crows for e in (0, 5)]
    out += [(pitches[1], crows[1], 5, lead) for lead in ((1, 4) if fmt == "nv12" else (4, 8))]
    return out


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_equals_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd.preprocess import YuvFrames, yuv_to_rgb
    ys, cs = REF.make_content(H * 1000 + W, NI, H, W, fmt)
    combos = [(m, f, o) for m in ("bt601", "bt709") for f in (False, True) for o in ("rgb", "bgr")]
    want = {c: torch.from_numpy(REF.convert(ys, cs, H, W, fmt, *c)) for c in combos}
    assert torch.equal(want[combos[0]].flip(1), want[combos[1]])
    launches = 0
    for pitch, crow, extra, lead in _layouts(H, W, fmt):
        flat, rows = REF.pack(ys, cs, fmt, pitch, crow, extra, lead)
        host = torch.from_numpy(flat)
        dev = host.cuda()
        for full_pitch in (True, False):
            y, uv = REF.plane_views(dev, NI, H, W, fmt, pitch, crow, rows, lead, full_pitch=full_pitch)
            for c in combos if full_pitch else combos[:1]:
                s = YuvFrames(y, uv, H, W, fmt=fmt, matrix=c[0], full_range=c[1], order=c[2])
                out = torch.full((1 + NI + 1, 3, H, W), 0xAB, dtype=torch.uint8, device="cuda")
                got = yuv_to_rgb(s, out=out[1:1 + NI])
                o = out.cpu()
                assert got.data_ptr() == out[1].data_ptr()
                assert torch.equal(o[1:1 + NI], want[c]), (pitch, crow, extra, lead, c)
                assert bool((o[0] == 0xAB).all()) and bool((o[-1] == 0xAB).all()), (pitch, crow, extra, lead, c)
                launches += 1
        assert torch.equal(dev.cpu(), host), (pitch, crow, extra, lead)
    # the output the wrapper allocates itself; one surface; no surface
    y, uv = REF.plane_views(dev, NI, H, W, fmt, pitch, crow, rows, lead)
    s = YuvFrames(y, uv, H, W, fmt=fmt, matrix="bt601")
    got = yuv_to_rgb(s)
    assert got.is_cuda and got.is_contiguous() and got.dtype == torch.uint8 and torch.equal(got.cpu(), want[("bt601", False, "rgb")])
    assert torch.equal(yuv_to_rgb(s[1:2]).cpu(), want[("bt601", False, "rgb")][1:2])
    assert tuple(yuv_to_rgb(s[3:]).shape) == (0, 3, H, W)
    assert launches == 14 * 9


def test_host_planes_convert_on_the_host_and_device_planes_on_the_device_to_the_same_bits():
    from mdqe_cvpr2023_amd.preprocess import YuvFrames, yuv_to_rgb
    H, W = 33, 131
    for fmt in ("nv12", "p010"):
        ys, cs = REF.make_content(9, 2, H, W, fmt)
        flat, rows = REF.pack(ys, cs, fmt, 512, 64, 3)
        host = torch.from_numpy(flat)
        a = yuv_to_rgb(YuvFrames(*REF.plane_views(host, 2, H, W, fmt, 512, 64, rows), H, W, fmt=fmt))
        b = yuv_to_rgb(YuvFrames(*REF.plane_views(host.cuda(), 2, H, W, fmt, 512, 64, rows), H, W, fmt=fmt))
        assert not a.is_cuda and b.is_cuda and torch.equal(a, b.cpu())


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


L, OUT = 17, (90, 150)


def _surfaces(h, w, fmt, pitch, crow, device, **kw):
    """The synthetic video as decoder surfaces: luma from its green plane, chroma from its sub-sampled red and blue planes (a picture
    with moving objects, which is all the model needs), in ONE allocation of [L, crow + ceil(h/2) + 2, pitch] with poison padding."""
    from bench import synth_video
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    v = synth_video(0, L, seed=1, h=h, w=w, n_obj=4).numpy().astype(np.int64)
    ys = v[:, 1]
    cs = np.stack([v[:, 0, ::2, ::2], v[:, 2, ::2, ::2]], -1).reshape(L, (h + 1) // 2, -1)
    if fmt == "p010":
        ys, cs = (ys << 8) | 0x2A, (cs << 8) | 0x15                 # (8-bit values in the top byte, something in the low 6 bits)
    dt = np.uint8 if fmt == "nv12" else np.uint16
    flat, rows = REF.pack(ys.astype(dt), cs.astype(dt), fmt, pitch, crow, extra_rows=2)
    t = torch.from_numpy(flat)
    t = t if fmt == "nv12" else t.view(torch.int16)
    buf = t.view(L, rows, -1).to(device)
    return YuvFrames.from_surface(buf, h, w, crow, fmt=fmt, **kw)


def _same(a, b, path="result"):
    assert type(a) is type(b), path
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), path
    else:
        assert a == b, path


def _forward_pair(model, s, keys=None):
    from mdqe_cvpr2023_amd.preprocess import yuv_to_rgb
    Ho, Wo = OUT
    rgb = yuv_to_rgb(s)
    want = model([{"image": rgb.to(model.device), "height": Ho, "width": Wo}])
    got = model([{"image": s, "height": Ho, "width": Wo}])
    _same(got, want)
    assert len(want["pred_scores"]) > 0
    if keys is not None:
        assert keys <= set(want)
    return want


@pytest.mark.parametrize("where", ["host", "device"])
def test_forward_on_surfaces_equals_forward_on_the_converted_frames(small, where):
    cfg, model = small
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda" if where == "device" else "cpu")
    before = s.y.clone(), s.uv.clone()
    want = _forward_pair(model, s, {"pred_masks"})
    assert want["image_size"] == OUT and any(bool(m.any()) for m in want["pred_masks"])
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])


@pytest.mark.parametrize("where", ["host", "device"])
def test_forward_with_overlay_paints_on_the_converted_frames(small, where):
    cfg, model = small
    s = _surfaces(96, 160, "nv12", 160, 96, "cuda" if where == "device" else "cpu", matrix="bt601", full_range=True, order="bgr")
    model.overlay_output = True
    try:
        want = _forward_pair(model, s, {"pred_overlay", "pred_track_ids"})
    finally:
        model.overlay_output = False
    pic = want["pred_overlay"]
    assert tuple(pic.shape) == (L,) + OUT + (3,) and int(pic.max()) > 0


@pytest.mark.parametrize("where", ["host", "device"])
def test_forward_with_resize_on_device_resizes_the_converted_frames(small, where):
    cfg, model = small
    s = _surfaces(120, 200, "nv12", 256, 128, "cuda" if where == "device" else "cpu")
    model.resize_on_device = True
    try:
        want = _forward_pair(model, s, {"pred_masks"})
        # and the resize really ran: the same surfaces without it give other scores
        model.resize_on_device = False
        other = model([{"image": s, "height": OUT[0], "width": OUT[1]}])
    finally:
        model.resize_on_device = False
    assert other["pred_scores"] != want["pred_scores"]


def test_forward_stream_over_surfaces_equals_forward(small):
    """Two videos of surfaces (host planes, then device planes) through forward_stream(), whose look-ahead starts the second video's
    conversion under the first one's tail: each result equals forward() on that video and forward() on its converted frames."""
    from mdqe_cvpr2023_amd.preprocess import yuv_to_rgb
    cfg, model = small
    Ho, Wo = OUT
    vids = [_surfaces(96, 160, "nv12", 256, 128, "cpu"), _surfaces(96, 160, "nv12", 160, 96, "cuda", matrix="bt601", full_range=True)]
    got = list(model.forward_stream([[{"image": s, "height": Ho, "width": Wo}] for s in vids]))
    assert len(got) == 2
    for s, g in zip(vids, got):
        _same(g, model([{"image": s, "height": Ho, "width": Wo}]))
        _same(g, model([{"image": yuv_to_rgb(s).to(model.device), "height": Ho, "width": Wo}]))
    assert got[0]["pred_scores"] != got[1]["pred_scores"] or not all(torch.equal(a, b) for a, b in zip(got[0]["pred_masks"], got[1]["pred_masks"]))


def test_forward_on_p010_surfaces(small):
    cfg, model = small
    for where in ("cpu", "cuda"):
        _forward_pair(model, _surfaces(96, 160, "p010", 512, 96, where), {"pred_masks"})


def test_online_overlay_session_on_surfaces_equals_the_converted_frames_and_forward(small):
    from mdqe_cvpr2023_amd.preprocess import yuv_to_rgb
    cfg, model = small
    Ho, Wo = OUT
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda", order="bgr")
    rgb = yuv_to_rgb(s)

    def session(feed):
        ov = model.online_video(height=Ho, width=Wo, emit="overlay", keep=True)
        wins = []
        for a in range(0, L, 5):
            wins += ov.push(feed[a:a + 5])
            assert ov.frames_held <= (a + 5) + 4
        wins += ov.close()
        return wins, ov.result()
    wy, ry = session(s)
    wr, rr = session(rgb)
    _same(ry, rr)
    assert [w.frames for w in wy] == [w.frames for w in wr] == [(0, 6), (6, 12), (12, 17)]
    for a, b in zip(wy, wr):
        assert a.track_ids == b.track_ids
        _same(a.cls_probs, b.cls_probs)
        _same(a.labels, b.labels)
        _same(a.overlay, b.overlay)
    model.overlay_output, model.label_output = True, True
    try:
        ref = model([{"image": s, "height": Ho, "width": Wo}])
    finally:
        model.overlay_output, model.label_output = False, False
    assert torch.equal(ry["pred_overlay"], ref["pred_overlay"]) and torch.equal(ry["pred_label_map"], ref["pred_label_map"])
    assert ry["pred_scores"] == ref["pred_scores"] and ry["pred_labels"] == ref["pred_labels"]
    # host surfaces pushed into a session of another emit: the same windows
    sh = _surfaces(96, 160, "nv12", 256, 128, "cpu", order="bgr")
    ov = model.online_video(height=Ho, width=Wo, emit="labels", keep=True)
    wl = []
    for a in range(0, L, 5):
        wl += ov.push(sh[a:a + 5])
    wl += ov.close()
    assert all(torch.equal(a.labels, b.labels) for a, b in zip(wl, wy)) and len(wl) == len(wy)


def test_a_push_of_another_size_raises(small):
    cfg, model = small
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda")
    ov = model.online_video(height=OUT[0], width=OUT[1])
    ov.push(s[:3])
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    with pytest.raises(RuntimeError, match="differs from the first push"):
        ov.push(YuvFrames(s.y[3:5, :94], s.uv[3:5, :47], 94, 160))
    with pytest.raises(RuntimeError, match="differs from the first push"):
        ov.push(YuvFrames(s.y[3:5], s.uv[3:5], 96, 158))
    with pytest.raises(RuntimeError, match="differs from the first push"):
        ov.push(torch.zeros(2, 3, 96, 158, dtype=torch.uint8, device="cuda"))
    ov.push(s[3:5])                                                   # the session goes on


def test_the_sharded_driver_and_a_coco_config_refuse_surfaces(small):
    from mdqe_cvpr2023_amd import sharding
    cfg, model = small
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda")
    plan = sharding.chunk_plan(L, cfg.n_frames_test, cfg.clip_stride, L)
    with pytest.raises(ValueError, match="YuvFrames"):
        sharding.run_round_robin(model, {0: s}, plan, 0, 1, None, OUT)
    _, image_model = _model(is_coco=True)
    with pytest.raises(ValueError, match="YuvFrames"):
        image_model([{"image": s[:cfg.n_frames], "height": OUT[0], "width": OUT[1]}])
