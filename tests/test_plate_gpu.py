"""Object removal on the device: the four kernels of csrc/plate.hip (ops.plate_update, ops.plate_update_yuv, ops.plate_picture,
ops.plate_picture_yuv) against the numpy rule (tests/_plate_ref.py), and the style above them: forward() with
Style(replace="tracks", backdrop="plate") and online_video(style=...), RGB pictures and NV12 surfaces.  Integers only: every comparison
is exact.

Kernel shapes: the picture kernel's tile is 16 x 64 cells, so 19 x 70 and 37 x 150 cross tile borders both ways with ragged edges; the
surfaces are 19 x 71 (odd both ways: chroma pairs with 1 and 2 in-picture pixels) and 37 x 150."""
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

import _grow_ref as GREF  # noqa: E402
import _matte_ref as MREF  # noqa: E402
import _overlay_ref as OREF  # noqa: E402
import _plate_ref as REF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402
from test_matte_gpu import _Logits  # noqa: E402
from test_overlay_gpu import L, OUT, PLANS, _forward, _model, _online, _same  # noqa: E402
from test_overlay_yuv_gpu import _layouts, _raw, _session, _surfaces  # noqa: E402
from test_overlay_yuv_gpu import _frames as _yuv_frames  # noqa: E402

SHAPES = [(19, 70), (37, 150)]
F = 5
EVERY = np.ones(256, dtype=np.uint8)
SENTINEL = 0xCD


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _start(seed, h, w, C, top, N):
    """A state in mid-video: counts 0..N (so the default N saturates too), P = 0 where nothing has been seen."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, N + 1, size=(h, w))
    P = rng.integers(0, 256 * top + 1, size=(h, w, C))
    P[n == 0] = 0
    return P.astype(np.int64), n.astype(np.int64)


def _rgb_frames(kind, s, seed):
    """Frames whose source values on the output grid can go wrong, and those values: "u8" / "f32" at the output's size (made from s),
    "u8 small" / "f32 small" at 11 x 40 (nearest-sampled).  float32 frames hold a NaN, values far out of range and halves."""
    Fn, Ho, Wo, _ = s.shape
    rng = np.random.default_rng(seed)
    if "small" in kind:
        fr = rng.integers(0, 256, size=(Fn, 3, 11, 40))
    else:
        fr = np.ascontiguousarray(np.moveaxis(s, -1, 1))
    if kind.startswith("f32"):
        fr = fr.astype(np.float32) + rng.choice(np.array([0.0, 0.25, -0.25, 0.5, -0.5], dtype=np.float32), size=fr.shape)
        fr[0, 0, 0, 0], fr[1, 1, 2, 3], fr[2, 2, 4, 5], fr[3, 0, 5, 7] = np.nan, 1e9, -1e9, 255.5
        fr[:, :, 6, :8] = np.array([-0.5, 0.5, 1.5, 2.5, 254.5, 255.49, 256.0, np.inf], dtype=np.float32)
    else:
        fr = fr.astype(np.uint8)
    return fr, OREF.source_values(fr, Fn, Ho, Wo)


# ---- the update kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "u8 small", "f32", "f32 small"])
@pytest.mark.parametrize("shape", SHAPES)
def test_update_against_the_reference(shape, kind):
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = shape
    for N in (1, 2, 3, 64):
        s0, block = REF.update_case(Ho * Wo + N, F, Ho, Wo, 3, 255, N)
        fr, s = _rgb_frames(kind, s0, N)
        # (a block map made by the margin: the generated one grown by 2 pixels, every label growing)
        for blk in (block, GREF.grow(block, EVERY, 2)):
            REF.check_update_case(s, blk, N)
            for start in (REF.fresh(Ho, Wo, 3), _start(N, Ho, Wo, 3, 255, N)):
                stats = {}
                want = REF.to_state(*REF.update(*start, s, blk == 0, N, stats))
                assert N != 64 or start[1].max() == 0 or stats["saturated"] > 0     # (the default N saturates from a state in mid-video)
                fr_dev, blk_dev = _dev(fr), _dev(blk)
                st = _dev(REF.to_state(*start))
                assert ops.plate_update(st, fr_dev, blk_dev, N) is st
                got = st.cpu().numpy()
                assert np.array_equal(got, want), (shape, kind, N, int((got != want).sum()))
                # two calls of 3 + 2 frames, the second on a view into the store: the same state; and runs are identical
                two = _dev(REF.to_state(*start))
                ops.plate_update(two, fr_dev[:3], blk_dev[:3], N)
                ops.plate_update(two, fr_dev[3:], blk_dev[3:], N)
                again = ops.plate_update(_dev(REF.to_state(*start)), fr_dev, blk_dev, N)
                assert torch.equal(two, st) and torch.equal(again, st)
    # frames a stride apart (a view into a larger store), and no frames: nothing changes
    store = torch.zeros(F, 4, Ho, Wo, dtype=torch.uint8, device="cuda")
    store[:, :3] = _dev(np.moveaxis(s0, -1, 1).astype(np.uint8))
    st = _dev(REF.to_state(*REF.fresh(Ho, Wo, 3)))
    ops.plate_update(st, store[:, :3], _dev(block), 64)
    assert np.array_equal(st.cpu().numpy(), REF.to_state(*REF.update(*REF.fresh(Ho, Wo, 3), s0, block == 0, 64)))
    before = st.clone()
    ops.plate_update(st, store[:0, :3], _dev(block[:0]), 64)
    assert torch.equal(st, before)


def _surface_case(H, W, fmt, N, seed):
    """Surfaces, a block map and the planes' observed values: (ys, cs stored samples, block, luma values [F, H, W, 1], chroma values
    [F, ch, cw, 2])."""
    ys, cs = YREF.make_content(seed, F, H, W, fmt)
    _, block = REF.update_case(seed, F, H, W, 1, 255, N)
    sh = 6 if fmt == "p010" else 0
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return ys, cs, block, (ys.astype(np.int64) >> sh)[..., None], (cs.astype(np.int64) >> sh).reshape(F, ch, cw, 2)


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(19, 71), (37, 150)])
def test_update_yuv_against_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops
    top = 255 if fmt == "nv12" else 1023
    ch, cw = (H + 1) // 2, (W + 1) // 2
    for N in (1, 3, 64):
        ys, cs, block, sy, sc = _surface_case(H, W, fmt, N, H * W + N)
        for blk in (block, GREF.grow(block, EVERY, 3)):
            obs_c = REF.observed_chroma(blk)
            REF.check_update_case(sy, blk, N)
            assert obs_c.any() and not obs_c.all()
            for k, (pitch, crow, extra, lead) in enumerate(_layouts(H, W, fmt)):
                start_y, start_c = (REF.fresh(H, W, 1), REF.fresh(ch, cw, 2)) if k == 0 else (_start(k, H, W, 1, top, N), _start(k + 9, ch, cw, 2, top, N))
                want_y = REF.to_state(*REF.update(*start_y, sy, blk == 0, N))
                want_c = REF.to_state(*REF.update(*start_c, sc, obs_c, N))
                flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
                src = _yuv_frames(_dev(flat), F, H, W, fmt, pitch, crow, rows, lead)
                py, pc, blk_dev = _dev(REF.to_state(*start_y)), _dev(REF.to_state(*start_c)), _dev(blk)
                assert ops.plate_update_yuv(py, pc, src, blk_dev, N) == (py, pc)
                assert np.array_equal(py.cpu().numpy(), want_y) and np.array_equal(pc.cpu().numpy(), want_c), (H, W, fmt, N, k)
                ty, tc = _dev(REF.to_state(*start_y)), _dev(REF.to_state(*start_c))
                ops.plate_update_yuv(ty, tc, src[:3], blk_dev[:3], N)
                ops.plate_update_yuv(ty, tc, src[3:], blk_dev[3:], N)
                assert torch.equal(ty, py) and torch.equal(tc, pc)
    ops.plate_update_yuv(py, pc, src[:0], blk_dev[:0], N)             # no surfaces: nothing changes
    assert np.array_equal(py.cpu().numpy(), want_y)


# ---- the picture kernels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES + [(1, 3), (16, 64), (17, 65)])
def test_picture_against_the_reference_at_every_alignment(shape):
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = shape
    cases = REF.picture_cases(Ho + Wo, Ho, Wo, 3, 255) if Ho > 4 else {"one row": (np.array([[[0] * 3, [25600, 300, 65280], [0] * 3]]), np.array([[0, 4, 0]]))}
    fill = (3, 250, 77)
    fill_dev = torch.tensor(fill, dtype=torch.uint8, device="cuda")
    n_bytes = Ho * Wo * 3
    for k, (name, (P, n)) in enumerate(cases.items()):
        st = _dev(REF.to_state(P, n))
        for j, reach in enumerate((0, 1, 5, 32)):
            want = REF.picture(P, n, reach, fill).astype(np.uint8)
            if name == "holes" and Ho == 19 and reach == 5:
                assert np.array_equal(REF.sources(n, reach), REF.sources_pixelwise(n, reach))
            shift = (k + j) % 4                                       # every 1..3-byte misalignment, and none
            raw = torch.full((n_bytes + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
            out = raw[shift:shift + n_bytes].view(Ho, Wo, 3)
            assert ops.plate_picture(st, fill_dev, reach, out) is out
            r = raw.cpu()
            assert bool((r[:shift] == SENTINEL).all()) and bool((r[shift + n_bytes:] == SENTINEL).all())
            got = r[shift:shift + n_bytes].view(Ho, Wo, 3).numpy()
            assert np.array_equal(got, want), (shape, name, reach, shift, int((got != want).sum()))
            again = ops.plate_picture(st, fill_dev, reach)            # a fresh output: identical from run to run
            assert again is not out and torch.equal(again, out)
            if name == "seen everywhere":
                assert np.array_equal(got, ((P + 128) >> 8).astype(np.uint8))
            if name == "nothing seen":
                assert (got == np.array(fill, dtype=np.uint8)).all()
    assert torch.equal(st, _dev(REF.to_state(P, n)))                  # the state is read only


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_every_misalignment_of_the_picture_with_a_search(shift):
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 19, 70
    P, n = REF.picture_cases(7, Ho, Wo, 3, 255)["holes"]
    fill_dev = torch.tensor((9, 8, 7), dtype=torch.uint8, device="cuda")
    raw = torch.full((Ho * Wo * 3 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = raw[shift:shift + Ho * Wo * 3].view(Ho, Wo, 3)
    assert out.data_ptr() % 4 == shift
    ops.plate_picture(_dev(REF.to_state(P, n)), fill_dev, 5, out)
    assert np.array_equal(out.cpu().numpy(), REF.picture(P, n, 5, (9, 8, 7)).astype(np.uint8))
    assert bool((raw[:shift] == SENTINEL).all()) and bool((raw[shift + Ho * Wo * 3:] == SENTINEL).all())


@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(19, 71), (37, 150)])
def test_picture_yuv_against_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops
    top, sh = (255, 0) if fmt == "nv12" else (1023, 6)
    dt = np.uint8 if fmt == "nv12" else np.uint16
    ch, cw = (H + 1) // 2, (W + 1) // 2
    luma, chroma = REF.picture_cases(H + W, H, W, 1, top), REF.picture_cases(H * W, ch, cw, 2, top)
    fill = np.array([top - 3, 5, top], dtype=np.int64)
    fill_dev = torch.from_numpy((fill | (0xFC00 if fmt == "nv12" else 0x0400)).astype(np.uint16).view(np.int16)).view(torch.uint16).cuda()      # (only the 8 / 10 bits count)
    for k, name in enumerate(luma):
        (Py, ny), (Pc, nc) = luma[name], chroma[name]
        py, pc = _dev(REF.to_state(Py, ny)), _dev(REF.to_state(Pc, nc))
        pitch, crow, extra, lead = _layouts(H, W, fmt)[k % 3]
        for reach in (0, 1, 5, 32):
            wy = (REF.picture(Py, ny, reach, fill[:1])[..., 0] << sh).astype(dt)
            wc = (REF.picture(Pc, nc, (reach + 1) // 2, fill[1:]).reshape(ch, 2 * cw) << sh).astype(dt)
            want, rows = YREF.pack(wy[None], wc[None], fmt, pitch, crow, extra, lead)
            flat = torch.full((want.size,), YREF.POISON, dtype=torch.uint8, device="cuda")
            out = _yuv_frames(flat, 1, H, W, fmt, pitch, crow, rows, lead)
            assert ops.plate_picture_yuv(py, pc, fill_dev, out, reach) is out
            got = flat.cpu().numpy()                                  # the whole allocation: padding is never written
            assert np.array_equal(got, want), (H, W, fmt, name, reach, int((got != want).sum()))
            flat2 = torch.full((want.size,), YREF.POISON, dtype=torch.uint8, device="cuda")
            ops.plate_picture_yuv(py, pc, fill_dev, _yuv_frames(flat2, 1, H, W, fmt, pitch, crow, rows, lead), reach)
            assert torch.equal(flat2, flat)


def test_a_still_background_behind_a_moving_square_comes_back_exactly():
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 19, 70
    rng = np.random.default_rng(5)
    scene = rng.integers(0, 256, size=(3, Ho, Wo)).astype(np.uint8)
    block = REF.moving_square(F, Ho, Wo)
    frames = np.repeat(scene[None], F, 0)
    frames[np.repeat((block != 0)[:, None], 3, 1)] = 255              # the object, wherever it stands
    fill = torch.zeros(3, dtype=torch.uint8, device="cuda")
    for N in (1, 2, 64):
        st = torch.zeros(Ho, Wo, 4, dtype=torch.int32, device="cuda")
        ops.plate_update(st, _dev(frames[:1]), _dev(block[:1]), N)
        first = ops.plate_picture(st, fill, 0).cpu().numpy()
        hidden = block[0] != 0
        assert not first[hidden].any() and np.array_equal(first[~hidden], np.moveaxis(scene, 0, -1)[~hidden])
        ops.plate_update(st, _dev(frames[1:]), _dev(block[1:]), N)
        assert np.array_equal(ops.plate_picture(st, fill, 0).cpu().numpy(), np.moveaxis(scene, 0, -1))      # once uncovered, exactly the scene
        assert np.array_equal(st[..., 3].cpu().numpy(), np.minimum((block == 0).sum(0), N))
    # and on surfaces
    ys, cs = YREF.make_content(3, 1, Ho, Wo, "p010")
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    src = YuvFrames(_dev(np.repeat(ys, F, 0).view(np.int16)), _dev(np.repeat(cs, F, 0).view(np.int16)), Ho, Wo, fmt="p010")
    py, pc = torch.zeros(Ho, Wo, 2, dtype=torch.int32, device="cuda"), torch.zeros(10, 35, 4, dtype=torch.int32, device="cuda")
    ops.plate_update_yuv(py, pc, src, _dev(block), 2)
    out = ops.plate_picture_yuv(py, pc, torch.zeros(3, dtype=torch.int16, device="cuda").view(torch.uint16), YuvFrames.empty(1, Ho, Wo, fmt="p010", device="cuda"), 0)
    assert np.array_equal(_raw(out.y, "p010")[0], ys[0] >> 6 << 6) and np.array_equal(_raw(out.uv, "p010")[0], cs[0] >> 6 << 6)


def test_device_refusals_and_empty_pictures():
    from mdqe_cvpr2023_amd import ops
    st = torch.zeros(6, 9, 4, dtype=torch.int32, device="cuda")
    fill = torch.zeros(3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="plate_picture: fill must be a CUDA tensor"):
        ops.plate_picture(st, fill.cpu())
    with pytest.raises(RuntimeError, match="plate_update: block must be a CUDA tensor"):
        ops.plate_update(st, torch.zeros(1, 3, 6, 9, dtype=torch.uint8, device="cuda"), torch.zeros(1, 6, 9, dtype=torch.uint8))
    # the state may not be an input or the output: refused by the library, nothing launched
    as_bytes = st.view(torch.uint8).view(-1)
    with pytest.raises(RuntimeError, match="plate_picture"):
        ops.plate_picture(st, fill, 4, as_bytes[:6 * 9 * 3].view(6, 9, 3))
    with pytest.raises(RuntimeError, match="plate_update"):
        ops.plate_update(st, torch.zeros(1, 3, 6, 9, dtype=torch.uint8, device="cuda"), as_bytes[:54].view(1, 6, 9))
    assert not st.any()
    empty = torch.zeros(0, 9, 4, dtype=torch.int32, device="cuda")
    assert tuple(ops.plate_picture(empty, fill).shape) == (0, 9, 3)
    assert ops.plate_update(empty, torch.zeros(2, 3, 4, 4, dtype=torch.uint8, device="cuda"), torch.zeros(2, 0, 9, dtype=torch.uint8, device="cuda")) is empty


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class _PlateSpy:
    """Records what the plate ops and the compositing painters are handed: per call the name and clones of the tensors that matter."""

    def __init__(self, monkeypatch):
        from mdqe_cvpr2023_amd import ops
        self.calls = []
        for name in ("grow_labels", "plate_update", "plate_update_yuv", "plate_picture", "plate_picture_yuv", "render_replace", "render_replace_yuv"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, real):
        def fn(*a, **kw):
            r = real(*a, **kw)
            keep = {}
            if name == "render_replace":
                keep = {"labels": a[0].clone(), "matte": a[4].clone(), "back": a[5].clone(), "back_ptr": a[5].data_ptr(), "k": len(a[1])}
            elif name == "render_replace_yuv":
                keep = {"labels": a[0].clone(), "matte": a[4].clone(), "back": a[5].clone() if hasattr(a[5], "uv") else a[5], "k": len(a[1]),
                        "back_ptr": a[5].y.data_ptr() if hasattr(a[5], "uv") else a[5].data_ptr()}
            elif name.startswith("plate_update"):
                keep = {"state_ptr": a[0].data_ptr()}
            self.calls.append((name, keep))
            return r
        return fn

    def take(self):
        c, self.calls = self.calls, []
        return c


@pytest.fixture(scope="module")
def video():
    """The fixture of test_matte_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5 frames, many tracks; the runs with
    replace="tracks" on a colour, and the windows' class rows from an online session."""
    from bench import synth_video
    from mdqe_cvpr2023_amd.render import Style
    _, model = _model(n_frames_window_test=6, apply_cls_thres=1e-6)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    base = {early: _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=Style(replace="tracks"))
            for early in (True, False)}
    _, wins, _ = _online(model, frames, [L], emit="labels")
    rows = [(w.frames, w.cls_probs) for w in wins]
    assert [f for f, _ in rows] == [(0, 6), (6, 12), (12, 17)]
    return model, frames, base, rows


def _styles():
    from mdqe_cvpr2023_amd.render import Style
    init = torch.randint(0, 256, OUT + (3,), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    return {"plate": Style(replace="tracks", backdrop="plate"),
            "tight": Style(replace="tracks", backdrop="plate", plate_margin=0, plate_reach=3, plate_frames=2, plate_fill=(9, 200, 31), alpha=0, contour=0),
            "init": Style(replace="tracks", backdrop="plate", plate_init=init, plate_margin=9, plate_reach=0, matte_gain=2.0)}


def _reference(style, lm, frames, rows, mattes):
    """The reference pipeline in numpy, fed the run's own label maps and mattes: per window the block map (the margin), the update of
    every frame, the picture, and the compositing painter.  -> (pictures [L, Ho, Wo, 3], the windows' backdrops)."""
    Ho, Wo = OUT
    fr = frames.cpu().numpy()
    P, n = REF.fresh(Ho, Wo, 3) if style.plate_init is None else REF.from_picture(style.plate_init.numpy())
    pics, backs = [], []
    for ((f0, f1), cls), mat in zip(rows, mattes):
        lab = lm[f0:f1].numpy()
        block = lab if style.plate_margin == 0 else GREF.grow(lab, EVERY, style.plate_margin)
        P, n = REF.update(P, n, OREF.source_values(fr[f0:f1], f1 - f0, Ho, Wo), block == 0, style.plate_frames)
        back = REF.picture(P, n, style.plate_reach, style.plate_fill).astype(np.uint8)
        backs.append(back)
        pics.append(MREF.replace_rgb(lab, fr[f0:f1], style.palette_on("cpu").numpy(), style.actions(cls).numpy(), mat, back, style.a256,
                                     style.contour, 1))
    return np.concatenate(pics), backs


def _mattes(calls, rows):
    """The windows' mattes from the painters' recorded calls (a window may be painted in several pieces)."""
    parts = [c for name, c in calls if name == "render_replace"]
    out, at = [], 0
    for (f0, f1), _ in rows:
        got = []
        while sum(len(g) for g in got) < f1 - f0:
            got.append(parts[at]["matte"].cpu().numpy())
            at += 1
        out.append(np.concatenate(got))
    assert at == len(parts)
    return out


def test_forward_removes_the_tracks_on_both_paths_and_nothing_else_changes(video, monkeypatch):
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    assert int(lm.max()) > 0
    spy = _PlateSpy(monkeypatch)
    seen = []
    for name, st in _styles().items():
        grows = int(st.plate_margin > 0)
        for early in (True, False):
            spy.take()
            got = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=st)
            calls = spy.take()
            # per window: the margin's grow launch, one update, one picture, one painter launch (an offline video is one piece)
            assert [c[0] for c in calls] == (["grow_labels"] * grows + ["plate_update", "plate_picture", "render_replace"]) * 3, (name, early)
            painted = [c for nm, c in calls if nm == "render_replace"]
            want, backs = _reference(st, lm, frames, rows, _mattes(calls, rows))
            for c, back, ((f0, f1), _) in zip(painted, backs, rows):      # what the painters were handed: the map as made, the plate's picture
                assert torch.equal(c["labels"].cpu(), lm[f0:f1]) and np.array_equal(c["back"].cpu().numpy(), back), (name, early)
            assert len({c["back_ptr"] for c in painted}) == 1 and len({c["state_ptr"] for nm, c in calls if nm == "plate_update"}) == 1
            assert set(got) == set(base[early])
            assert np.array_equal(got["pred_overlay"].numpy(), want), (name, early)
            for k in base[early]:                                      # every other key: the bits of replace="tracks" on a colour
                if k != "pred_overlay":
                    assert _same(got[k], base[early][k]), (name, early, k)
            assert not torch.equal(got["pred_overlay"], base[early]["pred_overlay"])
        assert all(not np.array_equal(want, s) for s in seen), name
        seen.append(want)
        if name == "init":       # where the first window's matte is 255 -- and no frame of the window taught the plate -- the picture is the init picture
            hidden = (GREF.grow(lm[:6].numpy(), EVERY, st.plate_margin) != 0).all(0)
            m0 = (_mattes(calls, rows)[0] == 255) & hidden[None]
            assert m0.any() and np.array_equal(got["pred_overlay"][:6].numpy()[m0], np.broadcast_to(st.plate_init.numpy(), (6,) + OUT + (3,))[m0])
    colour = dataclasses.replace(_styles()["plate"], backdrop=(0, 255, 0))      # the same style on a colour: the former picture
    again = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=colour)
    assert torch.equal(again["pred_overlay"], base[True]["pred_overlay"])


def test_online_windows_concatenate_to_the_offline_picture(video, monkeypatch):
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    st = _styles()["plate"]
    offline = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=st)["pred_overlay"]
    spy = _PlateSpy(monkeypatch)
    for sizes in PLANS:
        ov, wins, _ = _online(model, frames, sizes, emit="overlay", style=st)
        calls = spy.take()
        assert [w.frames for w in wins] == [f for f, _ in rows]
        for w in wins:
            assert torch.equal(w.labels, lm[w.frames[0]:w.frames[1]])
        assert torch.equal(torch.cat([w.overlay for w in wins]), offline), sizes
        names = [c[0] for c in calls]
        assert names.count("grow_labels") == 3 and names.count("plate_picture") == 3          # once per window, however many pieces
        assert names.count("plate_update") == names.count("render_replace") >= 3
        want, _ = _reference(st, lm, frames, rows, _mattes(calls, rows))
        assert np.array_equal(offline.numpy(), want)
        assert "pred_overlay" not in ov.result()


def test_no_plate_call_and_no_allocation_without_the_plate(video, monkeypatch):
    from mdqe_cvpr2023_amd import merge
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    spy = _PlateSpy(monkeypatch)
    made = []
    real = merge.Plate.__init__
    monkeypatch.setattr(merge.Plate, "__init__", lambda self, *a, **kw: (made.append(1), real(self, *a, **kw))[1])
    for st in (Style(), Style(replace="tracks"), Style(replace="background", backdrop=(1, 2, 3)), Style(blur="tracks", grow=2)):
        _forward(model, frames, overlay_output=True, overlay_style=st)
        ov, wins, _ = _online(model, frames, [L], emit="overlay", style=st)
        names = {c[0] for c in spy.take()}
        assert not made and not any(n.startswith("plate_") for n in names), st
        assert ("grow_labels" in names) == (st.grow > 0)
    _forward(model, frames, overlay_output=True, overlay_style=Style(replace="tracks", backdrop="plate"))
    assert made == [1]                                                # one Plate per video


def test_six_windows_reuse_the_first_windows_state_and_backdrop(video, monkeypatch):
    from mdqe_cvpr2023_amd import merge
    model, frames, base, rows = video
    st = _styles()["plate"]
    plates = []
    real = merge.Plate.__init__
    monkeypatch.setattr(merge.Plate, "__init__", lambda self, *a, **kw: (real(self, *a, **kw), plates.append(self))[0])
    ov = model.online_video(height=OUT[0], width=OUT[1], emit="overlay", style=st)
    wins, ptrs = [], []
    long = torch.cat([frames, frames])                                # 34 frames: six windows
    for a in range(0, len(long), 4):
        got = ov.push(long[a:a + 4])
        wins += got
        if got:
            p = plates[0]
            ptrs.append((p.state.data_ptr(), p.state.untyped_storage().data_ptr(), p.back.data_ptr(), p.scratch.data_ptr(), tuple(p.scratch.shape)))
    wins += ov.close()
    p = plates[0]
    ptrs.append((p.state.data_ptr(), p.state.untyped_storage().data_ptr(), p.back.data_ptr(), p.scratch.data_ptr(), tuple(p.scratch.shape)))
    assert len(wins) >= 6 and len(plates) == 1 and len(set(ptrs)) == 1, (len(wins), ptrs)
    assert tuple(p.state.shape) == OUT + (4,) and tuple(p.back.shape) == OUT + (3,) and p.scratch.shape[0] == 6


def test_an_nv12_session_removes_the_tracks(video, monkeypatch):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style, backdrop_yuv
    model = video[0]
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda", matrix="bt601", full_range=True, order="bgr")
    before = s.y.clone(), s.uv.clone()
    H, W = 96, 160
    ys = s.y[:, :H, :W].cpu().numpy().astype(np.int64)[..., None]
    cs = s.uv[:, :H // 2, :W].cpu().numpy().astype(np.int64).reshape(L, H // 2, W // 2, 2)
    init = s[3:4].to("cuda")
    kind = (s.fmt, s.matrix, s.full_range, s.order)
    ref, _, _ = _session(model, s, (5, 3, 7, 2), surface=True, style=Style(replace="tracks"))
    spy = _PlateSpy(monkeypatch)
    pictures = {}
    for name, st in (("plate", Style(replace="tracks", backdrop="plate", plate_fill=(200, 10, 90))),
                     ("init", Style(replace="tracks", backdrop="plate", plate_init=init, plate_margin=0, plate_reach=5, plate_frames=3))):
        for pushes in ((5, 3, 7, 2), (17,)):
            spy.take()
            wins, res, _ = _session(model, s, pushes, surface=True, style=st)
            calls = spy.take()
            names = [c[0] for c in calls]
            assert names.count("plate_picture_yuv") == 3 and names.count("grow_labels") == 3 * (st.plate_margin > 0)
            assert names.count("plate_update_yuv") == names.count("render_replace_yuv") >= 3 and "plate_update" not in names
            painted = [c for nm, c in calls if nm == "render_replace_yuv"]
            assert len({c["back_ptr"] for c in painted}) == 1
            fill = backdrop_yuv(st.plate_fill, *kind).numpy().astype(np.int64)
            if st.plate_init is None:
                (Py, ny), (Pc, nc) = REF.fresh(H, W, 1), REF.fresh(H // 2, W // 2, 2)
            else:
                (Py, ny), (Pc, nc) = REF.from_picture(ys[3]), REF.from_picture(cs[3])
            pal = st.palette_yuv_on("cuda", *kind)
            at = 0
            for win, r in zip(wins, ref):
                f0, f1 = win.frames
                assert torch.equal(win.labels, r.labels)
                lab = win.labels.numpy()
                block = lab if st.plate_margin == 0 else GREF.grow(lab, EVERY, st.plate_margin)
                Py, ny = REF.update(Py, ny, ys[f0:f1], block == 0, st.plate_frames)
                Pc, nc = REF.update(Pc, nc, cs[f0:f1], REF.observed_chroma(block), st.plate_frames)
                wy = REF.picture(Py, ny, st.plate_reach, fill[:1])[..., 0].astype(np.uint8)
                wc = REF.picture(Pc, nc, (st.plate_reach + 1) // 2, fill[1:]).reshape(H // 2, W).astype(np.uint8)
                mats = []
                while sum(len(m) for m in mats) < f1 - f0:            # (the window's pieces)
                    back = painted[at]["back"]
                    assert np.array_equal(back.y[0, :H, :W].cpu().numpy(), wy) and np.array_equal(back.uv[0, :H // 2, :W].cpu().numpy(), wc), (name, win.frames)
                    mats.append(painted[at]["matte"])
                    at += 1
                back = YuvFrames(_dev(wy[None]), _dev(wc[None]), H, W, fmt=s.fmt, matrix=s.matrix, full_range=s.full_range, order=s.order)
                want = ops.render_replace_yuv(win.labels.cuda(), s[f0:f1], pal, st.actions(win.cls_probs).cuda(), torch.cat(mats), back, None, 0,
                                              st.a256, st.contour, "tracks")
                pic = win.overlay
                assert isinstance(pic, YuvFrames) and not pic.is_cuda and pic.meta() == s.meta()
                assert torch.equal(pic.y[:, :, :W], want.y.cpu()) and torch.equal(pic.uv[:, :, :W], want.uv.cpu()), (name, win.frames)
            assert at == len(painted)
            whole = torch.cat([w.overlay.y for w in wins])
            assert torch.equal(whole, res["pred_overlay"].y)
            assert pictures.setdefault(name, whole) is whole or torch.equal(pictures[name], whole)      # whatever the pushes
            assert not torch.equal(whole, torch.cat([r.overlay.y for r in ref]))
    assert not torch.equal(pictures["plate"], pictures["init"])
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])


def test_refusals_at_the_model(video):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    wrong = torch.zeros(OUT[0] + 1, OUT[1], 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="(?s)plate_init picture is 91 x 150 but the output is 90 x 150.*resize"):
        _forward(model, frames, overlay_output=True, overlay_style=Style(replace="tracks", backdrop="plate", plate_init=wrong))
    again = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=Style(replace="tracks"))
    assert torch.equal(again["pred_overlay"], base[True]["pred_overlay"])
