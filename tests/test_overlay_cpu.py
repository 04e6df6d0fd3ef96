"""Rendered overlay frames, the host side: the reference painter (tests/_overlay_ref.py) on hand-computed cases, the palette and the
style, the errors that need no launch (the wrapper's argument checks, a bad `emit`, a bad `overlay_output`), the ABI entry, and the
frame store's bookkeeping on plain tensors.  No GPU."""
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

import _overlay_ref as REF  # noqa: E402


# ---- the painter on 3 x 4 cases worked out by hand -----------------------------------------------------------------------------------
def _case():
    """Label 5 on columns 0..2 of a 3 x 4 frame, background on column 3; a frame of one colour (100, 110, 120); colour 5 = (200, 100, 0)."""
    lab = np.zeros((1, 3, 4), dtype=np.uint8)
    lab[0, :, :3] = 5
    fr = np.zeros((1, 3, 3, 4), dtype=np.uint8)
    fr[0, 0], fr[0, 1], fr[0, 2] = 100, 110, 120
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[5] = (200, 100, 0)
    pal[0] = (9, 9, 9)                                               # never used: background keeps the source
    return lab, fr, pal


SRC, COL = (100, 110, 120), (200, 100, 0)
MIX = (150, 105, 60)        # (100*128 + 200*128 + 128) >> 8 = 38528 >> 8, (110*128 + 100*128 + 128) >> 8 = 27008 >> 8, (120*128 + 128) >> 8


@pytest.mark.parametrize("painter", [REF.paint, REF.paint_pixelwise])
def test_painter_on_hand_computed_cases(painter):
    lab, fr, pal = _case()
    # r = 1: only column 2 has a neighbour (column 3) with another label; the pixels of columns 0 and 1 on the image border are NOT edges
    got = painter(lab, fr, pal, 128, 1)[0]
    want = np.array([[MIX, MIX, COL, SRC]] * 3, dtype=np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # r = 2: column 1 sees column 3 two steps away; column 0 still sees nothing (two rows up or down lie outside or hold label 5)
    assert np.array_equal(painter(lab, fr, pal, 128, 2)[0], np.array([[MIX, COL, COL, SRC]] * 3, dtype=np.uint8))
    assert np.array_equal(painter(lab, fr, pal, 128, 3)[0], np.array([[COL, COL, COL, SRC]] * 3, dtype=np.uint8))
    assert np.array_equal(painter(lab, fr, pal, 128, 0)[0], np.array([[MIX, MIX, MIX, SRC]] * 3, dtype=np.uint8))
    # the ends of the blend: the source and the palette exactly
    assert np.array_equal(painter(lab, fr, pal, 0, 0)[0], np.array([[SRC] * 4] * 3, dtype=np.uint8))
    assert np.array_equal(painter(lab, fr, pal, 256, 0)[0], np.array([[COL, COL, COL, SRC]] * 3, dtype=np.uint8))
    # no frames: onto black
    assert np.array_equal(painter(lab, None, pal, 256, 1)[0], np.array([[COL, COL, COL, (0, 0, 0)]] * 3, dtype=np.uint8))
    assert np.array_equal(painter(lab, None, pal, 128, 0)[0], np.array([[(100, 50, 0)] * 3 + [(0, 0, 0)]] * 3, dtype=np.uint8))
    # a vertical neighbour, and an object cut by the border: the line runs where labels meet, not along the border
    lab2 = np.zeros((1, 3, 4), dtype=np.uint8)
    lab2[0, 0] = 5
    assert np.array_equal(painter(lab2, fr, pal, 128, 1)[0], np.array([[COL] * 4, [SRC] * 4, [SRC] * 4], dtype=np.uint8))


def test_painter_float_frames_and_sampling():
    lab = np.zeros((1, 2, 4), dtype=np.uint8)
    pal = np.zeros((256, 3), dtype=np.uint8)
    fr = np.zeros((1, 3, 1, 2), dtype=np.float32)
    fr[0, 0, 0] = (0.5, 1.5)            # half-even: 0 and 2
    fr[0, 1, 0] = (2.5, -3.0)           # 2 and 0
    fr[0, 2, 0] = (300.0, np.nan)       # 255 and 0
    got = REF.paint(lab, fr, pal, 128, 1)
    # Ho, Wo = 2, 4 from h0, w0 = 1, 2: sx = (X*2)//4 = 0, 0, 1, 1 and sy = 0
    want = np.array([[(0, 2, 255), (0, 2, 255), (2, 0, 0), (2, 0, 0)]] * 2, dtype=np.uint8)
    assert np.array_equal(got[0], want) and np.array_equal(REF.paint_pixelwise(lab, fr, pal, 128, 1)[0], want)


def test_vectorised_painter_equals_the_rule_written_as_loops():
    rng = np.random.default_rng(0)
    pal = rng.integers(0, 256, size=(256, 3)).astype(np.uint8)
    for Ho, Wo, h0, w0 in ((5, 7, 5, 7), (6, 5, 3, 4), (1, 3, 5, 7), (4, 1, 9, 2)):
        lab = rng.integers(0, 3, size=(2, Ho, Wo)).astype(np.uint8) * 127
        fr = rng.integers(0, 256, size=(2, 3, h0, w0)).astype(np.uint8)
        for r in range(4):
            for a in (0, 77, 256):
                assert np.array_equal(REF.paint(lab, fr, pal, a, r), REF.paint_pixelwise(lab, fr, pal, a, r))


# ---- palette and style ---------------------------------------------------------------------------------------------------------------
def test_default_palette_properties():
    from mdqe_cvpr2023_amd.render import default_palette
    pal = default_palette()
    assert pal.dtype == torch.uint8 and tuple(pal.shape) == (256, 3) and not pal.is_cuda
    assert torch.equal(pal, default_palette())                        # a pure function of the label
    p = pal.numpy().astype(np.int64)
    assert tuple(p[0]) == (0, 0, 0)
    assert len({tuple(r) for r in p[1:]}) == 255
    for i in range(1, 256):
        for j in range(i + 1, min(256, i + 8)):
            assert int(np.abs(p[i] - p[j]).sum()) >= 64, (i, j)
    assert int(p[1:].max(1).min()) >= 128


def test_style_validation():
    from mdqe_cvpr2023_amd.render import Style, default_palette
    s = Style()
    assert (s.alpha, s.contour, s.palette, s.a256) == (0.5, 1, None, 128)
    assert Style(alpha=0.25).a256 == 64 and Style(alpha=0).a256 == 0 and Style(alpha=1.0).a256 == 256 and Style(alpha=0.999).a256 == 256
    assert torch.equal(s.palette_on("cpu"), default_palette())
    pal = torch.arange(768, dtype=torch.int64).remainder(256).to(torch.uint8).view(256, 3)
    assert torch.equal(Style(palette=pal, contour=3).palette_on("cpu"), pal)
    for kw in ({"alpha": -0.01}, {"alpha": 1.01}, {"alpha": "0.5"}, {"alpha": float("nan")}, {"contour": -1}, {"contour": 4}, {"contour": 1.0},
               {"contour": True}, {"palette": pal.float()}, {"palette": pal[:255]}, {"palette": pal.view(3, 256)}, {"palette": pal.tolist()}):
        with pytest.raises(ValueError, match="overlay style"):
            Style(**kw)


# ---- errors that need no launch ------------------------------------------------------------------------------------------------------
def test_wrapper_argument_checks_come_before_any_launch():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.render import default_palette
    lab = torch.zeros(2, 6, 8, dtype=torch.uint8)
    fr = torch.zeros(2, 3, 6, 8, dtype=torch.uint8)
    pal = default_palette()
    out = torch.zeros(3, 6, 8, 3, dtype=torch.uint8)

    def call(lab=lab, fr=fr, pal=pal, out=out, **kw):
        return ops.render_overlay(lab, fr, pal, out, **kw)
    for bad in (lab.float(), lab[0], lab[:, :, ::2], torch.zeros(2, 6, 16, dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(RuntimeError, match="labels must be contiguous uint8"):
            call(lab=bad)
    for kw in ({"a256": 257}, {"a256": -1}, {"a256": 128.0}, {"contour": 4}, {"contour": -1}, {"contour": 1.5}):
        with pytest.raises(RuntimeError, match="a256 must be an int in 0..256 and contour an int in 0..3"):
            call(**kw)
    for bad in (pal.float(), pal[:255], pal.view(3, 256), torch.zeros(256, 6, dtype=torch.uint8)[:, ::2]):
        with pytest.raises(RuntimeError, match="palette must be contiguous uint8"):
            call(pal=bad)
    for bad in (out.float(), out[:, :, :, :2], out[:1], out.view(3, 6, 24), torch.zeros(3, 8, 6, 3, dtype=torch.uint8),
                torch.zeros(3, 6, 8, 6, dtype=torch.uint8)[..., ::2]):
        with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
            call(out=bad)
    for f_off in (2, -1):                                             # 2 + F > 3 frames
        with pytest.raises(RuntimeError, match="out must be contiguous CUDA uint8"):
            call(f_off=f_off)
    for bad in (fr.long(), fr[:1], fr[:, :2], fr[0], torch.zeros(2, 3, 6, 16, dtype=torch.uint8)[..., ::2], fr.half(),
                torch.zeros(2, 6, 8, 3, dtype=torch.uint8).permute(0, 3, 1, 2)):
        with pytest.raises(RuntimeError, match="render_overlay: (frames must be|every frame must be contiguous)"):
            call(fr=bad)
    big = torch.zeros(4, 3, 6, 8, dtype=torch.uint8)
    for ok_frames in (fr, fr.float(), None, big[::2], big[1:3]):      # right in every respect, but host tensors: the device check is last
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call(fr=ok_frames)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdqe_hip.h")).read(), flags=re.S)


def test_abi_declares_exports_and_binds_the_overlay_entry_point():
    from mdqe_cvpr2023_amd import _lib
    name = "mdqe_render_overlay_u8"
    src = _header()
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    h = _lib.load_library()
    assert re.search(r"\bint\s+%s\s*\(" % name, src), name + " is not declared in mdqe_hip.h"
    assert hasattr(h, name) and name in _lib.SIGNATURES
    proto = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, src, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_lib.SIGNATURES[name]) == 15
    assert h.mdqe_abi_version() == 6 and re.search(r"#define\s+MDQE_ABI_VERSION\s+6\b", src)      # no existing entry changed
    # out-of-range a256 / contour are refused by the entry point itself, before any pointer is looked at (NULL everywhere: no launch)
    fn = h.mdqe_render_overlay_u8
    assert fn(None, 1, 0, 4, 4, None, 1, 4, 4, None, 257, 1, None, 0, None) != 0
    assert fn(None, 1, 0, 4, 4, None, 1, 4, 4, None, -1, 1, None, 0, None) != 0
    assert fn(None, 1, 0, 4, 4, None, 1, 4, 4, None, 128, 4, None, 0, None) != 0
    assert fn(None, 1, 0, 4, 4, None, 1, 0, 4, None, 128, 1, None, 0, None) != 0          # Ho = 0
    assert fn(None, 1, 0, 4, 4, None, 1, 30000, 30000, None, 128, 1, None, 0, None) != 0  # Ho*Wo*3 >= 2^31
    assert fn(None, 1, 0, 4, 4, None, 0, 4, 4, None, 128, 1, None, 0, None) == 0          # F = 0: OK, nothing launched


def _standin(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    cfg = dataclasses.replace(PRESETS["R50_ovis_360"], **kw)

    def check():
        from mdqe_cvpr2023_amd.meta_arch import MDQE
        MDQE.check_label_capacity(types.SimpleNamespace(cfg=cfg))
    return types.SimpleNamespace(cfg=cfg, device=torch.device("cuda", 0), check_label_capacity=check)


def test_online_video_accepts_overlay_and_still_refuses_other_values():
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    from mdqe_cvpr2023_amd.render import Style
    ov = MDQE.online_video(_standin(), emit="overlay")
    assert ov.emit == "overlay" and ov.frames_held == 0 and ov.style == Style()
    st = Style(alpha=0.25, contour=2)
    assert MDQE.online_video(_standin(), emit="overlay", style=st).style is st
    assert ov.push(torch.empty(0, 3, 8, 8, dtype=torch.uint8)) == []      # n == 0: no-op
    assert MDQE.online_video(_standin(), emit="labels").frames_held == 0
    for bad in ("png", "overlays", None):
        with pytest.raises(ValueError, match="emit"):
            MDQE.online_video(_standin(), emit=bad)
    with pytest.raises(ValueError, match="n_max_inst"):
        MDQE.online_video(_standin(n_max_inst=256), emit="overlay")
    with pytest.raises(ValueError, match="style"):
        MDQE.online_video(_standin(), emit="overlay", style={"alpha": 0.5})
    with pytest.raises(ValueError, match="style"):
        MDQE.online_video(_standin(), emit="labels", style=st)


def test_window_has_overlay_and_its_fields_are_what_they_were():
    from mdqe_cvpr2023_amd import online
    assert [f.name for f in dataclasses.fields(online.Window)] == ["frames", "track_ids", "cls_probs", "masks", "rles", "boxes", "areas"]
    w = online.Window(frames=(0, 1), track_ids=[], cls_probs=torch.zeros(0, 2))
    assert w.overlay is None and w.labels is None and w.masks is None
    pic, lab = torch.zeros(1, 2, 3, 3, dtype=torch.uint8), torch.zeros(1, 2, 3, dtype=torch.uint8)
    w = online.Window(frames=(0, 1), track_ids=[], cls_probs=torch.zeros(0, 2), labels=lab, overlay=pic)
    assert w.overlay is pic and w.labels is lab


def _cpu_model(**kw):
    from mdqe_cvpr2023_amd.config import PRESETS
    from mdqe_cvpr2023_amd.meta_arch import MDQE
    return MDQE(dataclasses.replace(PRESETS["R50_ovis_360"], **kw), seed=1)


def test_overlay_output_and_style_setters():
    from mdqe_cvpr2023_amd.render import Style
    big, ok = _cpu_model(n_max_inst=256), _cpu_model(n_max_inst=255)
    assert big.overlay_output is False and ok.overlay_output is False and ok.overlay_style == Style()
    with pytest.raises(ValueError, match="n_max_inst"):
        big.overlay_output = True
    assert big.overlay_output is False
    big.overlay_output = False
    ok.overlay_output = True
    assert ok.overlay_output is True and ok.label_output is False
    for bad in ("only", 1, 0, None, "overlay", 1.0):
        with pytest.raises(ValueError, match="overlay_output"):
            ok.overlay_output = bad
    assert ok.overlay_output is True
    ok.overlay_output = False
    st = Style(alpha=0.25, contour=2)
    ok.overlay_style = st
    assert ok.overlay_style is st
    for bad in (None, {"alpha": 0.5}, 0.5):
        with pytest.raises(ValueError, match="overlay_style"):
            ok.overlay_style = bad


def test_the_sharded_driver_and_a_merger_without_frames_refuse_the_overlay():
    from mdqe_cvpr2023_amd import merge
    model = types.SimpleNamespace(overlay_output=True, geometry_output=False, label_output=False)
    with pytest.raises(ValueError, match="sharded"):
        merge.ClipMerger(model, (8, 8), (8, 8), (2, 2), n_frames=4)
    import inspect
    from mdqe_cvpr2023_amd import sharding
    assert "overlay_output is not offered by the sharded driver" in inspect.getsource(sharding)


# ---- the frame store's bookkeeping on plain tensors ----------------------------------------------------------------------------------
def _store_with(sizes, h=2, w=3):
    from mdqe_cvpr2023_amd.merge import FrameStore
    st, at, video = FrameStore(), 0, []
    for n in sizes:
        t = (torch.arange(at, at + n, dtype=torch.float32).view(n, 1, 1, 1) * torch.ones(1, 3, h, w)).contiguous()
        st.add(at, t)
        video.append(t)
        at += n
    return st, torch.cat(video)


def test_frame_store_pieces_and_drops():
    st, video = _store_with([4, 0, 3, 5])                             # frames 0..3, 4..6, 7..11 (an empty push holds nothing)
    assert st.frames_held == 12 and len(st.chunks) == 3
    one = st.pieces(1, 3)
    assert [(tuple(t.shape), f) for t, f in one] == [((2, 3, 2, 3), 1)] and torch.equal(one[0][0], video[1:3])
    assert one[0][0].untyped_storage().data_ptr() == st.chunks[0][1].untyped_storage().data_ptr()       # a view: no copy
    two = st.pieces(2, 6)                                             # a window that spans two pushes: two pieces
    assert [(int(t.shape[0]), f) for t, f in two] == [(2, 2), (2, 4)] and torch.equal(torch.cat([t for t, _ in two]), video[2:6])
    three = st.pieces(3, 9)
    assert [(int(t.shape[0]), f) for t, f in three] == [(1, 3), (3, 4), (2, 7)] and torch.equal(torch.cat([t for t, _ in three]), video[3:9])
    assert [(int(t.shape[0]), f) for t, f in st.pieces(4, 7)] == [(3, 4)]
    with pytest.raises(RuntimeError, match="does not hold"):
        st.pieces(10, 13)
    st.drop_before(3)                                                 # chunk 0 still holds frame 3
    assert st.frames_held == 12
    st.drop_before(4)                                                 # chunk 0 lies wholly before frame 4
    assert st.frames_held == 8 and [c[0] for c in st.chunks] == [4, 7]
    with pytest.raises(RuntimeError, match="does not hold"):
        st.pieces(3, 5)
    st.drop_before(9)
    assert st.frames_held == 5 and torch.equal(st.pieces(9, 12)[0][0], video[9:12])
    st.drop_before(12)
    assert st.frames_held == 0 and st.chunks == []
    # a chunk that may be the caller's memory is copied by own(); an owned one is left alone
    from mdqe_cvpr2023_amd.merge import FrameStore
    st, mine, theirs = FrameStore(), torch.zeros(2, 3, 2, 3), torch.ones(2, 3, 2, 3)
    st.add(0, mine, owned=True)
    st.add(2, theirs, owned=False)
    st.own()
    assert st.chunks[0][1] is mine and st.chunks[1][1] is not theirs and torch.equal(st.chunks[1][1], theirs)
    theirs.zero_()                                                    # the caller refills its buffer
    assert bool((st.pieces(2, 4)[0][0] == 1).all())


def test_frames_held_stays_bounded_by_the_schedule_over_the_push_plans():
    """The session's steps on the schedule alone (online.plan): a push adds its frames, the windows it flushes move `emitted` forward,
    then the chunks wholly before `emitted` are dropped -- what OnlineVideo.push does around the model.  After every push
    frames_held <= (received - emitted) + largest push - 1, and every flushed window finds its frames."""
    from mdqe_cvpr2023_amd import online as O
    from mdqe_cvpr2023_amd.merge import FrameStore
    from test_online_cpu import _cases
    checked = spanning = closed = 0
    for L, T, stride, win, sizes in _cases(n=300, seed=7):
        if stride > T:                # (no config has it: frames between two clips would belong to no clip, and a window could be flushed
            continue                  # before its frames have arrived; with stride <= T the flush clip ends at or behind the window's end)
        steps = O.plan(sizes, T, stride, win)
        n_win = sum(len(s["windows"]) for s in steps)
        st, emitted, received, k = FrameStore(), 0, 0, 0
        for n, step in zip(list(sizes) + [None], steps):
            if n is not None:
                st.add(received, torch.empty(n, 3, 1, 1))
                received += n
            assert received == step["received"]
            for _ in step["windows"]:                                 # window k: `win` frames, the last one whatever is left (at close())
                k += 1
                f1 = received if (n is None and k == n_win) else emitted + win
                assert emitted < f1 <= received
                parts = st.pieces(emitted, f1)
                assert sum(int(t.shape[0]) for t, _ in parts) == f1 - emitted and parts[0][1] == emitted
                spanning += len(parts) > 1
                emitted = f1
            st.drop_before(emitted)
            if n is not None:
                assert st.frames_held <= (received - emitted) + max(sizes) - 1, (L, T, stride, win, sizes)
                assert st.frames_held >= received - emitted
                checked += 1
        if any(c[2] for c in steps[-1]["clips"]):                     # (a schedule whose last clip ends exactly at L has no clamped clip:
            assert emitted == L and st.frames_held == 0               # close() then flushes nothing, as for every other output form)
            closed += 1
    print(checked, spanning, closed)
    assert checked > 1000 and spanning > 100 and closed > 50
