"""The edge-stopping blur on the device: mdqe_render_blur_within_u8 and mdqe_render_blur_within_yuv420sp (ops.render_blur(edge="stop"),
ops.render_blur_yuv(edge="stop")) against the numpy oracle (tests/_blur_within_ref.py), their equality with the plain painters under the
table [0, 1, 1, ...], label maps chosen for the membership mask (a one-pixel line across tiles, a checkerboard, the four corners, one
member pixel at a tile corner, the 32-bit bound), independence from every non-member's source, every output alignment, and the styles
above them: forward() with model.overlay_style and online_video(style=...) with blur_edge="stop", RGB pictures and NV12 surfaces, with
a margin, and the former calls for every style without it.  Integers only: every comparison is exact.

Kernel shapes: (70, 300) has tiles on both axes and a halo of 32 that reaches past a neighbouring tile; (3, 200) is shorter than the
radius one way and several tiles the other; (5, 7) -> (1, 3) is smaller than any radius; (60, 90) -> (120, 180) resamples.  The radii
(0, 1, 5, 8, 9, 17, 32) reach every padded radius (0, 4, 8, 16, 24, 32) and both sides of 8; each meets the four action tables with
contour 0..3 and a256 in {0, 128, 256} rotating through them."""
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

import _blur_ref as BREF  # noqa: E402
import _blur_within_ref as REF  # noqa: E402
import _grow_ref as GREF  # noqa: E402
import _overlay_yuv_ref as OYREF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402
from test_blur_gpu import A256, SENTINEL, YUV_SHAPES, _combos, _taps, video  # noqa: E402, F401  (`video`: the module's fixture)
from test_overlay_gpu import L, OUT, PLANS, _forward, _frames, _label_sets, _online, _palettes, _same  # noqa: E402
from test_overlay_yuv_gpu import _layouts, _raw, _session, _surfaces, _typed  # noqa: E402
from test_overlay_yuv_gpu import _frames as _yuv_frames  # noqa: E402
from test_overlay_yuv_gpu import _palette as _yuv_palette  # noqa: E402

SIZES = [(61, 97, 61, 97), (60, 90, 120, 180), (5, 7, 1, 3), (70, 300, 70, 300), (3, 200, 3, 200)]   # (h0, w0, Ho, Wo)
RADII = (0, 1, 5, 8, 9, 17, 32)
YUV_RADII = (0, 1, 5, 32)
TABLES = REF.action_tables()
F = 3


# ---- the RGB kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32", "none", "strided"])
@pytest.mark.parametrize("size", SIZES)
def test_render_blur_stop_against_the_reference(size, kind):
    from mdqe_cvpr2023_amd import ops
    h0, w0, Ho, Wo = size
    sets = _label_sets(Ho, Wo, seed=Ho * 1000 + Wo)
    fr_dev, fr_np = _frames(kind, F, h0, w0, seed=h0 + w0)
    pals = _palettes()
    acts = {k: torch.from_numpy(v).cuda() for k, v in TABLES.items()}
    n = 0
    for i, (radius, name, contour, a256) in enumerate(_combos(RADII)):
        lab, pal, f_off = sets[i % 2], pals[(i // 2) % 2], 1 - i % 2          # (f_off = 1: the output starts at an odd byte for odd Ho * Wo)
        taps_dev, taps_np = _taps(radius)
        out = torch.full((f_off + F + 1, Ho, Wo, 3), 0xAB, dtype=torch.uint8, device="cuda")
        lab_dev, pal_dev = torch.from_numpy(lab).cuda(), pal.cuda()
        assert ops.render_blur(lab_dev, fr_dev, pal_dev, acts[name], taps_dev, out, f_off, a256, contour, edge="stop") is out
        o = out.cpu()
        want = torch.from_numpy(REF.paint(lab, fr_np, pal.numpy(), TABLES[name], a256, contour, taps_np))
        assert torch.equal(o[f_off:f_off + F], want), (size, kind, radius, name, contour, a256)
        assert bool((o[:f_off] == 0xAB).all()) and bool((o[f_off + F:] == 0xAB).all())           # the guard frames
        if name == "plain":                                                                      # the plain painter, bit for bit
            plain = torch.full_like(out, 0xAB)
            ops.render_overlay(lab_dev, fr_dev, pal_dev, plain, f_off, a256, contour)
            assert torch.equal(plain, out), (size, kind, radius)
        if name == "all" and radius == 0:                                                        # the source itself
            src = BREF.OREF.source_values(fr_np, F, Ho, Wo)
            assert np.array_equal(o[f_off:f_off + F].numpy(), src.astype(np.uint8)), (size, kind)
        n += 1
    assert n == 28


def _mask_maps(Ho, Wo):
    """Label maps chosen for the membership mask; label 9 is the member, label 4 a tinted block in tiles of its own."""
    yy, xx = np.mgrid[:Ho, :Wo]
    line = np.zeros((2, Ho, Wo), dtype=np.uint8)
    line[0, 23, :] = 9                                                # one pixel wide, across every tile of a row of tiles
    line[1, :, 127] = 9                                               # ... and down the last column of a tile
    line[1, 5:60, 128] = 0
    checker = np.zeros((2, Ho, Wo), dtype=np.uint8)
    checker[0] = np.where((yy + xx) % 2 == 0, 9, 0)
    checker[1] = np.where((yy // 3 + xx // 5) % 2 == 0, 9, 4)
    corners = np.zeros((2, Ho, Wo), dtype=np.uint8)
    corners[:] = np.where((np.minimum(yy, Ho - 1 - yy) < 20) & (np.minimum(xx, Wo - 1 - xx) < 70) | (yy == 40), 9, 0)   # one region, all four corners
    corners[1, 25:45, 100:200] = 4
    single = np.zeros((2, Ho, Wo), dtype=np.uint8)
    single[0, 16, 64] = 9                                             # one member pixel at a tile's corner: D = taps[0]^2
    single[1, 15, 63] = 9
    single[1, 69, 299] = 9
    single[:, 40:50, 200:230] = 4
    return {"line": line, "checkerboard": checker, "corners": corners, "single": single}


@pytest.mark.parametrize("which", ["line", "checkerboard", "corners", "single"])
def test_label_maps_chosen_for_the_mask(which):
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 70, 300
    lab = _mask_maps(Ho, Wo)[which]
    act = np.zeros(256, dtype=np.uint8)
    act[9], act[4] = 3, 1
    fr = torch.randint(0, 256, (2, 3, Ho, Wo), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    pal = _palettes()[0]
    kept = np.moveaxis(fr.numpy(), 1, -1)
    for radius in (1, 8, 17, 32):
        taps_dev, taps_np = _taps(radius)
        out = torch.full((2, Ho, Wo, 3), 0xAB, dtype=torch.uint8, device="cuda")
        ops.render_blur(torch.from_numpy(lab).cuda(), fr.cuda(), pal.cuda(), torch.from_numpy(act).cuda(), taps_dev, out, 0, 128, 1, edge="stop")
        want = REF.paint(lab, fr.numpy(), pal.numpy(), act, 128, 1, taps_np)
        assert np.array_equal(out.cpu().numpy(), want), (which, radius)
        assert np.array_equal(want[lab == 0], kept[lab == 0])
        if which == "single":                                         # a member alone under the kernel keeps its value: N = v * D
            assert np.array_equal(want[lab == 9], kept[lab == 9])
        else:
            assert not np.array_equal(want[lab == 9], kept[lab == 9])


def test_the_32_bit_bound_an_all_255_picture_at_radius_32():
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 70, 300
    lab = torch.from_numpy(_label_sets(Ho, Wo, seed=1)[0][:2]).cuda()
    fr = torch.full((2, 3, Ho, Wo), 255, dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, Ho, Wo, 3), dtype=torch.uint8, device="cuda")
    ops.render_blur(lab, fr, _palettes()[0].cuda(), torch.from_numpy(TABLES["all"]).cuda(), _taps(32)[0], out, 0, 128, 1, edge="stop")
    assert bool((out == 255).all())


@pytest.mark.parametrize("table,radius", [("background", 17), ("mix", 17), ("background", 32), ("mix", 32)])
def test_a_blurred_pixel_does_not_depend_on_any_non_member_on_the_device(table, radius):
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 70, 300                                                  # (radius 32: members of one tile, non-members of the next under its taps)
    lab = _label_sets(Ho, Wo, seed=11)[0]
    act = TABLES[table]
    member = act[lab] == 3
    assert member.any() and (~member).any()
    g = torch.Generator().manual_seed(radius)
    fr = torch.randint(0, 256, (F, 3, Ho, Wo), generator=g, dtype=torch.uint8)
    other = torch.where(torch.from_numpy(member)[:, None], fr, torch.randint(0, 256, fr.shape, generator=g, dtype=torch.uint8))
    assert not torch.equal(other, fr)
    taps_dev, taps_np = _taps(radius)
    args = (torch.from_numpy(lab).cuda(), _palettes()[1].cuda(), torch.from_numpy(act).cuda(), taps_dev)
    outs = []
    for edge in ("stop", "bleed"):
        a, b = (ops.render_blur(args[0], x.cuda(), *args[1:], torch.empty((F, Ho, Wo, 3), dtype=torch.uint8, device="cuda"), 0, 128, 1,
                                edge=edge).cpu().numpy() for x in (fr, other))
        outs.append((a, b))
    (a, b), (pa, pb) = outs
    assert np.array_equal(a[member], b[member]) and not np.array_equal(a[~member], b[~member])
    assert not np.array_equal(pa[member], pb[member])                 # the plain blur takes the non-members in
    assert np.array_equal(a, REF.paint(lab, fr.numpy(), _palettes()[1].numpy(), act, 128, 1, taps_np))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_alignment_of_the_output_and_runs_are_identical(shift):
    from mdqe_cvpr2023_amd import ops
    pal = _palettes()[1]
    act = torch.from_numpy(TABLES["mix"]).cuda()
    for n, Ho, Wo, radius in ((2, 13, 9, 2), (2, 13, 70, 5), (1, 1, 2, 17), (1, 2, 3, 1), (1, 1, 1, 32), (1, 20, 132, 8)):
        rng = np.random.default_rng(n * Ho + Wo)
        lab = rng.integers(0, 256, size=(n, Ho, Wo)).astype(np.uint8)
        fr = torch.randint(0, 256, (n, 3, Ho, Wo), generator=torch.Generator().manual_seed(Ho), dtype=torch.uint8)
        taps_dev, taps_np = _taps(radius)
        nb = n * Ho * Wo * 3
        raw = torch.full((nb + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        out = raw[shift:shift + nb].view(n, Ho, Wo, 3)
        assert out.is_contiguous() and out.data_ptr() % 4 == shift
        args = (torch.from_numpy(lab).cuda(), fr.cuda(), pal.cuda(), act, taps_dev)
        ops.render_blur(*args, out, 0, 77, 2, edge="stop")
        want = torch.from_numpy(REF.paint(lab, fr.numpy(), pal.numpy(), TABLES["mix"], 77, 2, taps_np))
        r = raw.cpu()
        assert torch.equal(r[shift:shift + nb].view(n, Ho, Wo, 3), want), (shift, n, Ho, Wo)
        assert bool((r[:shift] == 0xAB).all()) and bool((r[shift + nb:] == 0xAB).all())
        again = torch.empty_like(out)
        ops.render_blur(*args, again, 0, 77, 2, edge="stop")
        assert torch.equal(again, out)                                # identical from run to run


def test_no_frames_to_paint_is_no_launch():
    from mdqe_cvpr2023_amd import ops
    pal, act = _palettes()[0].cuda(), torch.from_numpy(TABLES["all"]).cuda()
    out = torch.full((2, 4, 5, 3), 0xAB, dtype=torch.uint8, device="cuda")
    ops.render_blur(torch.zeros(0, 4, 5, dtype=torch.uint8, device="cuda"), None, pal, act, _taps(8)[0], out, 1, edge="stop")
    assert bool((out == 0xAB).all())


# ---- the surface kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", YUV_SHAPES)
def test_render_blur_yuv_stop_against_the_reference(H, W, fmt):
    from mdqe_cvpr2023_amd import ops
    ys, cs = YREF.make_content(H * 1000 + W, F, H, W, fmt)
    lab = OYREF.make_labels(H * 7 + W, F, H, W)
    pal_np, pal = _yuv_palette(H + W, fmt)
    combos = list(_combos(YUV_RADII))
    tables = {r: (_taps(r), _taps((r + 1) // 2)) for r in YUV_RADII}
    want = [REF.paint_yuv(ys, cs, lab, pal_np, TABLES[name], fmt, a256, contour, tables[r][0][1], tables[r][1][1]) for r, name, contour, a256 in combos]
    lab_dev, pal_dev = torch.from_numpy(lab).cuda(), pal.cuda()
    acts = {k: torch.from_numpy(v).cuda() for k, v in TABLES.items()}
    low = 0
    for pitch, crow, extra, lead in _layouts(H, W, fmt):              # tight; padded; entered one sample late
        flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
        host = torch.from_numpy(flat)
        dev = host.cuda()
        src = _yuv_frames(dev, F, H, W, fmt, pitch, crow, rows, lead)
        blank = torch.full((lead + (F + 2) * rows * pitch,), SENTINEL, dtype=torch.uint8)
        for (r, name, contour, a256), (wy, wc) in zip(combos, want):
            (taps, _), (taps_c, _) = tables[r]
            expect = blank.clone()
            e = _yuv_frames(expect, F + 2, H, W, fmt, pitch, crow, rows, lead)
            e.y[1:1 + F, :, :W] = _typed(wy, fmt)
            e.uv[1:1 + F, :, :wc.shape[2]] = _typed(wc, fmt)
            out_flat = blank.cuda()
            out = _yuv_frames(out_flat, F + 2, H, W, fmt, pitch, crow, rows, lead)
            assert ops.render_blur_yuv(lab_dev, src, pal_dev, acts[name], taps, taps_c, out, 1, a256, contour, edge="stop") is out
            assert torch.equal(out_flat.cpu(), expect), (pitch, crow, extra, lead, r, name, contour, a256)
            if name == "plain":                                       # the plain surface painter, bit for bit
                other = blank.cuda()
                ops.render_overlay_yuv(lab_dev, src, pal_dev, _yuv_frames(other, F + 2, H, W, fmt, pitch, crow, rows, lead), 1, a256, contour)
                assert torch.equal(other, out_flat), (pitch, r)
            if fmt == "p010" and name == "mix":                       # kept words keep all 16 bits (make_content sets low bits)
                keep = ~np.isin(TABLES[name][lab], (1, 3))
                assert np.array_equal(wy[keep], ys[keep])
                low += int((wy[keep] & 0x3F != 0).sum())
        assert torch.equal(dev.cpu(), host), (pitch, crow, extra, lead)   # the input allocation, padding included, is unchanged
        (taps, _), (taps_c, _) = tables[5]
        with pytest.raises(RuntimeError, match="render_blur_yuv"):    # in place is refused (MDQE_EINVAL), and nothing is written
            ops.render_blur_yuv(lab_dev, src, pal_dev, acts["all"], taps, taps_c, src, 0, 128, 1, edge="stop")
        if F > 1:
            with pytest.raises(RuntimeError, match="render_blur_yuv"):    # ... and so is an output that meets the input one surface on
                ops.render_blur_yuv(lab_dev[:F - 1], src[:F - 1], pal_dev, acts["all"], taps, taps_c, src, 1, 128, 1, edge="stop")
        assert torch.equal(dev.cpu(), host)
    if fmt == "p010" and H * W > 30:
        assert low > 0
    # the output the wrapper allocates itself (tight), twice: identical from run to run; and the host path says the same
    r, name, contour, a256 = combos[6]
    (taps, _), (taps_c, _) = tables[r]
    wy, wc = want[6]
    got = ops.render_blur_yuv(lab_dev, src, pal_dev, acts[name], taps, taps_c, None, 0, a256, contour, edge="stop")
    assert got.is_cuda and len(got) == F and got.meta() == src.meta() and np.array_equal(_raw(got.y, fmt), wy) and np.array_equal(_raw(got.uv, fmt), wc)
    again = ops.render_blur_yuv(lab_dev, src, pal_dev, acts[name], taps, taps_c, None, 0, a256, contour, edge="stop")
    assert torch.equal(again.y, got.y) and torch.equal(again.uv, got.uv)
    on_host = ops.render_blur_yuv(lab_dev.cpu(), src.to("cpu"), pal, acts[name].cpu(), taps.cpu(), taps_c.cpu(), None, 0, a256, contour, edge="stop")
    assert np.array_equal(_raw(on_host.y, fmt), wy) and np.array_equal(_raw(on_host.uv, fmt), wc)
    assert len(ops.render_blur_yuv(lab_dev[3:], src[3:], pal_dev, acts[name], taps, taps_c, edge="stop")) == 0


@pytest.mark.parametrize("fmt,top", [("nv12", 255), ("p010", 1023)])
def test_the_wide_sum_an_all_1023_surface_at_radius_32(fmt, top):
    from mdqe_cvpr2023_amd import ops
    H, W = 70, 300
    sh = 6 if fmt == "p010" else 0
    dt = np.uint16 if fmt == "p010" else np.uint8
    ys, cs = np.full((2, H, W), top << sh, dtype=dt), np.full((2, H // 2, W), top << sh, dtype=dt)
    lab = OYREF.make_labels(3, 2, H, W)
    pal_np, pal = _yuv_palette(1, fmt)
    pitch, crow, extra, lead = _layouts(H, W, fmt)[0]
    flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
    src = _yuv_frames(torch.from_numpy(flat).cuda(), 2, H, W, fmt, pitch, crow, rows, lead)
    got = ops.render_blur_yuv(torch.from_numpy(lab).cuda(), src, pal.cuda(), torch.from_numpy(TABLES["all"]).cuda(), _taps(32)[0], _taps(16)[0],
                              edge="stop")
    assert (_raw(got.y.cpu(), fmt) == top << sh).all() and (_raw(got.uv.cpu(), fmt) == top << sh).all()


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _paint(labels, frames, style, rows=None):
    """The oracle's picture of a label map in `style` (blur_edge "stop"); rows: [((f0, f1), class rows)] per window for `classes`."""
    pal = style.palette_on("cpu").numpy()
    fr = frames.cpu().numpy()
    taps = _taps(style.blur_radius)[1]
    if style.classes is None:
        return torch.from_numpy(REF.paint(labels.numpy(), fr, pal, style.actions().numpy(), style.a256, style.contour, taps))
    return torch.cat([torch.from_numpy(REF.paint(labels[f0:f1].numpy(), fr[f0:f1], pal, style.actions(c).numpy(), style.a256, style.contour,
                                                 taps)) for (f0, f1), c in rows])


class _BlurSpy:
    """Records the `edge` of every ops.render_blur / ops.render_blur_yuv call ("bleed" where the keyword is not given)."""

    def __init__(self, monkeypatch):
        from mdqe_cvpr2023_amd import ops
        self.edges = []
        for name in ("render_blur", "render_blur_yuv"):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, real):
        def fn(*a, **kw):
            self.edges.append((name, kw.get("edge", "bleed")))
            return real(*a, **kw)
        return fn

    def take(self):
        e, self.edges = self.edges, []
        return e


def test_forward_with_a_stop_style_on_both_paths_and_nothing_else_changes(video, monkeypatch):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    assert int(lm.max()) > 0
    st = Style(blur="background", blur_edge="stop")
    want = _paint(lm, frames, st)
    bleed = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=dataclasses.replace(st, blur_edge="bleed"))
    assert not torch.equal(want, bleed["pred_overlay"]) and not torch.equal(want, base[True]["pred_overlay"])
    spy = _BlurSpy(monkeypatch)
    for early in (True, False):
        got = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=st)
        assert spy.take() == [("render_blur", "stop")] * 3
        assert set(got) == set(base[early]), early
        pic = got["pred_overlay"]
        assert pic.dtype == torch.uint8 and tuple(pic.shape) == (L,) + OUT + (3,) and not pic.is_cuda
        assert torch.equal(got["pred_label_map"], lm) and torch.equal(pic, want), early
        for k in base[early]:                                                 # every other key: the bits of the default style's run
            if k != "pred_overlay":
                assert _same(got[k], base[early][k]), (early, k)
    # the styles without it make the former calls: a blur of tracks with "bleed", the default style no blur at all
    _forward(model, frames, overlay_output=True, label_output=True, overlay_style=Style(blur="tracks"))
    assert spy.take() == [("render_blur", "bleed")] * 3
    again = _forward(model, frames, overlay_output=True, label_output=True)      # the model's own style is back
    assert spy.take() == [] and torch.equal(again["pred_overlay"], base[True]["pred_overlay"])


def test_online_windows_concatenate_to_the_offline_picture(video):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    picked = sorted(set(rows[-1][1].argmax(1)[::2].tolist()))
    for st in (Style(blur="background", blur_edge="stop", alpha=0, contour=0), Style(blur="tracks", classes=picked, blur_radius=3, blur_edge="stop")):
        want = _paint(lm, frames, st, rows)
        for sizes in PLANS:
            ov, wins, _ = _online(model, frames, sizes, emit="overlay", style=st)
            assert [w.frames for w in wins] == [f for f, _ in rows]
            assert torch.equal(torch.cat([w.overlay for w in wins]), want), (st.blur, sizes)
            assert "pred_overlay" not in ov.result()


def test_a_stop_blur_of_tracks_with_a_margin_is_the_reference_on_the_grown_map(video):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    st = Style(blur="tracks", blur_edge="stop", grow=4)
    grown = torch.cat([ops.grow_labels(lm[f0:f1].cuda().contiguous(), st.grows(c).cuda(), st.grow).cpu() for (f0, f1), c in rows])
    assert np.array_equal(grown.numpy(), np.concatenate([GREF.grow(lm[f0:f1].numpy(), st.grows(c).numpy(), st.grow) for (f0, f1), c in rows]))
    assert int((grown != lm).sum()) > 100
    want = _paint(grown, frames, st)
    got = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=st)
    assert torch.equal(got["pred_overlay"], want) and torch.equal(got["pred_label_map"], lm)
    assert not torch.equal(want, _paint(lm, frames, st))


def test_online_nv12_surfaces_with_a_stop_blur(video):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style
    model = video[0]
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda", matrix="bt601", full_range=True, order="bgr")
    before = s.y.clone(), s.uv.clone()
    host = s.to("cpu")
    pushes = (5, 3, 7, 2)
    st = Style(blur="background", blur_edge="stop", alpha=0.25, contour=2, blur_radius=5)
    bleed, _, _ = _session(model, s, pushes, surface=True, style=dataclasses.replace(st, blur_edge="bleed"))
    wins, res, _ = _session(model, s, pushes, surface=True, style=st)
    assert [w.frames for w in wins] == [(0, 6), (6, 12), (12, 17)]
    pal = st.palette_yuv_on("cpu", s.fmt, s.matrix, s.full_range, s.order)
    taps_np, taps_c_np = _taps(st.blur_radius)[1], _taps((st.blur_radius + 1) // 2)[1]
    differs = False
    for win, ref in zip(wins, bleed):
        f0, f1 = win.frames
        assert torch.equal(win.labels, ref.labels)
        pic = win.overlay
        assert isinstance(pic, YuvFrames) and not pic.is_cuda and len(pic) == f1 - f0 and pic.meta() == s.meta()
        wy, wc = REF.paint_yuv(host.y[f0:f1, :, :160].numpy(), host.uv[f0:f1, :, :160].numpy(), win.labels.numpy(),
                               pal.view(torch.int16).numpy().astype(np.int64), st.actions().numpy(), "nv12", st.a256, st.contour,
                               taps_np, taps_c_np)
        assert np.array_equal(pic.y[:, :, :160].numpy(), wy) and np.array_equal(pic.uv[:, :, :160].numpy(), wc), win.frames
        want = ops.render_blur_yuv(win.labels, host[f0:f1], pal, st.actions(), st.taps_on("cpu"), st.taps_c_on("cpu"), None, 0,
                                   st.a256, st.contour, edge="stop")   # ... and the host path says the same
        assert torch.equal(pic.y[:, :, :160], want.y) and torch.equal(pic.uv[:, :, :160], want.uv)
        differs |= not torch.equal(pic.y, ref.overlay.y)
    assert differs
    assert torch.equal(torch.cat([w.overlay.y for w in wins]), res["pred_overlay"].y)
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])           # the caller's surfaces are not painted on
