"""Track paths on the device: mdqe_label_centroids_u8, mdqe_render_trails_u8 and mdqe_render_trails_yuv420sp (ops.label_centroids,
ops.render_trails, ops.render_trails_yuv) against tests/_paths_ref.py, bit for bit; that the trail entries work in place and leave
every other byte alone; the calls that launch nothing and the refused ones; and the layers above them: forward() with
Style(trail=...) and model.path_output, online_video(paths=True), RGB pictures and NV12 surfaces.  Integers only: every comparison is
exact.

Kernel shapes: 37 x 53 (less than one tile each way, nothing divides by 4 or 16; the centroid sweep's second band has 5 rows, so some of
its lanes are idle) and 70 x 150 (several tiles and bands both ways, partial ones on both edges); surfaces of 35 x 51 (odd both ways:
chroma blocks of 1 and 2 pixels) and 36 x 64."""
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

import _paths_ref as REF  # noqa: E402
import _yuv_ref as YREF  # noqa: E402
from test_overlay_gpu import L, PLANS, _forward, _model, _online, _same  # noqa: E402
from test_overlay_yuv_gpu import _frames as _yuv_frames  # noqa: E402
from test_overlay_yuv_gpu import _layouts, _session, _surfaces  # noqa: E402

F = 3
COLS = 70                                                             # columns of the point table: p_off up to 66, F = 3, one guard


def _noise(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _palette(seed):
    return torch.randint(0, 256, (256, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ---- centroids -----------------------------------------------------------------------------------------------------------------------
def _maps(Ho, Wo, n, seed):
    """uint8 [5, Ho, Wo]: rectangles of labels 1..n (and, n < 255, of labels above n, which no row counts) with salt on them; ONE label
    everywhere; per-pixel noise; rectangles again; background only."""
    rng = np.random.default_rng(seed)
    top = max(n, 1)
    lab = np.zeros((5, Ho, Wo), dtype=np.uint8)
    for f in (0, 3):
        for _ in range(14):
            y0, x0 = int(rng.integers(0, Ho)), int(rng.integers(0, Wo))
            lab[f, y0:y0 + int(rng.integers(1, Ho)), x0:x0 + int(rng.integers(1, Wo))] = rng.integers(1, min(top + 3, 255) + 1)
        salt = rng.random((Ho, Wo)) < 0.02
        lab[f][salt] = rng.integers(0, min(top + 3, 255) + 1, size=int(salt.sum()))
    lab[1] = top
    lab[2] = rng.integers(0, min(top + 3, 255) + 1, size=(Ho, Wo))
    return lab


@pytest.mark.parametrize("n", [0, 1, 7, 255])
@pytest.mark.parametrize("Ho,Wo", [(37, 53), (70, 150)])
def test_centroids_against_the_reference_with_garbage_and_guard_columns(Ho, Wo, n):
    from mdqe_cvpr2023_amd import ops
    lab = _maps(Ho, Wo, n, Ho * 1000 + Wo + n)
    if (Ho, Wo, n) == (70, 150, 1):                                   # one label everywhere: SX needs more than 16 bits
        assert int((lab[1] == 1).all()) and sum(range(150)) * 70 == 782250
    dev = torch.from_numpy(lab).cuda()
    for min_area in (0, 50):
        want_mom, want_pts = REF.centroids(lab, n, min_area)
        for p_off in (0, 3):
            mom = torch.full((n, 5, 3), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
            pts = torch.full((n + 1, p_off + 5 + 2, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            got_mom, got_pts = ops.label_centroids(dev, n, min_area, mom, pts, p_off)
            assert got_mom is mom and got_pts is pts
            assert np.array_equal(mom.cpu().numpy(), want_mom), (Ho, Wo, n, min_area)
            p = pts.cpu().numpy()
            assert np.array_equal(p[:n, p_off:p_off + 5], want_pts), (Ho, Wo, n, min_area, p_off)
            assert (p[:n, :p_off] == 0x5A5A5A5A).all() and (p[:n, p_off + 5:] == 0x5A5A5A5A).all() and (p[n:] == 0x5A5A5A5A).all()
        if n:
            present = want_mom[..., 0] >= max(1, min_area)
            assert present.any() and (want_pts[~present] == -1).all() and (want_pts[present] >= 0).all()
    # allocated outputs, the moments alone, identical from run to run
    mom, pts = ops.label_centroids(dev, n, 0)
    assert tuple(mom.shape) == (n, 5, 3) and tuple(pts.shape) == (n, 5, 2)
    mom2, none = ops.label_centroids(dev, n, 0, pts=False)
    assert none is None and torch.equal(mom, mom2) and np.array_equal(pts.cpu().numpy(), REF.centroids(lab, n, 0)[1])


def test_areas_equal_the_label_map_kernels_own_table():
    """One definition of area checked across two kernels: column 0 of the moments is column 0 of the geometry table
    ops.final_label_map writes for the map it makes from random logits."""
    from mdqe_cvpr2023_amd import ops
    n, Fw, Hm, Wm, h, w, Ho, Wo = 7, 5, 24, 40, 90, 150, 70, 150
    logits = torch.randn(n, Fw, Hm, Wm, generator=torch.Generator().manual_seed(4)).cuda()
    idx = torch.arange(n, dtype=torch.int32, device="cuda")
    out, geom = ops.final_label_map(logits, idx, 4, h, w, Ho, Wo, torch.empty(Fw, Ho, Wo, dtype=torch.uint8, device="cuda"), 0, geom=True)
    mom, pts = ops.label_centroids(out, n)
    area = geom.view(n, Fw, 5)[..., 0].cpu()
    assert int(area.sum()) > 1000 and torch.equal(mom[..., 0].cpu(), area.to(torch.int64))
    want_mom, want_pts = REF.centroids(out.cpu().numpy(), n)
    assert np.array_equal(mom.cpu().numpy(), want_mom) and np.array_equal(pts.cpu().numpy(), want_pts)
    g = geom.view(n, Fw, 5).cpu().numpy()                             # a centroid lies in its region's box
    live = want_mom[..., 0] > 0
    assert (want_pts[..., 0][live] >= g[..., 1][live]).all() and (want_pts[..., 0][live] <= g[..., 3][live]).all()


# ---- trails: the RGB kernel ------------------------------------------------------------------------------------------------------------
def _points(Ho, Wo, seed):
    """int32 [n = 12, COLS, 2]: the rows the rule distinguishes."""
    rng = np.random.default_rng(seed)
    t = np.arange(COLS)
    p = np.full((12, COLS, 2), -1, dtype=np.int64)
    p[0] = np.stack([(3 + 2 * t) % Wo, (2 + t) % Ho], 1)              # 1: steady motion (wrapping: a long segment now and then)
    p[1] = np.stack([(Wo - 4 - 2 * t) % Wo, (2 + t) % Ho], 1)         # 2: crosses row 1's line: the lower label wins
    corners = [(0, 0), (Wo - 1, 0), (Wo - 1, Ho - 1), (0, Ho - 1), (Wo // 2, 0), (0, Ho // 2), (Wo - 1, Ho // 2), (Wo // 2, Ho - 1)]
    p[2] = [corners[(j // 2) % 8] for j in t]                         # 3: borders and corners, each held two frames (L2 == 0)
    p[3, COLS - 6] = (Wo // 3, Ho // 3)                               # 4: a lone point
    p[4, ::4] = np.stack([(5 + 3 * t[::4]) % Wo, (Ho - 3 - t[::4]) % Ho], 1)          # 5: gaps of three columns, bridged
    p[5] = rng.integers(-2 ** 31, 2 ** 31, size=(COLS, 2))            # 6: garbage, huge and negative, with a few points in the picture
    p[5, ::5] = np.stack([rng.integers(0, Wo, size=len(t[::5])), rng.integers(0, Ho, size=len(t[::5]))], 1)
    p[6] = np.stack([np.where(t % 3 == 0, Wo, (7 * t) % Wo), np.where(t % 3 == 1, Ho, (5 * t) % Ho)], 1)   # 7: x = Wo, y = Ho: absent
    p[7] = (Wo - 9, Ho - 7)                                           # 8: standing still
    p[8] = np.stack([Wo // 2 + t % 3, (4 * t) % Ho], 1)               # 9: steep
    p[10] = np.stack([np.clip(Wo // 2 + np.cumsum(rng.integers(-3, 4, size=COLS)), 0, Wo - 1),
                      np.clip(Ho // 2 + np.cumsum(rng.integers(-3, 4, size=COLS)), 0, Ho - 1)], 1)         # 11: a random walk
    p[11] = np.stack([rng.integers(0, Wo, size=COLS), rng.integers(0, Ho, size=COLS)], 1)                  # 12: jumps across the picture
    return p.astype(np.int32)                                         # (10: absent throughout)


@pytest.mark.parametrize("Ho,Wo", [(37, 53), (70, 150)])
def test_trails_against_the_reference_in_place_with_guard_frames(Ho, Wo):
    from mdqe_cvpr2023_amd import ops
    pts = _points(Ho, Wo, Ho + Wo)
    n, pal = pts.shape[0], _palette(Ho)
    src = _noise((F + 2, Ho, Wo, 3), Ho * Wo)
    dpts, dpal = torch.from_numpy(pts).cuda(), pal.cuda()
    drawn = 0
    for trail in (1, 5, 64):
        for width in (1, 2, 5):
            for p_off in (2, 66):                                     # p_off + f - trail < 0 for trail 5 and 64; every column there for 64
                if p_off == 66 and trail != 64:
                    continue
                pic = src.cuda()
                assert ops.render_trails(pic, dpts, n, dpal, F, 1, p_off, trail, width) is pic
                want = REF.trails_rgb(src.numpy(), pts, n, pal.numpy(), F, 1, p_off, trail, width)
                # (the whole buffer: the frames before f_off and behind the call keep their bytes)
                assert np.array_equal(pic.cpu().numpy(), want), (Ho, Wo, trail, width, p_off)
                drawn += int((want != src.numpy()).any(-1).sum())
                # pieces: two calls with shifted offsets give the bytes of one; identical from run to run
                two = src.cuda()
                ops.render_trails(two, dpts, n, dpal, 1, 1, p_off, trail, width)
                ops.render_trails(two, dpts, n, dpal, F - 1, 2, p_off + 1, trail, width)
                assert torch.equal(two, pic), (Ho, Wo, trail, width, p_off)
    assert drawn > 3000


def test_reference_line_is_what_the_kernel_draws_for_one_track_and_a_row_strided_table():
    """n == 1 (no stride check applies) and a table whose rows lie further apart than its columns need."""
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 37, 53
    pts = _points(Ho, Wo, 5)
    wide = torch.full((12, COLS + 9, 2), -7, dtype=torch.int32)
    wide[:, :COLS] = torch.from_numpy(pts)
    view = wide.cuda()[:, :COLS]
    assert not view.is_contiguous()
    pal, src = _palette(2), _noise((F, Ho, Wo, 3), 3)
    for n in (1, 12):
        pic = src.cuda()
        ops.render_trails(pic, view, n, pal.cuda(), F, 0, 10, 5, 2)
        assert np.array_equal(pic.cpu().numpy(), REF.trails_rgb(src.numpy(), pts, n, pal.numpy(), F, 0, 10, 5, 2)), n


def test_255_tracks_of_64_segments_in_one_tile_walk_the_list_in_chunks():
    from mdqe_cvpr2023_amd import ops
    Ho, Wo, n, trail = 37, 53, 255, 64
    rng = np.random.default_rng(255)
    cx, cy = (np.arange(n) * 7) % Wo, (np.arange(n) * 3) % Ho         # each track jitters around its own spot: high labels stay visible
    pts = np.stack([np.clip(cx[:, None] + rng.integers(-2, 3, size=(n, trail + 1)), 0, Wo - 1),
                    np.clip(cy[:, None] + rng.integers(-2, 3, size=(n, trail + 1)), 0, Ho - 1)], 2).astype(np.int32)
    pal, src = _palette(6), _noise((1, Ho, Wo, 3), 7)
    rows = {tuple(c): l for l, c in enumerate(pal.tolist())}
    for width in (1, 3):
        pic = src.cuda()
        ops.render_trails(pic, torch.from_numpy(pts).cuda(), n, pal.cuda(), 1, 0, trail, trail, width)
        want = REF.trails_rgb(src.numpy(), pts, n, pal.numpy(), 1, 0, trail, trail, width)
        assert np.array_equal(pic.cpu().numpy(), want), width
        shown = {rows[tuple(c)] for c in want.reshape(-1, 3).tolist() if tuple(c) in rows}
        assert len(shown) > 100 and max(shown) > 150, width            # labels far down the list show: every chunk is walked


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_byte_alignment_of_the_picture(shift):
    from mdqe_cvpr2023_amd import ops
    Ho, Wo = 37, 53
    pts = _points(Ho, Wo, 8)
    pal, src = _palette(3), _noise((F, Ho, Wo, 3), 11)
    nb = src.numel()
    raw = torch.full((nb + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    pic = raw[shift:shift + nb].view(F, Ho, Wo, 3)
    pic.copy_(src)
    assert pic.is_contiguous() and pic.data_ptr() % 4 == shift
    ops.render_trails(pic, torch.from_numpy(pts).cuda(), 12, pal.cuda(), F, 0, 20, 16, 5)
    want = REF.trails_rgb(src.numpy(), pts, 12, pal.numpy(), F, 0, 20, 16, 5)
    r = raw.cpu()
    assert np.array_equal(r[shift:shift + nb].view(F, Ho, Wo, 3).numpy(), want), shift
    assert bool((r[:shift] == 0xAB).all()) and bool((r[shift + nb:] == 0xAB).all())


# ---- trails: the surface kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(35, 51), (36, 64)])
def test_trails_yuv_against_the_reference_padding_and_low_bits_kept(H, W, fmt):
    from mdqe_cvpr2023_amd import ops, render
    pts = _points(H, W, H * W)
    n = pts.shape[0]
    pal_y = render.palette_yuv(_palette(H + W), fmt, "bt601", True, "rgb")
    ys, cs = YREF.make_content(H * 1000 + W, F + 1, H, W, fmt)        # (P010: noise in the low 6 bits of every word)
    dpts, dpal = torch.from_numpy(pts).cuda(), pal_y.cuda()
    combos = [(1, 1, 2), (5, 2, 2), (64, 5, 66), (64, 1, 3)]          # (trail, width, p_off)
    want = [REF.trails_yuv(ys, cs, fmt, H, W, pts, n, pal_y.numpy().astype(np.int64), F, 1, p_off, trail, width) for trail, width, p_off in combos]
    for pitch, crow, extra, lead in _layouts(H, W, fmt):              # tight; padded; padded and entered one sample late
        flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
        for (trail, width, p_off), (wy, wc) in zip(combos, want):
            buf = torch.from_numpy(flat).cuda()
            s = _yuv_frames(buf, F + 1, H, W, fmt, pitch, crow, rows, lead)
            assert ops.render_trails_yuv(s, dpts, n, dpal, F, 1, p_off, trail, width) is s
            # the whole allocation: the padding, surface 0 in front of f_off, and for P010 all 16 bits of every word the rule leaves alone
            assert np.array_equal(buf.cpu().numpy(), YREF.pack(wy, wc, fmt, pitch, crow, extra, lead)[0]), (pitch, crow, lead, trail, width)
    for wy, wc in want:
        assert not np.array_equal(wy, ys) and not np.array_equal(wc, cs)
        assert np.array_equal(wy[0], ys[0]) and np.array_equal(wc[0], cs[0])
        if fmt == "p010":                                             # written words are value << 6, the others kept their noise
            assert bool(((wy != ys) & ((wy & 63) != 0)).sum() == 0) and bool(((wy == ys) & ((wy & 63) != 0)).any())


# ---- calls that launch nothing, calls that are refused ----------------------------------------------------------------------------------
def _entries():
    from mdqe_cvpr2023_amd import _lib
    h = _lib.load_library()

    def cen(F=1, Ho=8, Wo=8, n=1, min_area=0, stride=64, p_off=0):
        return h.mdqe_label_centroids_u8(None, F, Ho, Wo, n, min_area, None, None, stride, p_off, None)

    def rgb(F=1, Ho=8, Wo=8, f_off=0, stride=64, p_off=0, n=1, trail=4, width=2):
        return h.mdqe_render_trails_u8(None, F, Ho, Wo, f_off, None, stride, p_off, n, trail, width, None, None)

    def yuv(F=1, H=32, W=64, f_off=0, stride=64, p_off=0, n=1, trail=4, width=2, fmt=0, yp=64, ys=64 * 48, cp=64, cs=64 * 48):
        return h.mdqe_render_trails_yuv420sp(None, yp, ys, None, cp, cs, F, H, W, fmt, f_off, None, stride, p_off, n, trail, width, None, None)
    return cen, rgb, yuv


def test_calls_that_launch_nothing_return_ok():
    from mdqe_cvpr2023_amd import ops
    cen, rgb, yuv = _entries()
    for call in (cen, rgb, yuv):                                      # (null pointers: a launch would have been refused as MDQE_ENULL first)
        assert call(F=0) == 0 and call(n=0) == 0 and call(F=0, n=0) == 0
        assert call() == 3
    pts = torch.from_numpy(_points(8, 9, 1)).cuda()
    pal, src = _palette(1), _noise((2, 8, 9, 3), 2)
    pic = src.cuda()
    ops.render_trails(pic, pts, 12, pal.cuda(), 0, 1, 5, 4, 2)        # F == 0
    ops.render_trails(pic, pts, 0, pal.cuda(), 2, 0, 5, 4, 2)         # n == 0
    ops.render_trails(pic, pts, 12, pal.cuda(), 2, 0, 0, 64, 5, )     # (something to draw: the picture changes)
    assert not torch.equal(pic.cpu(), src)
    pic = src.cuda()
    ops.render_trails(pic, torch.full_like(pts, -1), 12, pal.cuda(), 2, 0, 5, 4, 2)     # nothing present: no pixel written
    assert torch.equal(pic.cpu(), src)
    lab = torch.zeros(0, 8, 9, dtype=torch.uint8, device="cuda")
    mom, p = ops.label_centroids(lab, 3)
    assert tuple(mom.shape) == (3, 0, 3) and tuple(p.shape) == (3, 0, 2)


def test_every_refused_argument_returns_einval_with_null_pointers():
    cen, rgb, yuv = _entries()
    EINVAL = 1
    shared = ({"n": -1}, {"n": 256}, {"F": -1}, {"p_off": -1}, {"n": 2, "stride": 1}, {"n": 2, "p_off": 32, "stride": 65},
              {"n": 2, "F": 3, "p_off": 30, "stride": 65})
    for call in (cen, rgb, yuv):
        size = ("H", "W") if call is yuv else ("Ho", "Wo")
        for kw in shared + tuple({k: v} for k in size for v in (0, -4, 16385)):
            assert call(**kw) == EINVAL, (call.__name__, kw)
            if "F" not in kw and "n" not in kw:
                assert call(**dict(kw, F=0)) == EINVAL and call(**dict(kw, n=0)) == EINVAL, (call.__name__, kw)   # ... whatever else says "no launch"
        assert call(**{"n": 2, "p_off": 31, "stride": 64}) == 3        # (the smallest stride that is accepted)
    assert cen(min_area=-1) == EINVAL and cen(min_area=-1, n=0) == EINVAL
    assert cen(F=8, Ho=16384, Wo=16384) == EINVAL and cen(F=7, Ho=16384, Wo=16384) == 3
    for call in (rgb, yuv):
        for kw in ({"trail": 0}, {"trail": 65}, {"trail": -1}, {"width": 0}, {"width": 6}, {"f_off": -1}):
            assert call(**kw) == EINVAL, (call.__name__, kw)
            assert call(**dict(kw, F=0)) == EINVAL and call(**dict(kw, n=0)) == EINVAL, (call.__name__, kw)
    assert rgb(F=8, Ho=16384, Wo=16384) == EINVAL
    assert yuv(F=2 ** 15, H=256, W=256, ys=256 * 400, cs=256 * 400, yp=256, cp=256, stride=2 ** 17) == EINVAL                 # F*H*W = 2^31
    # the surface conditions of mdqe_annotate_yuv420sp
    for kw in ({"fmt": 2}, {"fmt": -1}, {"yp": 63}, {"cp": 63}, {"ys": -1}, {"cs": -1}, {"fmt": 1, "yp": 127}, {"fmt": 1, "yp": 129, "cp": 128},
               {"fmt": 1, "yp": 128, "cp": 128, "ys": 128 * 48 + 1}, {"F": 2, "ys": 64 * 32 - 1}, {"F": 2, "cs": 64 * 16 - 1}):
        assert yuv(**kw) == EINVAL, kw
        assert yuv(**dict(kw, n=0)) == EINVAL, kw
    assert yuv(fmt=1, yp=128, cp=128, ys=128 * 48, cs=128 * 48, n=0) == 0 and yuv(F=2, ys=64 * 32, cs=64 * 16, n=0) == 0


# ---- the model -----------------------------------------------------------------------------------------------------------------------
from test_annotate_gpu import _annotated, _pieces, _Spy  # noqa: E402

T, WIDTH = 5, 2                                                       # a trail that reaches back over a whole window of 6 frames but not two


@pytest.fixture(scope="module")
def video():
    """The fixture of test_annotate_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5 frames, many tracks -- and the
    plain run every case here compares with, once."""
    from bench import synth_video
    _, model = _model(n_frames_window_test=6, apply_cls_thres=1e-6)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    base = _forward(model, frames, overlay_output=True, label_output=True)
    lab = base["pred_label_map"].numpy()
    n = int(lab.max())
    assert 0 < n <= 255
    return model, frames, base, n, REF.centroids(lab, n, 0)


def _with_paths(model, frames, **attrs):
    model.path_output = True
    try:
        return _forward(model, frames, **attrs)
    finally:
        model.path_output = False


def _ref_trails(base, pts, n, st):
    return torch.from_numpy(REF.trails_rgb(base["pred_overlay"].numpy(), pts, n, st.palette_on("cpu").numpy(), L, 0, 0, st.trail, st.trail_width))


class _Calls:
    """Every ops function a run calls, by name and in order."""

    def __init__(self, monkeypatch):
        import types
        from mdqe_cvpr2023_amd import ops
        self.names = []
        for name, fn in list(vars(ops).items()):
            if isinstance(fn, types.FunctionType) and not name.startswith("_") and fn.__module__ == ops.__name__:
                monkeypatch.setattr(ops, name, self._counted(name, fn))

    def _counted(self, name, fn):
        def call(*a, **kw):
            self.names.append(name)
            return fn(*a, **kw)
        return call

    def take(self):
        names, self.names = self.names, []
        return names


NEW = ("label_centroids", "render_trails", "render_trails_yuv")


def test_forward_with_a_trail_is_the_reference_over_the_plain_overlay_and_nothing_else_changes(video, monkeypatch):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, n, (_, pts) = video
    st = Style(trail=T, trail_width=WIDTH)
    want = _ref_trails(base, pts, n, st)
    changed = int((want != base["pred_overlay"]).any(-1).sum())
    print("tracks:", n, "trail pixels:", changed)
    assert changed > 200
    calls = _Calls(monkeypatch)
    for early in (True, False):
        plain = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early)
        parent = calls.take()
        assert not set(parent) & set(NEW) and _same(plain, base)      # the defaults: exactly the launches of before
        got = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=st)
        ours = calls.take()
        assert [c for c in ours if c not in NEW] == parent            # the same calls in the same order, and between them ...
        assert ours.count("label_centroids") == ours.count("render_trails") == 3 and "render_trails_yuv" not in ours   # ... one of each per window
        assert set(got) == set(base) and torch.equal(got["pred_overlay"], want), early
        for k in base:                                                # every other key keeps its bits
            if k != "pred_overlay":
                assert _same(got[k], base[k]), (early, k)
    # a longer, wider trail and a min_area that takes small regions out: another picture, the reference's again
    st2 = Style(trail=16, trail_width=5, min_area=40)
    pts2 = REF.centroids(base["pred_label_map"].numpy(), n, 40)[1]
    assert (pts2 != pts).any()
    got = _forward(model, frames, overlay_output=True, overlay_style=st2)
    assert torch.equal(got["pred_overlay"], _ref_trails(base, pts2, n, st2)) and "pred_label_map" not in got


def test_trails_lie_under_boxes_and_captions(video, monkeypatch):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, n, (_, pts) = video
    st = Style(trail=T, trail_width=WIDTH, box=2, caption="id+class+score")
    _, lab_wins, _ = _online(model, frames, [L], emit="labels")
    rows = [(w.frames, w.cls_probs) for w in lab_wins]
    spy = _Spy(monkeypatch)
    got = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=st)
    geoms, calls = spy.take()
    assert calls == 3
    want = _annotated(_ref_trails(base, pts, n, st), geoms, rows, st)  # (annotate-ref applied after trails-ref, window by window)
    assert torch.equal(got["pred_overlay"], want)
    only_notes = _forward(model, frames, overlay_output=True, overlay_style=Style(box=2, caption="id+class+score"))["pred_overlay"]
    assert not torch.equal(only_notes, want)


def test_online_pushes_give_forwards_bytes_across_windows_and_pushes(video, monkeypatch):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, n, (mom, pts) = video
    st = Style(trail=T, trail_width=WIDTH)
    want = _ref_trails(base, pts, n, st)
    calls = _Calls(monkeypatch)
    for sizes in PLANS:
        ov, wins, _ = _online(model, frames, sizes, emit="overlay", style=st)
        ours = calls.take()
        windows = [w.frames for w in wins]
        assert windows == [(0, 6), (6, 12), (12, 17)]
        assert ours.count("label_centroids") == 3 and ours.count("render_trails") == _pieces(sizes, windows), sizes
        assert torch.equal(torch.cat([w.overlay for w in wins]), want), sizes
        assert all(w.centroids is None and w.moments is None for w in wins)       # Style(trail=...) without paths: nothing extra is read back
    ov, wins, _ = _online(model, frames, PLANS[2], emit="overlay")   # Style(): the painter alone
    assert not set(calls.take()) & set(NEW) and torch.equal(torch.cat([w.overlay for w in wins]), base["pred_overlay"])


def test_path_output_offline_and_online_beside_every_form(video):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, n, (mom, pts) = video
    inst = base["pred_track_ids"]
    want_c = torch.from_numpy(np.stack([pts[i] for i in inst]))
    want_m = torch.from_numpy(np.stack([mom[i] for i in inst]))
    assert int((want_c >= 0).all(-1).sum()) > 20
    print("absent (output, frame) pairs:", int((want_c < 0).any(-1).sum()), "of", want_c.shape[0] * L)
    plain = _forward(model, frames)
    for attrs in ({}, {"early_masks": False}, {"label_output": "only"}, {"rle_output": True}, {"overlay_output": True, "label_output": True},
                  {"overlay_output": True, "early_masks": False, "overlay_style": Style(trail=3)}):
        got = _with_paths(model, frames, **attrs)
        ref = _forward(model, frames, **attrs)
        assert set(got) == set(ref) | {"pred_centroids", "pred_moments", "pred_track_ids"}, attrs
        assert got["pred_centroids"].dtype == torch.int32 and got["pred_moments"].dtype == torch.int64
        assert torch.equal(got["pred_centroids"], want_c) and torch.equal(got["pred_moments"], want_m), attrs
        assert got["pred_track_ids"] == inst
        for k in ref:
            assert _same(got[k], ref[k]), (attrs, k)
    assert "pred_centroids" not in plain and "pred_track_ids" not in plain
    for emit in ("masks", "rle", "labels", "overlay"):
        for sizes in (PLANS[0], PLANS[2]):
            ov, wins, _ = _online(model, frames, sizes, emit=emit, paths=True, keep=True)
            for w in wins:
                f0, f1 = w.frames
                k = len(w.track_ids)
                assert w.centroids.dtype == torch.int32 and w.centroids.is_pinned() == bool(k) and tuple(w.centroids.shape) == (k, f1 - f0, 2)
                assert np.array_equal(w.centroids.numpy(), pts[:k, f0:f1]) and np.array_equal(w.moments.numpy(), mom[:k, f0:f1]), (emit, w.frames)
            res = ov.result()
            assert res["pred_track_ids"] == inst and torch.equal(res["pred_centroids"], want_c) and torch.equal(res["pred_moments"], want_m)
    ov, wins, _ = _online(model, frames, PLANS[0], emit="masks", paths=True)
    assert "pred_centroids" not in ov.result() and wins[0].centroids is not None


def test_nv12_surface_session_with_a_trail(video, monkeypatch):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style
    model = video[0]
    st = Style(trail=T, trail_width=3)
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda", matrix="bt601", full_range=True, order="bgr")
    before = s.y.clone(), s.uv.clone()
    pushes = (5, 3, 7, 2)
    plain, res0, _ = _session(model, s, pushes, surface=True)
    calls = _Calls(monkeypatch)
    wins, res, _ = _session(model, s, pushes, surface=True, style=st, paths=True)
    ours = calls.take()
    windows = [w.frames for w in wins]
    assert windows == [(0, 6), (6, 12), (12, 17)] and ours.count("render_trails_yuv") == _pieces(pushes, windows) == 6 and "render_trails" not in ours
    lab = torch.cat([w.labels for w in wins]).numpy()
    n = int(lab.max())
    mom, pts = REF.centroids(lab, n, 0)
    pal = st.palette_yuv_on("cpu", s.fmt, s.matrix, s.full_range, s.order).numpy().astype(np.int64)
    base = YuvFrames.cat([w.overlay for w in plain])
    wy, wc = REF.trails_yuv(base.y.numpy(), base.uv.numpy(), "nv12", 96, 160, pts, n, pal, L, 0, 0, st.trail, st.trail_width)
    got = res["pred_overlay"]
    assert isinstance(got, YuvFrames) and got.meta() == s.meta()
    assert np.array_equal(got.y.numpy(), wy) and np.array_equal(got.uv.numpy(), wc)
    assert int((wy != base.y.numpy()).sum()) > 200
    for w in wins:
        k, (f0, f1) = len(w.track_ids), w.frames
        assert np.array_equal(w.centroids.numpy(), pts[:k, f0:f1]) and np.array_equal(w.moments.numpy(), mom[:k, f0:f1])
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])           # the caller's surfaces are not drawn on
