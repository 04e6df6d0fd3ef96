"""The soft matte and the compositing painter on the device: ops.final_matte (mdqe_final_matte_u8) against the float64 reference of
tests/_matte_ref.py, ops.render_replace (mdqe_render_replace_u8) against its numpy restatement, and the styles above them: forward()
and online_video() with render.Style(replace=...).

The matte.  Bit-certain cases use test_label_map_gpu's logits of +-1, +-2, +-3: with factor 4 every up-sampled value is an exact multiple
of 1/16 in fp32 whatever the order and fusing of the products, so vmax and U are the oracle's, and 255 * sigmoid(gain * k / 16), k =
-48..48, k != 0, stays >= 3.3e-3 levels from a rounding tie for gain in {0.5, 1, 2, 4} (checked in test_matte_cpu.py; fp32 carries
about 6e-5 levels of error) while v == 0 is settled by U: the device plane must EQUAL the float64 reference.  Float logits (randn * 4):
|device - reference| <= 1 everywhere, equality wherever the float64 level lies more than 1e-3 from a half-integer, and at most 0.5 % of
the pixels may lie that close (measured with the CPU fp32 path on these inputs: at most 0.29 %, no mismatch outside, largest
fp32-to-float64 deviation 6.2e-5 levels); U there is the untouched ops.final_label_map's.  The invariant (matte >= 128) == (label map !=
0) is exact in every case.

The painter is integers only: every comparison is exact."""
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

import _matte_ref as REF  # noqa: E402
import _paths_ref as PREF  # noqa: E402
from test_annotate_gpu import _annotated  # noqa: E402
from test_label_map_gpu import FACTOR, SHAPES, _int_logits  # noqa: E402
from test_overlay_gpu import L, OUT, PLANS, _forward, _frames, _label_sets, _model, _online, _palettes, _same  # noqa: E402

GAINS = (0.5, 1.0, 2.0, 4.0)
GUARD = 0xAB


def _take(rows_on):
    t = np.zeros(256, dtype=np.uint8)
    for r in rows_on:
        t[r + 1] = 1
    return t


def _run_matte(dev, rows, shape, take, gain, f_off=2, shift=0):
    """One launch into a plane that starts `shift` bytes behind an aligned address, guard frames around -> the Fw frames on the host."""
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    Fw = int(dev.shape[1])
    nb = (f_off + Fw + 1) * Ho * Wo
    raw = torch.full((nb + 8,), GUARD, dtype=torch.uint8, device="cuda")
    out = raw[shift:shift + nb].view(f_off + Fw + 1, Ho, Wo)
    assert out.data_ptr() % 4 == shift
    idx = torch.tensor(rows, dtype=torch.int32, device="cuda")
    t = None if take is None else torch.from_numpy(take).cuda()
    assert ops.final_matte(dev, idx, FACTOR, h, w, Ho, Wo, out, f_off, t, gain) is out
    r = raw.cpu()
    o = r[shift:shift + nb].view(f_off + Fw + 1, Ho, Wo)
    assert bool((r[:shift] == GUARD).all()) and bool((r[shift + nb:] == GUARD).all())
    assert bool((o[:f_off] == GUARD).all()) and bool((o[f_off + Fw:] == GUARD).all())           # the guard frames
    return o[f_off:f_off + Fw]


def _label_map(dev, rows, shape):
    from mdqe_cvpr2023_amd import ops
    Hm, Wm, h, w, Ho, Wo = shape
    out = torch.empty((int(dev.shape[1]), Ho, Wo), dtype=torch.uint8, device="cuda")
    ops.final_label_map(dev, torch.tensor(rows, dtype=torch.int32, device="cuda"), FACTOR, h, w, Ho, Wo, out, 0)
    return out.cpu()


@pytest.mark.parametrize("shape", SHAPES)
def test_matte_equals_the_float64_reference_on_integer_logits(shape):
    Hm, Wm, h, w, Ho, Wo = shape
    n, Fw = 5, 3
    lg = _int_logits(n, Fw, Hm, Wm, seed=Hm + Wo)
    dev = lg.cuda()
    k = 0
    for rows in ([0, 1, 2, 3, 4], [3, 0, 4, 1]):
        v, bits = REF.oracle_values(lg[rows], h, w, Ho, Wo)
        seen = set()
        for take in (None, _take([1, 4]), _take([])):                 # every row; a table that drops some; one that drops all
            part = REF.participating(rows, take)
            lab = _label_map(dev, [rows[i] for i in part], shape)
            for gain in GAINS:
                want, level, vmax = REF.matte(v[part], bits[part], gain)
                got = _run_matte(dev, rows, shape, take, gain, shift=k % 4)
                k += 1
                assert torch.equal(got, torch.from_numpy(want)), (shape, rows, gain, None if take is None else part)
                assert torch.equal(got >= 128, lab != 0)              # the hard mask's edge, bit for bit
                if take is None:
                    seen |= set(np.unique(want).tolist())
                    assert int((vmax == 0).sum()) >= 1                # a pixel only U settles
                if not part:
                    assert int(got.max()) == 0
        assert {0, 255} <= seen and len(seen) > 20
        again = _run_matte(dev, rows, shape, None, 2.0)
        assert torch.equal(again, _run_matte(dev, rows, shape, None, 2.0))                      # identical from run to run


@pytest.mark.parametrize("n_sel,shape", [(0, (16, 24, 60, 90, 60, 90)), (1, (16, 24, 60, 90, 61, 97)), (255, (8, 12, 32, 48, 33, 47))])
def test_matte_with_no_one_and_255_rows(n_sel, shape):
    Hm, Wm, h, w, Ho, Wo = shape
    Fw = 2
    lg = _int_logits(n_sel, Fw, Hm, Wm, seed=n_sel) if n_sel else torch.zeros(0, Fw, Hm, Wm)
    rows = torch.randperm(n_sel, generator=torch.Generator().manual_seed(n_sel)).tolist()
    dev = lg.cuda()
    v, bits = REF.oracle_values(lg[rows], h, w, Ho, Wo)
    takes = [None] + ([_take(rows[::3])] if n_sel == 255 else [])
    for i, take in enumerate(takes):
        part = REF.participating(rows, take)
        for gain in (1.0, 4.0):
            want = REF.matte(v[part], bits[part], gain)[0]
            got = _run_matte(dev, rows, shape, take, gain, shift=1 + i)
            assert torch.equal(got, torch.from_numpy(want)), (n_sel, gain)
            assert torch.equal(got >= 128, _label_map(dev, [rows[j] for j in part], shape) != 0)
    if n_sel == 0:
        assert int(got.max()) == 0                                    # a window without tracks: zeros, as the label map


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_matte_on_float_logits(shape, seed):
    Hm, Wm, h, w, Ho, Wo = shape
    n, Fw = 5, 3
    lg = torch.randn(n, Fw, Hm, Wm, generator=torch.Generator().manual_seed(seed)) * 4
    dev = lg.cuda()
    rows = list(range(n))
    v, _ = REF.oracle_values(lg, h, w, Ho, Wo)
    for take in (None, _take([0, 2, 3])):
        part = REF.participating(rows, take)
        U = (_label_map(dev, [rows[i] for i in part], shape) != 0).numpy()      # the untouched kernel's bits
        for gain in (1.0, 0.37, 3.0):
            level = 255.0 / (1.0 + np.exp(-float(np.float32(gain)) * v[part].max(0)))
            a = np.rint(level).astype(np.int64)
            want = np.where(U, np.maximum(a, 128), np.minimum(a, 127))
            got = _run_matte(dev, rows, shape, take, gain, shift=seed + 1).numpy().astype(np.int64)
            near = np.abs(level - np.floor(level) - 0.5) <= 1e-3
            worst, share = int(np.abs(got - want).max()), float(near.mean())
            print("shape %s seed %d gain %.2f: max |dev - ref| %d, within 1e-3 of a tie %.4f %%, mismatches outside %d"
                  % (shape, seed, gain, worst, 100 * share, int((got != want)[~near].sum())))
            assert worst <= 1
            assert np.array_equal(got[~near], want[~near])
            assert share <= 0.005
            assert np.array_equal(got >= 128, U)                      # exact on float logits too


def test_final_matte_refuses_bad_arguments():
    from mdqe_cvpr2023_amd import ops
    lg = torch.zeros(2, 1, 4, 6, device="cuda")
    idx = torch.arange(2, dtype=torch.int32, device="cuda")
    out = torch.full((1, 16, 24), GUARD, dtype=torch.uint8, device="cuda")
    for gain in (0.0, -1.0, 64.5, float("nan"), float("inf"), True):
        with pytest.raises(RuntimeError, match="gain"):
            ops.final_matte(lg, idx, 4, 16, 24, 16, 24, out, 0, None, gain)
    with pytest.raises(RuntimeError, match="take"):
        ops.final_matte(lg, idx, 4, 16, 24, 16, 24, out, 0, torch.zeros(255, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="out"):
        ops.final_matte(lg, idx, 4, 16, 24, 16, 24, out, 1)
    assert bool((out == GUARD).all())
    ops.final_matte(torch.zeros(2, 0, 4, 6, device="cuda"), idx, 4, 16, 24, 16, 24, out, 1)   # Fw == 0: nothing to do
    assert bool((out == GUARD).all())


# ---- the RGB painter -----------------------------------------------------------------------------------------------------------------
SIZES = [(61, 97, 61, 97), (60, 90, 120, 180), (96, 160, 61, 97)]      # (h0, w0, Ho, Wo): equal, up- and down-sampled
F = 3


def _actions(seed=0):
    rng = np.random.default_rng(seed)
    bg = np.ones(256, dtype=np.uint8)
    bg[0] = 4
    tr = np.full(256, 4, dtype=np.uint8)
    tr[0] = 0
    return {"background": bg, "tracks": tr, "mix": np.array([0, 1, 4, 2], dtype=np.uint8)[rng.integers(0, 4, size=256)]}


@pytest.mark.parametrize("kind", ["u8", "f32", "none", "strided"])
@pytest.mark.parametrize("size", SIZES)
def test_render_replace_against_the_reference(size, kind):
    from mdqe_cvpr2023_amd import ops
    h0, w0, Ho, Wo = size
    sets = _label_sets(Ho, Wo, seed=Ho * 1000 + Wo)
    fr_dev, fr_np = _frames(kind, F, h0, w0, seed=h0 + w0)
    pals, acts = _palettes(), _actions()
    mat = REF.ramp_matte(F, Ho, Wo, seed=Ho + Wo)
    assert {0, 255} <= set(np.unique(mat).tolist()) and len(np.unique(mat)) == 256
    rng = np.random.default_rng(Ho)
    backs = [np.array([0, 255, 0], dtype=np.uint8), rng.integers(0, 256, size=(Ho, Wo, 3)).astype(np.uint8)]
    mat_dev = torch.from_numpy(mat).cuda()
    k = 0
    for name, act in acts.items():
        for mode in (0, 1):
            for back in backs:
                for contour in (0, 2):
                    lab, pal, f_off, a256 = sets[k % 2], pals[(k // 2) % 2], 1 - k % 2, (128, 0, 256, 77)[k % 4]
                    out = torch.full((f_off + F + 1, Ho, Wo, 3), GUARD, dtype=torch.uint8, device="cuda")
                    lab_dev = torch.from_numpy(lab).cuda()
                    got = ops.render_replace(lab_dev, fr_dev, pal.cuda(), torch.from_numpy(act).cuda(), mat_dev, torch.from_numpy(back).cuda(),
                                             out, f_off, a256, contour, ops.REPLACE_MODES[mode])
                    assert got is out
                    o = out.cpu()
                    want = REF.replace_rgb(lab, fr_np, pal.numpy(), act, mat, back, a256, contour, mode)
                    assert torch.equal(o[f_off:f_off + F], torch.from_numpy(want)), (size, kind, name, mode, back.shape, contour, a256)
                    assert bool((o[:f_off] == GUARD).all()) and bool((o[f_off + F:] == GUARD).all())
                    if kind == "u8" and h0 == Ho:                     # full weight and a kept label: the source byte itself
                        wt = 255 - mat if mode else mat
                        keep = (wt == 255) & (act[lab] != 1)
                        assert keep.any() and np.array_equal(o[f_off:f_off + F].numpy()[keep], np.moveaxis(fr_np, 1, -1)[keep])
                    k += 1
    assert k == 24
    # a matte of 255 everywhere in mode "background" with the plain table is the plain overlay, bit for bit
    plain = np.ones(256, dtype=np.uint8)
    plain[0] = 0
    full = torch.full((F, Ho, Wo), 255, dtype=torch.uint8, device="cuda")
    a = torch.empty((F, Ho, Wo, 3), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    lab_dev = torch.from_numpy(sets[0]).cuda()
    ops.render_replace(lab_dev, fr_dev, pals[0].cuda(), torch.from_numpy(plain).cuda(), full, torch.from_numpy(backs[0]).cuda(), a, 0, 128, 1)
    ops.render_overlay(lab_dev, fr_dev, pals[0].cuda(), b, 0, 128, 1)
    assert torch.equal(a, b)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_alignment_of_the_output_and_runs_are_identical(shift):
    from mdqe_cvpr2023_amd import ops
    pal, act = _palettes()[1], _actions()["mix"]
    for n, Ho, Wo in ((2, 13, 9), (1, 1, 2), (1, 2, 3), (1, 1, 1), (1, 20, 132)):
        rng = np.random.default_rng(n * Ho + Wo)
        lab = rng.integers(0, 256, size=(n, Ho, Wo)).astype(np.uint8)
        mat = rng.integers(0, 256, size=(n, Ho, Wo)).astype(np.uint8)
        back = rng.integers(0, 256, size=(Ho, Wo, 3)).astype(np.uint8)
        fr = torch.randint(0, 256, (n, 3, Ho, Wo), generator=torch.Generator().manual_seed(Ho), dtype=torch.uint8)
        nb = n * Ho * Wo * 3
        raw = torch.full((nb + 8,), GUARD, dtype=torch.uint8, device="cuda")
        out = raw[shift:shift + nb].view(n, Ho, Wo, 3)
        assert out.is_contiguous() and out.data_ptr() % 4 == shift
        # the label map, the matte and the backdrop picture at every alignment too: views one byte further in
        def odd(a):
            t = torch.zeros(a.size + 4, dtype=torch.uint8, device="cuda")
            v = t[shift:shift + a.size].view(a.shape)
            v.copy_(torch.from_numpy(a))
            return v
        args = (odd(lab), fr.cuda(), pal.cuda(), torch.from_numpy(act).cuda(), odd(mat), odd(back))
        ops.render_replace(*args, out, 0, 77, 2, "tracks")
        want = torch.from_numpy(REF.replace_rgb(lab, fr.numpy(), pal.numpy(), act, mat, back, 77, 2, 1))
        r = raw.cpu()
        assert torch.equal(r[shift:shift + nb].view(n, Ho, Wo, 3), want), (shift, n, Ho, Wo)
        assert bool((r[:shift] == GUARD).all()) and bool((r[shift + nb:] == GUARD).all())
        again = torch.empty_like(out)
        ops.render_replace(*args, again, 0, 77, 2, "tracks")
        assert torch.equal(again, out)                                # identical from run to run


def test_render_replace_refusals_and_no_frames_is_no_launch():
    from mdqe_cvpr2023_amd import ops
    pal, act = _palettes()[0].cuda(), torch.from_numpy(_actions()["background"]).cuda()
    out = torch.full((2, 4, 5, 3), GUARD, dtype=torch.uint8, device="cuda")
    col = torch.tensor([1, 2, 3], dtype=torch.uint8, device="cuda")
    none = torch.zeros(0, 4, 5, dtype=torch.uint8, device="cuda")
    ops.render_replace(none, None, pal, act, none, col, out, 1)
    assert bool((out == GUARD).all())
    lab = torch.zeros(1, 4, 5, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="matte"):
        ops.render_replace(lab, None, pal, act, torch.zeros(1, 4, 6, dtype=torch.uint8, device="cuda"), col, out)
    with pytest.raises(RuntimeError, match="backdrop"):
        ops.render_replace(lab, None, pal, act, lab, torch.zeros(4, 6, 3, dtype=torch.uint8, device="cuda"), out)
    with pytest.raises(RuntimeError, match="backdrop"):
        ops.render_replace(lab, None, pal, act, lab, col.cpu(), out)
    with pytest.raises(RuntimeError, match="mode"):
        ops.render_replace(lab, None, pal, act, lab, col, out, mode="both")
    assert bool((out == GUARD).all())


# ---- the surface painter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "p010"])
@pytest.mark.parametrize("H,W", [(61, 97), (64, 96)])
def test_render_replace_yuv_against_the_reference(H, W, fmt):
    import _overlay_yuv_ref as OYREF
    import _yuv_ref as YREF
    from mdqe_cvpr2023_amd import ops
    from test_overlay_yuv_gpu import _frames as _yuv_frames
    from test_overlay_yuv_gpu import _layouts, _raw, _typed
    from test_overlay_yuv_gpu import _palette as _yuv_palette
    SENT = 0xCD
    ys, cs = YREF.make_content(H * 1000 + W, F, H, W, fmt)
    bys, bcs = YREF.make_content(H + W, 1, H, W, fmt)                  # the backdrop surface
    lab = OYREF.make_labels(H * 7 + W, F, H, W)
    mat = REF.ramp_matte(F, H, W, seed=H)
    lab[2, 10:20, 10:30] = 0
    mat[2, 10:20, 10:30] = 255                                        # whole blocks kept at full weight (mode "background")
    pal_np, pal = _yuv_palette(H + W, fmt)
    top = 255 if fmt == "nv12" else 1023
    colour_np = (top, 3, top // 2)
    colour = torch.tensor(colour_np, dtype=torch.int32).to(torch.uint16).cuda()
    acts = _actions()
    combos = [(name, mode, surf, (0, 2)[k % 2], (128, 0, 256, 77)[k % 4])
              for k, (name, mode, surf) in enumerate((n, m, sf) for n in acts for m in (0, 1) for sf in (False, True))]
    want = [REF.replace_yuv(ys, cs, lab, pal_np, acts[n], mat, (bys[0], bcs[0]) if sf else colour_np, fmt, a256, contour, m)
            for n, m, sf, contour, a256 in combos]
    lab_dev, mat_dev, pal_dev = torch.from_numpy(lab).cuda(), torch.from_numpy(mat).cuda(), pal.cuda()
    acts_dev = {k: torch.from_numpy(v).cuda() for k, v in acts.items()}
    low = 0
    for li, (pitch, crow, extra, lead) in enumerate(_layouts(H, W, fmt)):  # tight; padded; entered one sample late
        flat, rows = YREF.pack(ys, cs, fmt, pitch, crow, extra, lead)
        host = torch.from_numpy(flat)
        dev = host.cuda()
        src = _yuv_frames(dev, F, H, W, fmt, pitch, crow, rows, lead)
        bflat, brows = YREF.pack(bys, bcs, fmt, pitch, crow, extra, lead)
        bdev = torch.from_numpy(bflat).cuda()
        back = _yuv_frames(bdev, 1, H, W, fmt, pitch, crow, brows, lead)
        blank = torch.full((lead + (F + 2) * rows * pitch,), SENT, dtype=torch.uint8)
        for ci, ((name, mode, surf, contour, a256), (wy, wc)) in enumerate(zip(combos, want)):
            expect = blank.clone()
            e = _yuv_frames(expect, F + 2, H, W, fmt, pitch, crow, rows, lead)
            e.y[1:1 + F, :, :W] = _typed(wy, fmt)
            e.uv[1:1 + F, :, :wc.shape[2]] = _typed(wc, fmt)
            out_flat = blank.cuda()
            out = _yuv_frames(out_flat, F + 2, H, W, fmt, pitch, crow, rows, lead)
            args = (lab_dev, src, pal_dev, acts_dev[name], mat_dev, back if surf else colour)
            assert ops.render_replace_yuv(*args, out, 1, a256, contour, ops.REPLACE_MODES[mode]) is out           # f_off = 1, sentinels around
            assert torch.equal(out_flat.cpu(), expect), (pitch, crow, extra, lead, name, mode, surf, contour, a256)
            if (ci + li) % 4 == 0:                                    # in place: the same samples, the padding untouched
                own_flat = dev.clone()
                own = _yuv_frames(own_flat, F, H, W, fmt, pitch, crow, rows, lead)
                ops.render_replace_yuv(lab_dev, own, pal_dev, acts_dev[name], mat_dev, back if surf else colour, own, 0, a256, contour,
                                       ops.REPLACE_MODES[mode])
                assert np.array_equal(_raw(own.y[:, :, :W], fmt), wy) and np.array_equal(_raw(own.uv[:, :, :wc.shape[2]], fmt), wc)
                pe = host.clone()
                pv = _yuv_frames(pe, F, H, W, fmt, pitch, crow, rows, lead)
                pv.y[:, :, :W] = _typed(wy, fmt)
                pv.uv[:, :, :wc.shape[2]] = _typed(wc, fmt)
                assert torch.equal(own_flat.cpu(), pe)
            if fmt == "p010":                                         # words the rule leaves alone keep all 16 bits; the others lose the low 6
                wt = 255 - mat.astype(np.int64) if mode else mat.astype(np.int64)
                kept = (acts[name][lab] != 1) & (wt == 255)
                assert np.array_equal(wy[kept], ys[kept]) and (wy[~kept] & 0x3F == 0).all()
                low += int((wy[kept] & 0x3F != 0).sum())
                if mode == 0 and name != "mix":
                    assert np.array_equal(wc[2, 5:10, 10:30], cs[2, 5:10, 10:30])                 # chroma pairs of wholly kept blocks
        assert torch.equal(dev.cpu(), host) and torch.equal(bdev.cpu(), torch.from_numpy(bflat))  # the inputs are unchanged
        # the overlap refusals: an output that meets the input one surface on, the backdrop surface, or the matte
        with pytest.raises(RuntimeError, match="render_replace_yuv"):
            ops.render_replace_yuv(lab_dev[:F - 1], src[:F - 1], pal_dev, acts_dev["mix"], mat_dev[:F - 1], colour, src, 1, 128, 1)
        with pytest.raises(RuntimeError, match="render_replace_yuv"):
            ops.render_replace_yuv(lab_dev[:1], src[:1], pal_dev, acts_dev["mix"], mat_dev[:1], back, back, 0, 128, 1)
        assert torch.equal(dev.cpu(), host) and torch.equal(bdev.cpu(), torch.from_numpy(bflat))
    if fmt == "p010":
        assert low > 0
    # the output the wrapper allocates itself (tight), twice: identical from run to run
    name, mode, surf, contour, a256 = combos[5]
    wy, wc = want[5]
    got = ops.render_replace_yuv(lab_dev, src, pal_dev, acts_dev[name], mat_dev, back if surf else colour, None, 0, a256, contour, ops.REPLACE_MODES[mode])
    assert got.is_cuda and len(got) == F and got.meta() == src.meta() and np.array_equal(_raw(got.y, fmt), wy) and np.array_equal(_raw(got.uv, fmt), wc)
    again = ops.render_replace_yuv(lab_dev, src, pal_dev, acts_dev[name], mat_dev, back if surf else colour, None, 0, a256, contour, ops.REPLACE_MODES[mode])
    assert torch.equal(again.y, got.y) and torch.equal(again.uv, got.uv)
    assert len(ops.render_replace_yuv(lab_dev[3:], src[3:], pal_dev, acts_dev[name], mat_dev[3:], colour)) == 0


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class _Logits:
    """Wraps ops.final_label_map: a copy of every window's logits and the arguments the map was made with, in window order; and counts
    the calls of the painters and of ops.final_matte."""

    def __init__(self, monkeypatch):
        from mdqe_cvpr2023_amd import ops
        self.windows, self.calls = [], {}
        real_map = ops.final_label_map

        def label_map(logits, inst_idx, factor, h, w, Ho, Wo, out, f_off, geom=None):
            self.windows.append((logits.clone(), factor, h, w, Ho, Wo))
            return real_map(logits, inst_idx, factor, h, w, Ho, Wo, out, f_off, geom=geom)
        monkeypatch.setattr(ops, "final_label_map", label_map)
        for name in ("final_matte", "render_replace", "render_replace_yuv", "render_overlay", "render_overlay_yuv", "render_mosaic",
                     "render_blur"):
            monkeypatch.setattr(ops, name, self._counted(name, getattr(ops, name)))

    def _counted(self, name, real):
        def fn(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return real(*a, **kw)
        return fn

    def take(self):
        w, c = self.windows, self.calls
        self.windows, self.calls = [], {}
        return w, c


@pytest.fixture(scope="module")
def video():
    """The fixture of test_blur_gpu.py: 17 frames of 96 x 160, output 90 x 150, windows of 6, 6 and 5 frames, many tracks; the run with
    the default style, and the windows' class rows from an online session."""
    from bench import synth_video
    _, model = _model(n_frames_window_test=6, apply_cls_thres=1e-6)
    frames = synth_video(0, L, seed=1, h=96, w=160, n_obj=4).cuda()
    base = {early: _forward(model, frames, overlay_output=True, label_output=True, early_masks=early) for early in (True, False)}
    _, wins, _ = _online(model, frames, [L], emit="labels")
    rows = [(w.frames, w.cls_probs) for w in wins]
    assert [f for f, _ in rows] == [(0, 6), (6, 12), (12, 17)]
    return model, frames, base, rows


def _styles(rows):
    from mdqe_cvpr2023_amd.render import Style
    last = rows[-1][1]
    picked = sorted(set(last.argmax(1)[::2].tolist()))
    back = torch.randint(0, 256, OUT + (3,), generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
    return {"background": Style(replace="background"),
            "tracks": Style(replace="tracks", backdrop=(10, 20, 250), matte_gain=2.0, contour=2),
            "picture": Style(replace="background", backdrop=back, alpha=0, contour=0, matte_gain=0.5),
            "classes": Style(replace="tracks", classes=picked), "virtual": Style(replace="background", classes=picked)}


def _by_hand(windows, rows, lm, frames, style):
    """The picture of a replace style from the three ops called by hand on the windows' logits (on the device), window by window."""
    from mdqe_cvpr2023_amd import ops
    pics = []
    for (lg, factor, h, w, Ho, Wo), ((f0, f1), cls) in zip(windows, rows):
        n, nf = int(lg.shape[0]), f1 - f0
        assert int(lg.shape[1]) == nf and n == int(cls.shape[0])
        idx = torch.arange(n, dtype=torch.int32, device="cuda")
        lab = torch.empty((nf, Ho, Wo), dtype=torch.uint8, device="cuda")
        ops.final_label_map(lg, idx, factor, h, w, Ho, Wo, lab, 0)
        assert torch.equal(lab.cpu(), lm[f0:f1])
        mat = ops.final_matte(lg, idx, factor, h, w, Ho, Wo, torch.empty_like(lab), 0, style.takes(cls).cuda(), style.matte_gain)
        pic = torch.empty((nf, Ho, Wo, 3), dtype=torch.uint8, device="cuda")
        ops.render_replace(lab, frames[f0:f1], style.palette_on("cuda"), style.actions(cls).cuda(), mat, style.backdrop_on("cuda"), pic, 0,
                           style.a256, style.contour, style.replace)
        # ... and the references on the host say the same about the painter
        back = style.backdrop_on("cpu").numpy()
        want = REF.replace_rgb(lab.cpu().numpy(), frames[f0:f1].cpu().numpy(), style.palette_on("cpu").numpy(), style.actions(cls).numpy(),
                               mat.cpu().numpy(), back, style.a256, style.contour, ops.REPLACE_MODES.index(style.replace))
        assert torch.equal(pic.cpu(), torch.from_numpy(want))
        pics.append(pic.cpu())
    return torch.cat(pics)


@pytest.fixture(scope="module")
def logits(video):
    """The windows' logits of the fixture's video, taken once from a run with the default style."""
    model, frames, base, rows = video
    mp = pytest.MonkeyPatch()
    try:
        spy = _Logits(mp)
        _forward(model, frames, overlay_output=True, label_output=True)
        windows, calls = spy.take()
    finally:
        mp.undo()
    assert len(windows) == 3 and calls == {"render_overlay": 3}       # the default style: exactly the plain ops
    return windows


def test_forward_with_a_replace_style_on_both_paths_and_nothing_else_changes(video, logits):
    model, frames, base, rows = video
    styles = _styles(rows)
    lm = base[True]["pred_label_map"]
    assert int(lm.max()) > 0
    tables = [styles["virtual"].actions(c)[1:int(c.shape[0]) + 1].tolist() for _, c in rows]
    assert any(4 in t for t in tables) and any(1 in t for t in tables)               # some tracks are kept and some go
    seen = []
    for name, st in styles.items():
        want = _by_hand(logits, rows, lm, frames, st)
        assert not torch.equal(want, base[True]["pred_overlay"]) and all(not torch.equal(want, s) for s in seen), name
        seen.append(want)
        for early in (True, False):
            got = _forward(model, frames, overlay_output=True, label_output=True, early_masks=early, overlay_style=st)
            assert set(got) == set(base[early]), (name, early)
            pic = got["pred_overlay"]
            assert pic.dtype == torch.uint8 and tuple(pic.shape) == (L,) + OUT + (3,) and not pic.is_cuda
            assert torch.equal(got["pred_label_map"], lm) and torch.equal(pic, want), (name, early)
            for k in base[early]:                                                     # every other key: the bits of the default style's run
                if k != "pred_overlay":
                    assert _same(got[k], base[early][k]), (name, early, k)
    again = _forward(model, frames, overlay_output=True, label_output=True)          # the model's own style is back
    assert torch.equal(again["pred_overlay"], base[True]["pred_overlay"])


def test_online_windows_concatenate_to_the_offline_picture(video, logits):
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    styles = _styles(rows)
    for name in ("background", "classes", "picture"):
        st = styles[name]
        want = _by_hand(logits, rows, lm, frames, st)
        for sizes in PLANS:
            ov, wins, _ = _online(model, frames, sizes, emit="overlay", style=st)
            assert [w.frames for w in wins] == [f for f, _ in rows]
            for w in wins:
                assert torch.equal(w.labels, lm[w.frames[0]:w.frames[1]])
            assert torch.equal(torch.cat([w.overlay for w in wins]), want), (name, sizes)


def test_a_replacement_lies_under_trails_boxes_and_captions(video, logits, monkeypatch):
    from mdqe_cvpr2023_amd.render import Style
    from test_annotate_gpu import _Spy
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    n = int(lm.max())
    st = Style(replace="background", trail=5, trail_width=2, box=2, caption="id+class+score")
    pts = PREF.centroids(lm.numpy(), n, 0)[1]
    replaced = _by_hand(logits, rows, lm, frames, Style(replace="background"))
    trailed = torch.from_numpy(PREF.trails_rgb(replaced.numpy(), pts, n, st.palette_on("cpu").numpy(), L, 0, 0, st.trail, st.trail_width))
    spy = _Spy(monkeypatch)
    got = _forward(model, frames, overlay_output=True, label_output=True, overlay_style=st)
    geoms, calls = spy.take()
    assert calls == 3
    want = _annotated(trailed, geoms, rows, st)
    assert torch.equal(got["pred_overlay"], want) and torch.equal(got["pred_label_map"], lm)
    assert not torch.equal(trailed, replaced) and not torch.equal(want, trailed)


def test_the_ops_called_are_the_replace_ones_and_the_default_style_keeps_the_plain_ones(video, monkeypatch):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    spy = _Logits(monkeypatch)
    _forward(model, frames, overlay_output=True, label_output=True, overlay_style=Style(replace="tracks"))
    assert spy.take()[1] == {"final_matte": 3, "render_replace": 3}
    _online(model, frames, [L], emit="overlay")
    assert spy.take()[1] == {"render_overlay": 3}
    _forward(model, frames, overlay_output=True, label_output=True, overlay_style=Style(mosaic="tracks"))
    assert spy.take()[1] == {"render_mosaic": 3}


def test_refusals_of_the_replace_style_at_the_model(video):
    from mdqe_cvpr2023_amd.render import Style
    model, frames, base, rows = video
    wrong = torch.zeros(OUT[0] + 1, OUT[1], 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="resize the picture"):
        _forward(model, frames, overlay_output=True, overlay_style=Style(replace="background", backdrop=wrong))
    again = _forward(model, frames, overlay_output=True, label_output=True)
    assert torch.equal(again["pred_overlay"], base[True]["pred_overlay"])


def test_an_nv12_session_replaces_the_tracks_of_some_classes(video, monkeypatch):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd.preprocess import YuvFrames
    from mdqe_cvpr2023_amd.render import Style
    from test_overlay_yuv_gpu import _session, _surfaces
    model, frames, base, rows = video
    picked = sorted(set(rows[-1][1].argmax(1)[::2].tolist()))
    s = _surfaces(96, 160, "nv12", 256, 128, "cuda", matrix="bt601", full_range=True, order="bgr")
    before = s.y.clone(), s.uv.clone()
    backdrop = s[3:4].to("cuda")                                      # one surface of the session's kind as the backdrop
    spy = _Logits(monkeypatch)
    for st in (Style(replace="tracks", classes=picked), Style(replace="background", backdrop=backdrop, matte_gain=2.0)):
        wins, res, _ = _session(model, s, (5, 3, 7, 2), surface=True, style=st)
        windows, calls = spy.take()
        # (one matte sweep per window, one painter launch per piece of pushed surfaces)
        assert set(calls) == {"final_matte", "render_replace_yuv"} and calls["final_matte"] == 3 and calls["render_replace_yuv"] >= 3
        assert [w.frames for w in wins] == [(0, 6), (6, 12), (12, 17)]
        pal = st.palette_yuv_on("cuda", s.fmt, s.matrix, s.full_range, s.order)
        back = st.backdrop_yuv_on("cuda", s.fmt, s.matrix, s.full_range, s.order)
        differs = False
        for win, (lg, factor, h, w, Ho, Wo) in zip(wins, windows):
            f0, f1 = win.frames
            c = win.cls_probs
            pic = win.overlay
            assert isinstance(pic, YuvFrames) and not pic.is_cuda and len(pic) == f1 - f0 and pic.meta() == s.meta()
            idx = torch.arange(int(lg.shape[0]), dtype=torch.int32, device="cuda")
            lab = win.labels.cuda()
            mat = ops.final_matte(lg, idx, factor, h, w, Ho, Wo, torch.empty_like(lab), 0, st.takes(c).cuda(), st.matte_gain)
            want = ops.render_replace_yuv(lab, s[f0:f1], pal, st.actions(c).cuda(), mat, back, None, 0, st.a256, st.contour, st.replace)
            assert torch.equal(pic.y[:, :, :160], want.y.cpu()) and torch.equal(pic.uv[:, :, :160], want.uv.cpu()), (st.replace, win.frames)
            host = ops.render_replace_yuv(win.labels, s[f0:f1].to("cpu"), pal.cpu(), st.actions(c), mat.cpu(),
                                          back.to("cpu") if isinstance(back, YuvFrames) else back.cpu(), None, 0, st.a256, st.contour, st.replace)
            assert torch.equal(host.y, want.y.cpu()) and torch.equal(host.uv, want.uv.cpu())       # ... and the host path says the same
            differs |= not torch.equal(want.y, s[f0:f1].y[:, :, :160])
        assert differs
        spy.take()                                                    # (the calls made by hand above)
    assert torch.equal(s.y, before[0]) and torch.equal(s.uv, before[1])           # the caller's surfaces are not painted on
    _session(model, s, (5, 3, 7, 2), surface=True)                                # the default style: the plain surface op, as ever
    calls = spy.take()[1]
    assert set(calls) == {"render_overlay_yuv"} and calls["render_overlay_yuv"] >= 3


# ---- the matte as an output ----------------------------------------------------------------------------------------------------------
def _by_hand_matte(windows, rows, spec):
    from mdqe_cvpr2023_amd import ops
    out = []
    for (lg, factor, h, w, Ho, Wo), ((f0, f1), cls) in zip(windows, rows):
        idx = torch.arange(int(lg.shape[0]), dtype=torch.int32, device="cuda")
        take = spec.takes(cls)
        plane = torch.empty((f1 - f0, Ho, Wo), dtype=torch.uint8, device="cuda")
        out.append(ops.final_matte(lg, idx, factor, h, w, Ho, Wo, plane, 0, None if take is None else take.cuda(), spec.gain).cpu())
    return torch.cat(out)


def _forward_matte(model, frames, spec, **attrs):
    saved = model.matte_output
    try:
        model.matte_output = spec
        return _forward(model, frames, **attrs)
    finally:
        model.matte_output = saved


def test_matte_output_offline_on_both_paths_equals_online_and_ops_final_matte(video, logits):
    from mdqe_cvpr2023_amd.render import Matte
    model, frames, base, rows = video
    lm = base[True]["pred_label_map"]
    picked = sorted(set(rows[-1][1].argmax(1)[::2].tolist()))
    for spec in (Matte(), Matte(classes=picked, gain=2.0)):
        want = _by_hand_matte(logits, rows, spec)
        assert int(want.max()) >= 128 and int(want.min()) < 128
        if spec.classes is None:
            assert torch.equal(want >= 128, lm != 0)                  # the union of the tracks' masks, bit for bit
        for early in (True, False):
            got = _forward_matte(model, frames, spec, overlay_output=True, label_output=True, early_masks=early)
            assert set(got) == set(base[early]) | {"pred_matte"}, early
            pm = got["pred_matte"]
            assert pm.dtype == torch.uint8 and tuple(pm.shape) == (L,) + OUT and not pm.is_cuda and torch.equal(pm, want), (spec, early)
            for k in base[early]:                                     # every other output keeps its bits
                assert _same(got[k], base[early][k]), (early, k)
            plain = _forward_matte(model, frames, spec, early_masks=early)        # beside the dense masks alone
            assert torch.equal(plain["pred_matte"], want) and "pred_track_ids" in plain and "pred_masks" in plain
        for emit in ("rle", "overlay", "masks"):
            for sizes in (PLANS[0], PLANS[2]):
                ov, wins, _ = _online(model, frames, sizes, emit=emit, matte=spec, keep=True)
                assert [w.frames for w in wins] == [f for f, _ in rows]
                for w in wins:
                    assert w.matte.dtype == torch.uint8 and w.matte.is_pinned() and torch.equal(w.matte, want[w.frames[0]:w.frames[1]]), (emit, w.frames)
                assert torch.equal(ov.result()["pred_matte"], want)
    again = _forward(model, frames, overlay_output=True, label_output=True)
    assert "pred_matte" not in again and model.matte_output is None
    _, wins, _ = _online(model, frames, [L], emit="rle")
    assert all(w.matte is None for w in wins)


def test_matte_output_refusals(video):
    from mdqe_cvpr2023_amd.render import Matte
    model = video[0]
    with pytest.raises(ValueError, match="render.Matte"):
        model.matte_output = 1.0
    with pytest.raises(ValueError, match="render.Matte"):
        model.online_video(matte=True)
    assert model.matte_output is None
    model.matte_output = Matte(gain=0.5)
    assert model.matte_output == Matte(gain=0.5)
    model.matte_output = None
