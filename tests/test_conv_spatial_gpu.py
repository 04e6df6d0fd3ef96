"""The convolution and spatial kernels of the per-frame path (csrc/winograd.hip, stem_conv.hip, dwconv.hip and the small kernels of
spatial.hip) against float64 (tests/_conv_spatial_ref.py), element by element, through the C entry points: a launch passes only if
EVERY element lies within its own derived bound (the exact kernels: equal bits) and if it wrote all of its output view and nothing
else -- every output is a view of a larger buffer pre-filled with a sentinel bit pattern, with guard bands before and behind it and
in the padding columns of a pitched output (the scheme of tests/test_gemm_forms_gpu.py).  The cases are the smallest that reach
every loop count of the capped grids, ragged and exact tiles, both sides of every store guard, and every plane-batch tile of the
K-step-16 GEMM.  tests/test_conv_spatial_ref_cpu.py shows on the same cases that the bounds admit the formulas in float32 and reject
the seeded mistakes.  The achieved err / bound of every kernel group goes to the parity-margin table (_golden.record_margin)."""
import ctypes

import pytest
import torch

import _conv_spatial_ref as R
from _golden import record_margin
from test_attn_norm_gpu import canary_nd, dense, rows_view
from test_gemm_forms_gpu import SENT, check_canary

pytestmark = pytest.mark.gpu

WORST, COUNT = {}, {}


@pytest.fixture(autouse=True)
def _restore_switches():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import lib
    fast = ops.DW_FAST
    try:
        yield
    finally:
        lib.mdqe_debug_winograd_tile(0)
        ops.DW_FAST = fast


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\ntest_conv_spatial_gpu: {sum(COUNT.values())} launches compared element by element")
    for group in sorted(COUNT):
        print(f"    {COUNT[group]:4d}  {group}: worst err / bound {WORST[group]:.3f}")


def compare(group, stage, out, ref, bound, what):
    """Record the achieved err / bound of the worst element, then hold every element to its bound (None: equal bits)."""
    out = out.cpu().reshape(ref.shape)
    if bound is None:
        assert torch.equal(out, ref), f"{what}: {int((out != ref).sum())} of {ref.numel()} elements differ from the exact result"
        ratio = 0.0
    else:
        ratio, err, b = R.worst_ratio(out, ref, bound)
        record_margin("conv_spatial " + group, stage, err, scale=b, tol=1.0)
        R.check_within(out, ref, bound, what)
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    COUNT[group] = COUNT.get(group, 0) + 1


def nhwc_view(NI, H, W, C, ld=None):
    ld = ld or C
    return canary_nd((NI, H, W, C), (H * W * ld, W * ld, ld, 1))


def strided_images(t, extra):
    """A device copy of t [NI, ...] whose images lie numel / NI + extra elements apart (random values between them)."""
    NI, n = t.shape[0], t[0].numel()
    b = torch.randint(0, 200, (NI, n + extra), device="cuda").to(t.dtype)
    b[:, :n] = t.reshape(NI, n).cuda()
    return b, n + extra


# ---- Winograd ---------------------------------------------------------------------------------------------------------------------
def wino_u(w):
    """U of the weight through mdqe_winograd_weight_f32, into a guarded buffer."""
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    Cout, _, _, Cin = w.shape
    wd = w.cuda().contiguous()
    buf, Uv = dense((16, Cout, Cin))
    check(lib.mdqe_winograd_weight_f32(ptr(wd), Cout, Cin, ptr(Uv), cur_stream()), "winograd_weight")
    check_canary(buf, Uv, f"winograd_weight {Cout} x {Cin}")
    return Uv


def run_wino(geom, what, Uv=None):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    NI, H, W, Cin, Cout, act, bias, ldx, xpad = geom
    c = R.wino_case(geom)
    xb, xs = strided_images(c["x"], xpad)
    Uv = Uv if Uv is not None else wino_u(c["w"])
    bd = c["b"].cuda() if bias else None
    buf, out = nhwc_view(NI, H, W, Cout, Cout + ldx)
    nb = lib.mdqe_winograd_workspace_bytes(NI, H, W, Cin, Cout)
    assert nb % 4 == 0
    ws = torch.full((nb // 4 + 4096,), SENT, dtype=torch.int32, device="cuda")
    check(lib.mdqe_conv3x3_winograd_f32(ptr(xb), xs if xpad else 0, ptr(Uv), ptr(bd), ptr(out), Cout + ldx, NI, H, W, Cin, Cout, ops.ACT[act],
                                        ptr(ws), nb, cur_stream()), what)
    check_canary(buf, out, what)
    assert bool((ws[nb // 4:] == SENT).all()), f"{what}: wrote behind the workspace"
    return out, c


@pytest.mark.parametrize("geom", R.WINO_CASES, ids=str)
def test_winograd_entry_point(geom):
    what = f"conv3x3_winograd {geom}"
    out, c = run_wino(geom, what)
    g = R.wino_geometry(geom)
    stage = "one image over the group budget" if g["per_img"] > R.GROUP_BYTES else f"T={'<32' if g['T'] < 32 else '>=32'} act={geom[5]}"
    compare("winograd", stage, out, c["ref"], c["bound"], what)


@pytest.mark.parametrize("Cout,Cin", R.WINO_WEIGHTS)
def test_winograd_weight_is_rounded_once_from_double(Cout, Cin):
    w = torch.randn(Cout, 3, 3, Cin, generator=R._gen(Cout, Cin))
    u64 = R.wino_weight64(w)
    compare("winograd weight", f"{Cout} x {Cin}", wino_u(w), u64, R.U * u64.abs(), f"winograd_weight {Cout} x {Cin}")


def test_winograd_bits_do_not_depend_on_the_plane_product_tile():
    """csrc/winograd.hip: every K-step-16 tile accumulates an element over K in the same order.  T = 216 rows and N = 260 columns are
    ragged against every tile's rows and columns."""
    from mdqe_cvpr2023_amd._lib import check, lib
    geom = R.WINO_RAGGED
    Uv = wino_u(R.wino_case(geom)["w"])
    try:
        base, c = run_wino(geom, "winograd default tile", Uv)
        compare("winograd", "tile default", base, c["ref"], c["bound"], "winograd default tile")
        for tile in R.WINO_TILES:
            check(lib.mdqe_debug_winograd_tile(tile))
            out, _ = run_wino(geom, f"winograd tile {tile}", Uv)
            assert torch.equal(out, base), f"plane-product tile {tile}: {int((out != base).sum())} of {base.numel()} elements differ from the default tile's"
            COUNT["winograd"] += 1
    finally:
        lib.mdqe_debug_winograd_tile(0)


def test_winograd_refusals():
    """Each is refused with an error code before anything is launched; the output and the workspace stay untouched.  Every buffer is
    large enough for the call it is handed, so a missing check would show as a written buffer, not as a stray store."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import cur_stream, lib, ptr
    NI, H, W = 3, 2, 3
    x = torch.randn(NI * H * W * 64 + 64, device="cuda")
    Ud = torch.randn(16 * 1028 * 64 + 64, device="cuda")
    bias = torch.randn(1028 + 64, device="cuda")
    out = torch.full((NI * H * W * 1100 + 64,), SENT, dtype=torch.int32, device="cuda")
    ws = torch.full((1 << 20,), SENT, dtype=torch.int32, device="cuda")

    def call(Cin=32, Cout=36, ldy=None, xo=0, uo=0, yo=0, bo=0, wo=0, short=0):
        nb = lib.mdqe_winograd_workspace_bytes(NI, H, W, Cin, Cout)
        assert 0 < nb <= ws.numel() * 4 - 64
        return lib.mdqe_conv3x3_winograd_f32(ptr(x) + xo, 0, ptr(Ud) + uo, ptr(bias) + bo, ptr(out) + yo, ldy or Cout, NI, H, W, Cin, Cout, 1,
                                             ptr(ws) + wo, nb - short, cur_stream())

    refused = {"Cin % 32 != 0": lambda: call(Cin=48), "Cout % 4 != 0": lambda: call(Cout=38, ldy=40), "Cout > 1024": lambda: call(Cout=1028),
               "ldy % 4 != 0": lambda: call(ldy=38), "ldy < Cout": lambda: call(ldy=32),
               "X off a 16-byte boundary": lambda: call(xo=4), "U off a 16-byte boundary": lambda: call(uo=8),
               "Y off a 16-byte boundary": lambda: call(yo=4), "bias off a 16-byte boundary": lambda: call(bo=4),
               "workspace off a 16-byte boundary": lambda: call(wo=4), "a workspace one byte short": lambda: call(short=1)}
    for what, f in refused.items():
        assert f() != 0, f"{what}: accepted"
        print(f"\nrefused: {what}")
    for mode in ("f16x3", "f16"):
        with ops.gemm_precision(mode):
            assert call() != 0, f"precision mode {mode}: accepted"
        print(f"\nrefused: precision mode {mode}")
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((ws == SENT).all())
    assert call() == 0                                                  # (the same arguments, unaltered, are accepted)
    torch.cuda.synchronize()
    assert not bool((out[:NI * H * W * 36] == SENT).any())


# ---- stem -------------------------------------------------------------------------------------------------------------------------
def _mean_std():
    return (ctypes.c_float * 3)(*R.MEAN), (ctypes.c_float * 3)(*R.STD)


@pytest.mark.parametrize("geom", R.STEM_CASES, ids=str)
def test_stem_conv(geom):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    NI, h, w, Hp, Wp, u8, spad = geom
    what = f"stem_conv {geom}"
    c = R.stem_case(geom)
    fb, fs = strided_images(c["frames"], spad)
    wk, bd = ops.stem_weight_kmajor(c["w"]).cuda(), c["b"].cuda()
    buf, out = nhwc_view(NI, Hp // 2, Wp // 2, 64)
    m, s = _mean_std()
    check(lib.mdqe_stem_conv_f32(ptr(fb), int(u8), fs, NI, h, w, Hp, Wp, m, s, ptr(wk), ptr(bd), ptr(out), cur_stream()), what)
    check_canary(buf, out, what)
    loops = R.stem_geometry(geom)["loops"]
    compare("stem_conv", f"{'uint8' if u8 else 'float32'} tiles per block {sorted(loops)}", out, c["ref"], c["bound"], what)


@pytest.mark.parametrize("geom", R.IM2COL_CASES, ids=str)
def test_stem_im2col(geom):
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    NI, h, w, Hp, Wp, u8, spad = geom
    what = f"stem_im2col {geom}"
    f = R.stem_frames(NI, h, w, u8)
    ref = R.im2col_ref(f, Hp, Wp)
    fb, fs = strided_images(f, spad)
    buf, out = rows_view(ref.shape[0], 160, 160)
    m, s = _mean_std()
    check(lib.mdqe_stem_im2col_f32(ptr(fb), int(u8), fs, NI, h, w, Hp, Wp, m, s, ptr(out), cur_stream()), what)
    check_canary(buf, out, what)
    compare("stem_im2col", "uint8" if u8 else "float32", out, ref, 2 * R.U * ref.abs(), what)


# ---- depthwise 5x5 ------------------------------------------------------------------------------------------------------------------
def run_dw(geom, what, case=None):
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    kernel, NI, H, W, C, up2 = geom
    c = case or R.dw_case(geom)
    x, wt, bias = c["x"].cuda(), c["wt"].cuda(), c["bias"].cuda()
    tw, tb = (c["tw"].cuda(), c["tb"].cuda()) if up2 else (None, None)
    OH, OW = (2 * H, 2 * W) if up2 else (H, W)
    buf, out = nhwc_view(NI, OH, OW, C)
    if kernel == "c256":
        check(lib.mdqe_dwconv5x5_c256_f32(ptr(x), ptr(wt), ptr(bias), ptr(out), NI, H, W, cur_stream()), what)
    elif kernel == "quad":
        check(lib.mdqe_dwconv5x5_up2_c256_f32(ptr(x), ptr(wt), ptr(bias), ptr(tw), ptr(tb), ptr(out), NI, H, W, cur_stream()), what)
    else:
        check(lib.mdqe_dwconv5x5_nhwc_f32(ptr(x), ptr(wt), ptr(bias), ptr(out), NI, OH, OW, C, int(up2), ptr(tw), ptr(tb), cur_stream()), what)
    check_canary(buf, out, what)
    return out, c


@pytest.mark.parametrize("geom", R.DW_CASES, ids=str)
def test_depthwise_kernels(geom):
    what = f"dwconv5x5 {geom}"
    out, c = run_dw(geom, what)
    compare(f"depthwise {geom[0]}", f"{'up2' if geom[5] else 'plain'} loops {sorted(R.dw_geometry(geom)['loops'])}", out, c["ref"], c["bound"], what)


@pytest.mark.parametrize("geom", [g for g in R.DW_CASES if g[0] == "quad" and g[2] * g[3] < 1000], ids=str)
def test_depthwise_generic_kernel_at_256_channels_meets_the_quad_cases(geom):
    """The two kernels of ConvTranspose x2 -> depthwise 5x5 on the same inputs, each against float64 (not against each other)."""
    what = f"dwconv5x5 generic on {geom}"
    c = R.dw_case(geom)
    out, _ = run_dw(("generic",) + tuple(geom[1:]), what, case=c)
    compare("depthwise generic", "up2 C=256", out, c["ref"], c["bound"], what)


# ---- max pool, upsample-add ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", R.POOL_CASES, ids=str)
def test_maxpool_is_exact(geom):
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    NI, H, W, C, _ = geom
    what = f"maxpool3x3s2 {geom}"
    c = R.pool_case(geom)
    x = c["x"].cuda()
    buf, out = nhwc_view(NI, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)
    check(lib.mdqe_maxpool3x3s2_nhwc_f32(ptr(x), ptr(out), NI, H, W, C, cur_stream()), what)
    check_canary(buf, out, what)
    compare("maxpool", "exact", out, c["ref"], None, what)


@pytest.mark.parametrize("geom", R.UP_CASES, ids=str)
def test_upsample_add_is_exact_out_of_place_and_in_place(geom):
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    NI, H, W, Hb, Wb, C = geom
    c = R.up_case(geom)
    a, b = c["a"].cuda(), c["b"].cuda()
    results = []
    for in_place in (False, True):
        what = f"upsample_nearest_add {geom} in place={in_place}"
        buf, out = nhwc_view(NI, H, W, C)
        if in_place:
            out.copy_(a)
        check(lib.mdqe_upsample_nearest_add_nhwc_f32(ptr(out if in_place else a), ptr(b), ptr(out), NI, H, W, Hb, Wb, C, cur_stream()), what)
        check_canary(buf, out, what)
        compare("upsample_add", "in place" if in_place else "out of place", out, c["ref"], None, what)
        results.append(out.clone())
    assert torch.equal(results[0], results[1])                          # the aliased launch, bit for bit


# ---- routing through ops ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fast", [True, False], ids=["DW_FAST", "generic"])
def test_ops_dwconv5x5_routes_both_ways_within_the_float64_bound(fast):
    from mdqe_cvpr2023_amd import ops
    ops.DW_FAST = fast
    for geom in (("c256", 2, 5, 8, 256, False), ("quad", 2, 5, 8, 256, True)):
        c = R.dw_case(geom)
        tw, tb = (c["tw"].cuda(), c["tb"].cuda()) if geom[5] else (None, None)
        out = ops.dwconv5x5(c["x"].cuda(), c["wt"].cuda(), c["bias"].cuda(), up2=geom[5], tw=tw, tb=tb)
        compare("ops.dwconv5x5", f"DW_FAST={fast} up2={geom[5]}", out, c["ref"], c["bound"], f"ops.dwconv5x5 {geom} DW_FAST={fast}")


def test_ops_conv2d_nhwc_with_a_registered_weight_within_the_float64_bound():
    from mdqe_cvpr2023_amd import ops
    geom = (2, 5, 7, 128, 36, "relu", True, 0, 0)
    c = R.wino_case(geom)
    wr = ops.winograd_weight(c["w"].cuda().contiguous())
    assert ops._wino_u(wr) is not None
    out = ops.conv2d_nhwc(c["x"].cuda(), wr, c["b"].cuda(), 1, 1, act="relu")
    compare("ops.conv2d_nhwc", "registered weight", out, c["ref"], c["bound"], f"ops.conv2d_nhwc {geom}")
    direct = ops.conv2d_nhwc(c["x"].cuda(), c["w"].cuda().contiguous(), c["b"].cuda(), 1, 1, act="relu")
    assert not torch.equal(out, direct)                                 # (the registered weight took the other arithmetic)
