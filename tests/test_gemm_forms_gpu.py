"""Every tile, kernel form and epilogue term of the GEMM family against the float64 value of the documented formula
(tests/_gemm_ref.py), element by element: a launch passes only if EVERY element lies within its own fp32 (or split-precision) bound,
and if the launch wrote all of C's [M, N] view and nothing else -- every output is a view of a larger buffer pre-filled with a
sentinel bit pattern.  tests/test_gemm_ref_cpu.py shows on the same cases that the bound admits the formula in float32 and rejects
nine one-off mistakes.

Refused combinations (MDQE_EINVAL; asserted by test_refused_combinations, nothing is skipped silently):

    form                     tile      why
    K-step 32 (variant 0)    4, 5      gemm.hip has no 256-column tile
    any, plain product       6         the LayerNorm tile is mdqe_gemm_ln_f32's (needs gamma / beta)
    any, plain product       10        no such tile code
    convolution, both forms  4, 5      no 256-column convolution tile
    convolution, both forms  6         the LayerNorm tile takes no convolution

Which arithmetic a split-precision launch gets (csrc/gemm_api.hip dispatch_gemm) -- the bound asserted is that arithmetic's:

    mode    tile  planes  eligible for the pre-split kernels    arithmetic
    f16x3   1     yes     yes                                   f16x3 (gemm_f16x3w.hip)
    f16x3   1, 2  any     otherwise                             f16x3 (gemm_f16x3.hip, splits in the kernel)
    f16     1     yes     yes                                   f16   (gemm_f16x3w.hip, one pass)
    f16     1, 2  any     otherwise                             fp32
    any     auto  any     no, at these sizes (64x64 tile)       fp32
"""
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FC12345                   # a quiet NaN with a payload: no kernel computes it
COUNT = {"launches": 0}


@pytest.fixture(autouse=True)
def _restore_switches():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import lib
    try:
        yield
    finally:
        lib.mdqe_debug_gemm_variant(2)
        lib.mdqe_debug_gemm_stages(0)
        lib.mdqe_debug_gemm_fast_epilogue(1)
        lib.mdqe_debug_gemm_rows_dot(1)
        ops.set_gemm_precision("f32")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\ntest_gemm_forms_gpu: {COUNT['launches']} launches compared element by element")


def set_form(form):
    from mdqe_cvpr2023_amd._lib import check, lib
    check(lib.mdqe_debug_gemm_variant({"k32": 0, "auto": 2}.get(form, 1)))
    check(lib.mdqe_debug_gemm_stages({"k16-stages3": 3, "k16-stages4": 4}.get(form, 0)))
    check(lib.mdqe_debug_gemm_fast_epilogue(0 if form == "k16-nofast" else 1))


# ---- canary ---------------------------------------------------------------------------------------------------------------------
def canary(M, N, ld, off=0, tail_rows=130):
    """An [M, N] fp32 view of pitch ld, `256 + off` floats into a sentinel-filled buffer with `tail_rows` more rows behind it."""
    front = 256 + off
    total = front + (M - 1) * ld + N + tail_rows * ld + 64
    buf = torch.full((total,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf.view(torch.float32).as_strided((M, N), (ld, 1), front)


def check_canary(buf, view, what):
    inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    inside.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(True)
    hit = buf == SENT
    outside_ok, inside_ok = torch.stack([hit[~inside].all(), ~hit[inside].any()]).tolist()
    assert outside_ok, f"{what}: wrote outside the [M, N] view"
    assert inside_ok, f"{what}: left elements of the [M, N] view unwritten"


def strided(t, ld=None, off=0):
    """A device copy of the 2-D (or 1-D) CPU tensor t as a view of pitch ld starting `off` floats into its buffer."""
    if t.dim() == 1:
        b = torch.zeros(t.numel() + off + 4, device="cuda")
        v = b[off:off + t.numel()]
    else:
        ld = ld or t.shape[1]
        b = torch.randn(off + t.shape[0] * ld + 8, device="cuda")
        v = b.as_strided(tuple(t.shape), (ld, 1), off)
    v.copy_(t)
    return v


def odd(n):
    return n + 1 if n % 2 == 0 else n + 2


def run_linear(op, kw, tile, what, mode="f32", ldc=None, c_off=0, bias_off=0, res_off=0, ldr=None, lda=None, ksplit=0, weight=None):
    """One launch of mdqe_gemm_nt_f32 into a canary view, compared with the float64 formula element by element."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    A, W = op["A"], op["W"]
    (M, K), N = A.shape, W.shape[0]
    ldc = ldc or N
    Ad = strided(A, lda) if lda else A.cuda()
    Wd = weight if weight is not None else W.cuda()
    bd = strided(kw["bias"], off=bias_off) if kw.get("bias") is not None else None
    rd = strided(kw["residual"], ldr, res_off) if kw.get("residual") is not None else None
    md = kw["rowmask"].cuda() if kw.get("rowmask") is not None else None
    buf, out = canary(M, N, ldc, c_off)
    args = dict(act=kw.get("act"), act_cols=kw.get("act_cols", 0), res_mod=kw.get("res_mod", 0), res_first=bool(kw.get("res_first", False)),
                mask_cols=kw.get("mask_cols", 0))
    if ksplit:
        # (through the C ABI: the workspace is a sentinel-filled buffer of this test's, `ksplit * M * N` floats and a tail behind them)
        ws = torch.full((ksplit * M * N + 4096,), SENT, dtype=torch.int32, device="cuda")
        check(lib.mdqe_gemm_nt_f32(ptr(Ad), Ad.stride(0) if M > 1 else K, ptr(Wd), ptr(bd), ptr(out), ldc, M, N, K, ops.ACT[args["act"]],
                                   args["act_cols"], ptr(rd), rd.stride(0) if rd is not None else 0, args["res_mod"], int(args["res_first"]),
                                   ptr(md.view(torch.uint8)) if md is not None else None, args["mask_cols"], tile, ksplit, ptr(ws),
                                   ptr(ops._wsplit(Wd)), cur_stream()), what)
        assert bool((ws[ksplit * M * N:] == SENT).all()), f"{what}: wrote behind the split-K workspace"
    else:
        ops.linear(Ad, Wd, bd, residual=rd, rowmask=md, out=out, ldc=ldc, tile=tile, **args)
    check_canary(buf, out, what)
    ref = R.gemm_ref64(A, W, prod=op["prod"], **kw)
    R.check_within(out.cpu(), ref, R.gemm_bound(A, W, absprod=op["absprod"], mode=mode, **kw), what)
    COUNT["launches"] += 1


def unaligned_cases(op, N):
    """(name, epilogue, launch kwargs): each operand unaligned on its own on a plain product with a residual (vec_ok == 0: the
    element-by-element epilogue everywhere), then all at once under the full combination."""
    plain = dict(bias=op["bias"], residual=op["res"])
    K = op["A"].shape[1]
    return [("odd ldc", plain, dict(ldc=odd(N))), ("C one float in", plain, dict(c_off=1)), ("bias one float in", plain, dict(bias_off=1)),
            ("residual one float in", plain, dict(res_off=1)), ("odd ldr", plain, dict(ldr=odd(N))), ("lda > K", plain, dict(lda=K + 4)),
            ("lda > K, relu", dict(plain, act="relu"), dict(lda=K + 8, ldc=N + 4, ldr=N + 8)),
            ("all unaligned", R.full_combo(N, op), dict(ldc=odd(N), c_off=1, bias_off=1, res_off=3, ldr=odd(N) + 2, lda=K + 4))]


@pytest.mark.parametrize("form,tile", R.FORMS, ids=[f"{f}-t{t}" for f, t in R.FORMS])
def test_plain_product_forms(form, tile):
    set_form(form)
    for shape, name, kw in R.linear_plan(tile, (form, tile) in R.FULL_FORMS):
        run_linear(R.operands(*shape), kw, tile, f"{form} tile {tile} {shape} {name}")
    bm, bn, _ = R.tile_geometry(tile)
    M, N, K = R.main_shape(bm, bn)
    op = R.operands(M, N, K)
    for name, kw, how in unaligned_cases(op, N):
        run_linear(op, kw, tile, f"{form} tile {tile} {(M, N, K)} {name}", **how)
    for shape, ks, kw in R.splitk_plan(tile):
        run_linear(R.operands(*shape), kw, tile, f"{form} tile {tile} {shape} ksplit={ks}", ksplit=ks)


REFUSED = [("k32", "linear", 4), ("k32", "linear", 5), ("k16", "linear", 6), ("k32", "linear", 6), ("k16", "linear", 10), ("k32", "linear", 10),
           ("k16", "conv", 4), ("k16", "conv", 5), ("k32", "conv", 4), ("k32", "conv", 5), ("k16", "conv", 6), ("k32", "conv", 6)]


@pytest.mark.parametrize("form,kind,tile", REFUSED)
def test_refused_combinations(form, kind, tile):
    """The table in the module docstring: MDQE_EINVAL, and nothing written."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import MdqeError
    set_form(form)
    if kind == "linear":
        op = R.operands(165, 100, 48)
        buf, out = canary(165, 100, 100)
        with pytest.raises(MdqeError, match="code 1"):
            ops.linear(op["A"].cuda(), op["W"].cuda(), op["bias"].cuda(), out=out, ldc=100, tile=tile)
    else:
        c = R.conv_operands(R.CONV_GEOMS[0])
        x, w = c["x"].permute(0, 2, 3, 1).contiguous().cuda(), c["w"].permute(0, 2, 3, 1).contiguous().cuda()
        M, N = c["prod"].shape
        buf, out = canary(M, N, N)
        with pytest.raises(MdqeError, match="code 1"):
            ops.conv2d_nhwc(x, w, c["bias"].cuda(), c["stride"], c["pad"], out=out.view(x.shape[0], c["OH"], c["OW"], N), tile=tile)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())


# ---- N <= 8: the row-dot kernel, and the MFMA tiles with its switch off -------------------------------------------------------
@pytest.mark.parametrize("rows_dot", [1, 0])
def test_few_output_columns(rows_dot):
    from mdqe_cvpr2023_amd._lib import check, lib
    check(lib.mdqe_debug_gemm_rows_dot(rows_dot))
    for what, A, W, kw, extra in R.other_plan():
        if extra["kind"] != "rows_dot":
            continue
        op = dict(A=A, W=W, prod=A.double() @ W.double().t(), absprod=A.double().abs() @ W.double().abs().t())
        run_linear(op, kw, 0, f"{what} switch {rows_dot}", ldc=W.shape[0] + 3)
        if A.shape[0] == 1030:
            run_linear(op, kw, 0, f"{what} switch {rows_dot} lda > K", lda=A.shape[1] + 4)


# ---- convolution ----------------------------------------------------------------------------------------------------------------
def run_conv(c, tile, what, img_pad=0, ldy_extra=0, ksplit=0):
    from mdqe_cvpr2023_amd import ops
    x, w, kw = c["x"], c["w"], c["kw"]
    NI, Cin, H, W_ = x.shape
    Cout = w.shape[0]
    M = NI * c["OH"] * c["OW"]
    img = H * W_ * Cin
    xb = torch.randn(NI, img + img_pad, device="cuda")
    xb[:, :img] = x.permute(0, 2, 3, 1).reshape(NI, img).cuda()
    xd = xb.as_strided((NI, H, W_, Cin), (img + img_pad, W_ * Cin, Cin, 1))
    wd = w.permute(0, 2, 3, 1).contiguous().cuda()
    ldy = Cout + ldy_extra
    buf, out = canary(M, Cout, ldy)
    out4 = out.as_strided((NI, c["OH"], c["OW"], Cout), (c["OH"] * c["OW"] * ldy, c["OW"] * ldy, ldy, 1), out.storage_offset())
    res = kw["residual"].cuda().view(NI, c["OH"], c["OW"], Cout) if kw.get("residual") is not None else None
    ops.conv2d_nhwc(xd, wd, kw["bias"].cuda(), c["stride"], c["pad"], act=kw.get("act"), residual=res, out=out4, tile=tile,
                    res_first=bool(kw.get("res_first", False)), ksplit=ksplit)
    check_canary(buf, out, what)
    R.check_within(out.cpu(), R.gemm_ref64(None, None, prod=c["prod"], **kw), R.gemm_bound(None, None, absprod=c["absprod"], K=c["K"], **kw), what)
    COUNT["launches"] += 1


@pytest.mark.parametrize("form", ["k16", "k32"])
@pytest.mark.parametrize("tile", (0,) + R.CONV_TILES)
def test_convolution_forms(form, tile):
    """Implicit-GEMM convolution against F.conv2d in float64 (Cin < 128: never the Winograd route)."""
    set_form(form)
    for what, c in R.conv_plan():
        run_conv(c, tile, f"{form} tile {tile} {what}", **c["launch"])


# ---- cat2 / pix -------------------------------------------------------------------------------------------------------------------
def test_cat2_and_pix_products():
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    for what, A, W, kw, extra in R.other_plan():
        if extra["kind"] not in ("cat2", "pix"):
            continue
        M, N = A.shape[0], W.shape[0]
        ldc = N + (1 if kw.get("act") else 4)                  # (N + 4 = 264: float4 stores; the others element by element)
        buf, out = canary(M, N, ldc)
        Wd, bd, act = W.cuda(), kw["bias"].cuda(), ops.ACT[kw.get("act")]
        s = extra["stride"]
        if extra["kind"] == "cat2":
            y, x2 = extra["y"].cuda(), extra["x2"].cuda()
            NI, OH, OW, K1 = y.shape
            _, H2, W2, lda2 = x2.shape
            check(lib.mdqe_gemm_nt_cat2_f32(ptr(y), K1, K1, ptr(x2), lda2, extra["K2"], NI, OH, OW, H2, W2, s, ptr(Wd), ptr(bd), ptr(out),
                                            ldc, N, act, cur_stream()), what)
        else:
            x = extra["x"].cuda()
            NI, H, W_, lda = x.shape
            OH, OW = (H - 1) // s + 1, (W_ - 1) // s + 1
            check(lib.mdqe_gemm_nt_pix_f32(ptr(x), lda, extra["K"], NI, H, W_, OH, OW, s, ptr(Wd), ptr(bd), ptr(out), ldc, N, act,
                                           cur_stream()), what)
        check_canary(buf, out, what)
        R.check_within(out.cpu(), R.gemm_ref64(A, W, **kw), R.gemm_bound(A, W, **kw), what)
        COUNT["launches"] += 1


# ---- the rank-4 side term -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["auto", "k32", "f16x3"])
def test_side_term(form):
    """In the K-step-16 kernel's epilogue (default form), and as a pass of its own behind the K-step-32 form and in mode f16x3 (where
    the dispatcher gives these sizes the 64x64 fp32 tile: the fp32 bound)."""
    from mdqe_cvpr2023_amd import ops
    if form == "f16x3":
        ops.set_gemm_precision("f16x3")
    else:
        set_form(form)
    for what, A, W, kw, extra in R.other_plan():
        if extra["kind"] != "side":
            continue
        M, N = A.shape[0], W.shape[0]
        buf, out = canary(M, N, N + 4)
        ops.linear_side(A.cuda(), W.cuda(), kw["bias"].cuda(), kw["side"].cuda(), kw["side_w"].cuda(), kw["side_cols"], out=out)
        check_canary(buf, out, f"{form} {what}")
        R.check_within(out.cpu(), R.gemm_ref64(A, W, **kw), R.gemm_bound(A, W, **kw), f"{form} {what}")
        COUNT["launches"] += 1


# ---- Linear + LayerNorm in one kernel ---------------------------------------------------------------------------------------
def test_linear_layernorm_entry_points():
    """mdqe_gemm_ln_f32 / mdqe_gemm_ln2_f32 through the C ABI (below ops.LINEAR_LN_MIN_ROWS ops.linear_ln would take two kernels),
    C aliasing the residual and not; float64 LayerNorm of the float64 product; the GEMM bound propagated as _gemm_ref.ln_bound says."""
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    eps = 1e-5
    for what, A, W, kw, extra in R.other_plan():
        if extra["kind"] != "ln":
            continue
        M, K = A.shape
        g1, b1, g2, b2 = extra["ln"]
        x64 = R.gemm_ref64(A, W, **kw)
        ref1, bd1 = R.ln_ref64(x64, g1, b1, eps), R.ln_bound(x64, R.gemm_bound(A, W, **kw), g1, b1, eps)
        ref2, bd2 = R.ln_ref64(ref1, g2, b2, eps), R.ln_bound(ref1, bd1, g2, b2, eps)
        Ad, Wd, bd = A.cuda(), W.cuda(), kw["bias"].cuda()
        dev = [t.cuda() for t in (g1, b1, g2, b2)]
        for alias in (True, False):
            for second in (False, True):
                w_ = f"{what} alias={alias} second={second}"
                buf, out = canary(M, 256, 256 if alias else 260)
                if alias:
                    out.copy_(kw["residual"])
                    rd = out
                else:
                    rd = strided(kw["residual"], 264)
                if second:
                    buf2, out2 = canary(M, 256, 268)
                    check(lib.mdqe_gemm_ln2_f32(ptr(Ad), K, ptr(Wd), ptr(bd), ptr(out), out.stride(0), M, 256, K, ptr(rd), rd.stride(0), ptr(dev[0]),
                                                ptr(dev[1]), ptr(dev[2]), ptr(dev[3]), ptr(out2), 268, eps, cur_stream()), w_)
                    check_canary(buf2, out2, w_ + " C2")
                    R.check_within(out2.cpu(), ref2, bd2, w_ + " C2")
                else:
                    check(lib.mdqe_gemm_ln_f32(ptr(Ad), K, ptr(Wd), ptr(bd), ptr(out), out.stride(0), M, 256, K, ptr(rd), rd.stride(0), ptr(dev[0]),
                                               ptr(dev[1]), eps, cur_stream()), w_)
                check_canary(buf, out, w_)
                R.check_within(out.cpu(), ref1, bd1, w_)
                COUNT["launches"] += 1


# ---- split precision ----------------------------------------------------------------------------------------------------------------
def _arith(mode, tile, planes, eligible):
    """The table in the module docstring."""
    if tile == 0:
        return "f32"
    if mode == "f16x3":
        return "f16x3"
    return "f16" if (tile == 1 and planes and eligible) else "f32"


def _weight(op, planes):
    from mdqe_cvpr2023_amd import ops
    Wd = op["W"].cuda()
    if planes:
        ops.const_weight(Wd)
    K = op["W"].shape[1]
    assert (ops._wsplit(Wd) is not None) == (planes and Wd.shape[0] >= 128 and K % 32 == 0)
    return Wd


@pytest.mark.parametrize("mode", ["f16x3", "f16"])
@pytest.mark.parametrize("planes", [True, False], ids=["planes", "noplanes"])
def test_split_precision_tiles(mode, planes):
    from mdqe_cvpr2023_amd import ops
    ops.set_gemm_precision(mode)
    for M, N, K in R.SPLIT_SHAPES:
        op = R.split_operands(M, N, K)
        Wd = _weight(op, planes)
        for tile in (1, 2):
            for name, kw in (("none", {}), ("all", R.full_combo(N, op))):
                run_linear(op, kw, tile, f"{mode} planes={planes} tile {tile} {(M, N, K)} {name}", mode=_arith(mode, tile, planes, True), weight=Wd)


@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_split_precision_256_column_tile(mode):
    """Row counts at which the dispatcher gives the pre-split kernel its 128 x 256 tile (201 and 401 row blocks)."""
    from mdqe_cvpr2023_amd import ops
    ops.set_gemm_precision(mode)
    M, N, K = R.SPLIT_BIG[mode]
    op = R.split_operands(M, N, K)
    Wd = _weight(op, True)
    for name, kw in (("none", {}), ("all", R.full_combo(N, op))):
        run_linear(op, kw, 1, f"{mode} {(M, N, K)} {name}", mode=mode, weight=Wd)


@pytest.mark.parametrize("mode", ["f16x3", "f16"])
def test_split_precision_products_the_presplit_kernels_cannot_take(mode):
    """Ragged K, N < 128, an unaligned C, split-K, each with planes where const_weight grants them: the auto tile stays on the fp32
    kernels in both modes, tile 1 in mode f16 too; tile 1 in mode f16x3 takes the kernel that splits its operands itself."""
    from mdqe_cvpr2023_amd import ops
    ops.set_gemm_precision(mode)
    for name, (M, N, K), how in R.SPLIT_INELIGIBLE:
        op = R.split_operands(M, N, K)
        Wd = _weight(op, True)
        for tile in (0, 1):
            for ename, kw in (("none", {}), ("all", R.full_combo(N, op))):
                run_linear(op, kw, tile, f"{mode} {name} tile {tile} {ename}", mode=_arith(mode, tile, True, False), weight=Wd, **how)


# ---- the activations' own error ---------------------------------------------------------------------------------------------------
def test_activation_error_of_the_device_functions():
    """What _gemm_ref.SIG_A / TANH_A rest on: a K = 4 product with an exact pre-activation value (A rows carry the grid, W rows are
    unit vectors) against the float64 function of the same fp32 argument.  The constants are 4 x the measured maximum."""
    from mdqe_cvpr2023_amd import ops
    x = torch.linspace(-20.0, 20.0, 1 << 18, dtype=torch.float64).float().view(-1, 4)
    A, W = x.cuda(), torch.eye(4).cuda()
    assert torch.equal(ops.linear(A, W, None, tile=3).cpu(), x)                 # the pre-activation value is exact
    worst = {}
    for act in ("sigmoid", "tanh", "gelu"):
        worst[act] = 0.0
        for tile in (3, 1):
            out = ops.linear(A, W, None, act=act, tile=tile).cpu().double()
            worst[act] = max(worst[act], float((out - R.act64(x.double(), act)).abs().max()))
        print(f"\nmeasured max |{act} - float64| over [-20, 20]: {worst[act]:.4e}")
    assert 4 * worst["sigmoid"] <= R.SIG_A, worst
    assert 4 * worst["tanh"] <= R.TANH_A, worst
    assert worst["gelu"] <= R.GELU_A, worst
