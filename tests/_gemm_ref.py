"""A float64 reference of the GEMM family's documented formula and a per-element error bound (a helper, not a conftest).

The value (`gemm_ref64`) is include/mdqe_hip.h's formula, written from its prose:

    C[m, n] = mask( act(sum_k A[m, k] W[n, k] + bias[n] + side[m, :] . side_w[n, :] (n < side_cols)) + residual[m % res_mod or m, n] )

with the residual added BEFORE the activation when `res_first`, the activation on the columns below `act_cols` (<= 0: all),
and the row mask zeroing the columns below `mask_cols` of the masked rows, last.

The bound (`gemm_bound`) holds for fp32 arithmetic that sums the K products in ANY order:

    |C - ref| <= (K + 8) * 2^-24 * S[m, n] * L_act + a_act,        S = |A| @ |W|^T + |bias| + |side term| + |residual|

Every one of the K products and the at most K - 1 + 4 additions behind it (bias, side term, residual, the rounding of the output
and of the activation's argument) is rounded to fp32 with relative error 2^-24, and a term of the sum passes through at most
K + 8 of those roundings, so the pre-activation value is off by at most (K + 8) 2^-24 S to first order.  The activation scales
that by its Lipschitz constant L_act (1 for none, ReLU and tanh, 1.13 for erf-GELU, 0.25 for the sigmoid) and adds its own
absolute error a_act:

    none, ReLU   0
    GELU         3.4e-7   (csrc/common.h: mdqe_gelu against the exact function over [-12, 12])
    sigmoid      4 x the device function's measured maximum error   (1 / (1 + __expf(-x)))
    tanh         4 x the device function's measured maximum error   (tanhf)

The sigmoid and tanh figures are MEASURED (tests/test_gemm_forms_gpu.py::test_activation_error_of_the_device_functions repeats
the measurement in every run): a K = 4 product whose A rows carry a grid of 262 144 points over [-20, 20] and whose W rows are unit
vectors has an exact pre-activation value, so the output's distance from the float64 function of the same fp32 argument is the
device function's error plus one output rounding.  Measured on an MI355X: sigmoid 9.144e-08, tanh 7.191e-08 (and GELU 3.301e-07, inside its documented 3.4e-7); the
constants are 4 x that, rounded up (3.7e-07 and 2.9e-07): the factor covers what the grid does not sample and the rounding of the
output.  Columns without the activation take L = 1, a = 0; a masked element must be exactly 0 (bound 0).

Split-precision modes (`mode`), per unit of |A| @ |W|^T (P below), for operands of magnitude in [1/16, 4] (`split_operand`: the scaled
low plane then stays a normal f16 number):

    "f16x3"   3 * 2^-20 + (K + 8) * 2^-24
              hi = f16_rtz(x) keeps 11 significant bits (|x - hi| < 2^-10 |x|); lo = f16_rtz((x - hi) * 2048) keeps 11 bits of that
              remainder, so |x - hi - lo / 2048| < 2^-20 |x| per operand: two operands, 2 * 2^-20.  The kernels drop the lo * lo
              product, at most 2^-10 * 2^-10 = 2^-20 of |a| |w|.  Every f16 x f16 product is exact in fp32; the accumulation is fp32.
    "f16"     2^-10 + 2^-22 + (K + 8) * 2^-24
              both operands rounded to nearest f16 (relative 2^-11 each): (1 + 2^-11)^2 - 1 = 2^-10 + 2^-22; fp32 accumulation.

The bias / side / residual part of S keeps the fp32 factor in every mode.  The comparison (`check_within`) passes only if EVERY
element lies within its own bound: no aggregate norm, no element left out.

The LayerNorm entry points (`ln_ref64`, `ln_bound`): y = (x - mean) / sqrt(var + eps) * gamma + beta over a row of N values.  With
d = max_n |dx[n]| the row's largest pre-norm error (the GEMM bound above with the residual in S) and r = 1 / sqrt(var + eps):
the mean moves by at most d, every centred value by at most 2 d, sqrt(var) by at most 2 d (it is 1-Lipschitz in the centred
vector's RMS), so the normalised value xh = (x - mean) r moves by at most 2 d r + |xh| * 2 d r = 2 d r (1 + |xh|) to first order.
The kernel's own fp32 statistics and affine map: the mean of N values in fp32, in any order, is off by at most N 2^-24 mean|x|,
which is N 2^-24 m1 in units of the standard deviation (m1 = mean|x| r); the centred sum of squares, the rsqrt and the products
add at most (N + 16) 2^-24 relative to xh and to that shift.  Together at most (N + 16) * 2^-24 * (1 + m1) * (1 + |xh|).  So

    |y - ref| <= |gamma| * (2 d r * 1.01 + (N + 16) * 2^-24 * (1 + m1)) * (1 + |xh|) + 2^-23 * (|gamma xh| + |beta|)

(the factor 1.01 stands for the second-order terms: d r is below 1e-3 at the test's magnitudes).  A second LayerNorm of the
result propagates the first one's bound in the same way.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24                      # fp32 unit roundoff

SIG_MEAS, TANH_MEAS = 9.144e-8, 7.191e-8      # measured on an MI355X (see the docstring)
SIG_A, TANH_A = 3.7e-7, 2.9e-7            # = 4 x measured, rounded up
GELU_A = 3.4e-7

ACT_L = {None: 1.0, "none": 1.0, "relu": 1.0, "gelu": 1.13, "sigmoid": 0.25, "tanh": 1.0}
ACT_A = {None: 0.0, "none": 0.0, "relu": 0.0, "gelu": GELU_A, "sigmoid": SIG_A, "tanh": TANH_A}

MODE_UNIT = {                       # error per unit of |A| @ |W|^T, without the (K + 8) * 2^-24 accumulation term
    "f32": 0.0,
    "f16x3": 3 * 2.0 ** -20,
    "f16": 2.0 ** -10 + 2.0 ** -22,
}


def act64(x, act):
    """The activation in float64 (erf-GELU, as nn.GELU's default)."""
    if act in (None, "none"):
        return x
    if act == "relu":
        return x.clamp_min(0.0)
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-x))
    if act == "tanh":
        return torch.tanh(x)
    raise ValueError(act)


def _res_rows(M, res_mod):
    m = torch.arange(M)
    return m % res_mod if res_mod > 0 else m


def _epilogue(y, dt, bias, act, act_cols, residual, res_mod, res_first, rowmask, mask_cols, side, side_w, side_cols):
    """The formula on a pre-activation product y [M, N] in dtype dt (float64: the reference; float32: its CPU restatement)."""
    M, N = y.shape
    y = y.clone()
    if bias is not None:
        y += bias.to(dt)
    if side is not None and side_cols > 0:
        y[:, :side_cols] += side.to(dt) @ side_w.to(dt)[:side_cols].t()
    r = residual.to(dt)[_res_rows(M, res_mod)] if residual is not None else None
    if r is not None and res_first:
        y += r
    if act not in (None, "none"):
        c = N if act_cols <= 0 else min(act_cols, N)
        y[:, :c] = act64(y[:, :c], act)
    if r is not None and not res_first:
        y += r
    if rowmask is not None and mask_cols > 0:
        rows = rowmask.bool()
        c = min(mask_cols, N)
        y[rows, :c] = 0.0
    return y


def gemm_ref64(A, W, bias=None, act=None, act_cols=0, residual=None, res_mod=0, res_first=False, rowmask=None, mask_cols=0,
               side=None, side_w=None, side_cols=0, prod=None):
    """float64 value of the documented formula.  A [M, K], W [N, K]; `prod`: A.double() @ W.double().t() where the caller has it."""
    y = prod if prod is not None else A.double() @ W.double().t()
    return _epilogue(y, torch.float64, bias, act, act_cols, residual, res_mod, res_first, rowmask, mask_cols, side, side_w, side_cols)


def gemm_eval32(A, W, **kw):
    """The same formula evaluated in float32 on the CPU (what the bound must always admit)."""
    return _epilogue(A.float() @ W.float().t(), torch.float32, **{**dict(bias=None, act=None, act_cols=0, residual=None, res_mod=0,
                     res_first=False, rowmask=None, mask_cols=0, side=None, side_w=None, side_cols=0), **kw})


def gemm_bound(A, W, bias=None, act=None, act_cols=0, residual=None, res_mod=0, res_first=False, rowmask=None, mask_cols=0,
               side=None, side_w=None, side_cols=0, mode="f32", absprod=None, K=None):
    """Per-element bound [M, N] (float64) of fp32 accumulation in any order; see the module docstring.  `absprod`:
    |A| @ |W|^T in float64 where the caller has it (a convolution passes F.conv2d(|x|, |w|) and its K)."""
    P = absprod if absprod is not None else A.double().abs() @ W.double().abs().t()
    M, N = P.shape
    K = K if K is not None else A.shape[1]
    S = P.clone()
    if bias is not None:
        S += bias.double().abs()
    if side is not None and side_cols > 0:
        S[:, :side_cols] += side.double().abs() @ side_w.double().abs()[:side_cols].t()
    if residual is not None:
        S += residual.double().abs()[_res_rows(M, res_mod)]
    L = torch.ones(N, dtype=torch.float64)
    a = torch.zeros(N, dtype=torch.float64)
    if act not in (None, "none"):
        c = N if act_cols <= 0 else min(act_cols, N)
        L[:c] = ACT_L[act]
        a[:c] = ACT_A[act]
    b = ((K + 8) * U * S + MODE_UNIT[mode] * P) * L + a
    if rowmask is not None and mask_cols > 0:
        b[rowmask.bool(), :min(mask_cols, N)] = 0.0           # a masked element is exactly zero
    return b


def check_within(out, ref, bound, what=""):
    """Every element within its own bound; the message names the worst one."""
    out = out.double()
    assert out.shape == ref.shape == bound.shape, (what, out.shape, ref.shape, bound.shape)
    err = (out - ref).abs()
    bad = ~(err <= bound)                                     # (a NaN is bad)
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements outside their bound; worst at {idx}: "
                             f"got {float(out[idx])!r}, want {float(ref[idx])!r}, |err| {float(err[idx]):.3e} > bound {float(bound[idx]):.3e}")


def within(out, ref, bound):
    return bool(((out.double() - ref).abs() <= bound).all())


def split_operand(shape, g):
    """Operands for the split-precision modes: magnitude uniform in [1/16, 4], random sign."""
    mag = torch.rand(shape, generator=g) * (4.0 - 1.0 / 16) + 1.0 / 16
    sgn = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return mag * sgn


# ---- LayerNorm of a product ---------------------------------------------------------------------------------------------------
def ln_ref64(x64, gamma, beta, eps):
    return F.layer_norm(x64, (x64.shape[-1],), gamma.double(), beta.double(), eps)


def ln_bound(x64, dx, gamma, beta, eps):
    """Bound of LayerNorm(x) * gamma + beta computed in fp32 from an input that is off by at most dx [M, N] (module docstring)."""
    N = x64.shape[-1]
    mean = x64.mean(-1, keepdim=True)
    var = x64.var(-1, unbiased=False, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xh = (x64 - mean) * r
    d = dx.max(dim=-1, keepdim=True).values
    g = gamma.double().abs()
    m1 = x64.abs().mean(-1, keepdim=True) * r
    return g * (2 * d * r * 1.01 + (N + 16) * U * (1 + m1)) * (1 + xh.abs()) + 2 * U * ((gamma.double() * xh).abs() + beta.double().abs())


# ---- the planned cases: shared by the CPU test (float32 restatement inside the bound, mutants outside) and the GPU test --------
TILE_DIMS = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (64, 256), 5: (128, 256), 7: (32, 64), 8: (32, 128), 9: (64, 128)}
TILE_WM = {1: 2, 2: 2, 3: 2, 4: 1, 5: 2, 7: 1, 8: 1, 9: 2}        # waves along M (csrc/gemm_k16.hip mdqe_launch_gemm_k16)
KS = (4, 20, 48, 272)               # below one K-step; ragged for both steps; ragged for 32 only; 17 steps of 16


def shapes_for(bm, bn):
    """Pairwise cover of M in {1, BM, 2 BM + 37} x N in {BN, BN + 36, BN + 33} x K in KS: 12 shapes; every (M, N), (M, K), (N, K)
    pair occurs.  MAIN (below) is among them."""
    Ms, Ns = (1, bm, 2 * bm + 37), (bn, bn + 36, bn + 33)
    return [(Ms[i], Ns[(i + k) % 3], KS[k]) for k in range(4) for i in range(3)]


def main_shape(bm, bn):
    return (2 * bm + 37, bn + 36, 48)


_cache = {}


def operands(M, N, K, seed=0):
    """The inputs of one shape, with the float64 product and |A| @ |W|^T computed once (callers must not modify them).
    The residual and bias are of the product's own magnitude (about 1), so a wrong row or column shows."""
    key = (M, N, K, seed)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + 7919 * seed)
        A = torch.randn(M, K, generator=g)
        W = torch.randn(N, K, generator=g) / K ** 0.5
        d = dict(A=A, W=W, bias=torch.randn(N, generator=g), res=torch.randn(M, N, generator=g) * 1.5,
                 table=torch.randn(300, N, generator=g) * 1.5,
                 side=torch.randn(M, 4, generator=g), side_w=torch.randn(N, 4, generator=g) * 0.5,
                 rand_mask=torch.rand(M, generator=g) < 0.05)
        d["prod"] = A.double() @ W.double().t()
        d["absprod"] = A.double().abs() @ W.double().abs().t()
        _cache[key] = d
    return _cache[key]


def mask_sets(M, bm, wm, rand_mask):
    """The masked-row sets of the issue: none; first and last row; one wave's slice of the first (interior) tile; ~5 % at random."""
    none = torch.zeros(M, dtype=torch.bool)
    ends = none.clone(); ends[0] = True; ends[M - 1] = True
    wr = bm // wm
    wave = none.clone(); wave[(wm - 1) * wr:min(M, wm * wr)] = True           # the LAST wave's rows of tile 0
    if not bool(wave.any()):
        wave[M - 1] = True
    rnd = rand_mask.clone()
    if M > 2:
        rnd[1] = True                                                          # (never empty)
    return {"none": none, "ends": ends, "wave": wave, "random": rnd}


def epilogue_cases(M, N, bm, wm, op):
    """[(name, kwargs for gemm_ref64 / gemm_bound / the launch)]: the aligned epilogue combinations of the issue for one shape."""
    res, table = op["res"], op["table"]
    b = dict(bias=op["bias"])
    cases = [("nobias", {}), ("bias", dict(b))]
    for act in ("relu", "gelu", "sigmoid", "tanh"):
        for ac in (0, 5, N):
            cases.append((f"{act}/act_cols={ac}", dict(b, act=act, act_cols=ac)))
    cases.append(("res_plain", dict(b, residual=res)))
    cases.append(("res_after", dict(b, act="relu", residual=res)))
    cases.append(("res_before", dict(b, act="relu", residual=res, res_first=True)))
    for rm in (7, bm, bm + 3, 100):
        for rf in (False, True):
            # (ReLU: the K-step-16 kernel's few-instruction epilogue takes it, with its own row arithmetic, where a tile lies inside a period)
            cases.append((f"res_mod={rm}/first={int(rf)}", dict(b, act="relu", residual=table[:rm], res_mod=rm, res_first=rf)))
    for name, rows in mask_sets(M, bm, wm, op["rand_mask"]).items():
        for mc in (6, N):
            cases.append((f"mask={name}/cols={mc}", dict(b, rowmask=rows, mask_cols=mc)))     # (no ReLU: column mask_cols is never 0 by itself)
    cases.append(("mask+res_after", dict(b, act="relu", residual=res, rowmask=mask_sets(M, bm, wm, op["rand_mask"])["random"], mask_cols=6)))
    cases.append(("all", full_combo(N, op)))
    return cases


FORM_TILES = {                      # form -> tiles (tests/test_gemm_forms_gpu.py sets the switches); "auto" picks 64x64 at these sizes
    "k16": (1, 2, 3, 4, 5, 7, 8, 9), "k16-stages3": (1, 2, 9), "k16-stages4": (3, 7, 8), "k16-nofast": (1, 2, 3), "k32": (1, 2, 3),
    "auto": (0,),
}
FORMS = [(f, t) for f, ts in FORM_TILES.items() for t in ts]
FULL_FORMS = {("k16", 2), ("k32", 3)}          # every epilogue combination at every shape, not at the main shape only
SPLITK = ((2, 100), (7, 100), (2, 272), (7, 272))      # (ksplit, K): the last chunk is short


def tile_geometry(tile):
    bm, bn = TILE_DIMS.get(tile, (64, 64))
    return bm, bn, TILE_WM.get(tile, 2)


def linear_plan(tile, full):
    """[((M, N, K), case name, epilogue kwargs)] of one form: every epilogue combination at the main shape (at all twelve shapes
    when `full`), the plain product with a bias at the other shapes."""
    bm, bn, wm = tile_geometry(tile)
    plan = []
    for shape in shapes_for(bm, bn):
        op = operands(*shape)
        if full or shape == main_shape(bm, bn):
            plan += [(shape, name, kw) for name, kw in epilogue_cases(shape[0], shape[1], bm, wm, op)]
        else:
            plan.append((shape, "bias", dict(bias=op["bias"])))
    return plan


def splitk_plan(tile):
    bm, bn, _ = tile_geometry(tile)
    M, N = 2 * bm + 37, bn + 36
    return [((M, N, K), ks, full_combo(N, operands(M, N, K))) for ks, K in SPLITK]


def full_combo(N, op, res_mod=100):
    """Everything at once: bias, GELU on 5 columns, periodic residual first, ~5 % of the rows masked on 6 columns."""
    M = op["A"].shape[0]
    rows = op["rand_mask"].clone(); rows[0] = True
    return dict(bias=op["bias"], act="gelu", act_cols=5, residual=op["table"][:res_mod], res_mod=res_mod, res_first=True,
                rowmask=rows, mask_cols=6)


NO_EPILOGUE = dict(bias=None, act=None, act_cols=0, residual=None, res_mod=0, res_first=False, rowmask=None, mask_cols=0, side=None,
                   side_w=None, side_cols=0)

# ---- convolution: (NI, H, W, Cin, Cout, KH, KW, stride, pad) ---------------------------------------------------------------------
CONV_GEOMS = [(2, 5, 7, 32, 40, 3, 3, 1, 1), (2, 9, 7, 32, 37, 3, 3, 2, 1), (3, 5, 6, 64, 40, 1, 1, 2, 0), (1, 9, 7, 32, 40, 5, 5, 1, 2),
              (2, 6, 5, 32, 40, 3, 3, 1, 0)]
CONV_1X3 = (2, 5, 7, 32, 40, 1, 3, 1, 1)                  # asymmetric filter; pad 1 in both directions: two output rows see padding only
CONV_TILES = (1, 2, 3, 7, 8, 9)


def conv_operands(geom):
    key = ("conv",) + tuple(geom)
    if key not in _cache:
        NI, H, W, Cin, Cout, KH, KW, stride, pad = geom
        g = torch.Generator().manual_seed(sum(v * (i + 3) for i, v in enumerate(geom)))
        x = torch.randn(NI, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, KH, KW, generator=g) / (Cin * KH * KW) ** 0.5
        prod = F.conv2d(x.double(), w.double(), None, stride, pad).permute(0, 2, 3, 1)
        OH, OW = prod.shape[1], prod.shape[2]
        absprod = F.conv2d(x.double().abs(), w.double().abs(), None, stride, pad).permute(0, 2, 3, 1)
        _cache[key] = dict(x=x, w=w, stride=stride, pad=pad, OH=OH, OW=OW, K=KH * KW * Cin, prod=prod.reshape(-1, Cout).contiguous(),
                           absprod=absprod.reshape(-1, Cout).contiguous(), bias=torch.randn(Cout, generator=g),
                           res=torch.randn(NI * OH * OW, Cout, generator=g) * 1.5)
    return _cache[key]


def conv_plan():
    """[(name, dict(x, w, stride, pad, K, prod, absprod, kw, launch))]: `launch` is what the GPU test varies beside the epilogue
    (image pitch, output pitch, split-K); the values do not depend on it."""
    plan = []
    for geom in CONV_GEOMS + [CONV_1X3]:
        c = conv_operands(geom)
        plan.append((f"conv{geom}", dict(c, kw=dict(bias=c["bias"]), launch={})))
    c = conv_operands(CONV_GEOMS[0])
    plan.append(("conv image pitch", dict(c, kw=dict(bias=c["bias"]), launch=dict(img_pad=64))))
    plan.append(("conv ldy", dict(c, kw=dict(bias=c["bias"], act="relu"), launch=dict(ldy_extra=3))))
    plan.append(("conv res_first relu", dict(c, kw=dict(bias=c["bias"], act="relu", residual=c["res"], res_first=True), launch={})))
    plan.append(("conv res after", dict(c, kw=dict(bias=c["bias"], residual=c["res"]), launch={})))
    plan.append(("conv ksplit=3", dict(c, kw=dict(bias=c["bias"], act="relu", residual=c["res"], res_first=True), launch=dict(ksplit=3))))
    return plan


# ---- the other entry points ----------------------------------------------------------------------------------------------------
SPLIT_SHAPES = [(2 * 128 + 37, N, K) for N in (164, 256) for K in (32, 96)]
SPLIT_BIG = {"f16x3": (200 * 128 + 37, 256, 32), "f16": (400 * 128 + 37, 256, 32)}       # reach the 256-column pre-split tile
SPLIT_INELIGIBLE = [("K=48", (293, 256, 48), {}), ("N=100", (293, 100, 96), {}), ("unaligned C", (293, 256, 32), dict(c_off=1)),
                    ("split-K", (293, 256, 96), dict(ksplit=2))]


def split_operands(M, N, K):
    key = ("split", M, N, K)
    if key not in _cache:
        g = torch.Generator().manual_seed(31 * M + 7 * N + K)
        A, W = split_operand((M, K), g), split_operand((N, K), g)
        d = dict(A=A, W=W, bias=torch.randn(N, generator=g), table=torch.randn(100, N, generator=g) * 1.5, rand_mask=torch.rand(M, generator=g) < 0.05)
        d["prod"] = A.double() @ W.double().t()
        d["absprod"] = A.double().abs() @ W.double().abs().t()
        _cache[key] = d
    return _cache[key]


def cat_plan():
    """cat2 / pix: [(name, A, W, kw, extra)] with A the logical [M, K1 + K2] operand."""
    plan = []
    g = torch.Generator().manual_seed(4242)
    NI, H2, W2 = 6, 7, 5
    for stride in (2, 1):
        OH, OW = (H2 - 1) // stride + 1, (W2 - 1) // stride + 1
        M = NI * OH * OW
        for K1 in (16, 48):
            for K2 in (16, 48):
                for N in (37, 260):
                    if stride == 1 and (K1, K2) != (16, 48):
                        continue
                    lda2 = K2 + 4
                    y = torch.randn(NI, OH, OW, K1, generator=g)
                    x2 = torch.randn(NI, H2, W2, lda2, generator=g)
                    W = torch.randn(N, K1 + K2, generator=g) / (K1 + K2) ** 0.5
                    bias = torch.randn(N, generator=g)
                    xs = x2[:, ::stride, ::stride, :K2].reshape(M, K2)
                    for act in (None, "relu"):
                        plan.append((f"cat2 s{stride} K1={K1} K2={K2} N={N} {act}", torch.cat([y.reshape(M, K1), xs], 1), W, dict(bias=bias, act=act),
                                     dict(kind="cat2", y=y, x2=x2, K2=K2, stride=stride)))
                    if K1 == 16:
                        Wp = W[:, K1:].contiguous()
                        act = "relu" if N == 37 else None
                        plan.append((f"pix s{stride} K={K2} N={N} {act}", xs, Wp, dict(bias=bias, act=act), dict(kind="pix", x=x2, K=K2, stride=stride)))
    return plan


_plans = {}


def other_plan():
    if "other" not in _plans:
        _plans["other"] = _other_plan()
    return _plans["other"]


def _other_plan():
    """[(name, A, W, epilogue kwargs, extra)] of the entry points beside the plain product and the convolution."""
    plan = cat_plan()
    g = torch.Generator().manual_seed(777)
    for M, N, K in ((1, 100, 48), (165, 100, 48), (165, 292, 20)):             # side term (N % 4 == 0)
        A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        bias, side, side_w = torch.randn(N, generator=g), torch.randn(M, 4, generator=g), torch.randn(N, 4, generator=g) * 0.5
        for sc in (0, 4, 68, N):
            plan.append((f"side M={M} N={N} K={K} cols={sc}", A, W, dict(bias=bias, side=side, side_w=side_w, side_cols=sc), dict(kind="side")))
    for M in (1, 63, 65, 200):                                                 # Linear + LayerNorm (N == 256)
        for K in (4, 20, 272):
            A, W = torch.randn(M, K, generator=g), torch.randn(256, K, generator=g) / K ** 0.5
            bias, res = torch.randn(256, generator=g), torch.randn(M, 256, generator=g) * 1.5 + 0.25
            ln = (torch.randn(256, generator=g), torch.randn(256, generator=g), torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g))
            plan.append((f"ln M={M} K={K}", A, W, dict(bias=bias, residual=res), dict(kind="ln", ln=ln)))
    for N in range(1, 9):                                                      # N <= 8: the row-dot kernel
        for K in (256, 512):
            for M in (1, 7, 1030):
                A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
                kw = [dict(bias=torch.randn(N, generator=g)), dict(bias=torch.randn(N, generator=g), act="sigmoid", act_cols=2), dict(act="relu")][(N + M) % 3]
                plan.append((f"rows_dot M={M} N={N} K={K}", A, W, kw, dict(kind="rows_dot")))
    shapes = SPLIT_SHAPES + list(SPLIT_BIG.values()) + [s for _, s, _ in SPLIT_INELIGIBLE]
    for M, N, K in dict.fromkeys(shapes):                                      # split precision: no epilogue, and all of it at once
        op = split_operands(M, N, K)
        for name, kw in (("none", {}), ("all", full_combo(N, op))):
            plan.append((f"split M={M} N={N} K={K} {name}", op["A"], op["W"], kw, dict(kind="split", op=op, epi=name)))
    return plan
