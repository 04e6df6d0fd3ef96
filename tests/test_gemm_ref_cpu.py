"""The GEMM tests' criterion (tests/_gemm_ref.py) can tell right from wrong, shown without a GPU:
(a) the float64 reference equals a composition of torch's own operators; (b) the formula evaluated in float32 on the CPU lies
inside the per-element bound on every case the GPU file (tests/test_gemm_forms_gpu.py) runs -- the reference arithmetic alone never
trips it; (c) each of nine one-off mistakes an epilogue can make lies outside the bound on at least one element."""
import pytest
import torch
import torch.nn.functional as F

import _gemm_ref as R

TORCH_ACT = {None: lambda x: x, "relu": F.relu, "gelu": F.gelu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}


def composed(op, kw, dt=torch.float64, drop_k=False, res_shift=0, ignore_mod=False, dact=0, dmask=0, swap_first=False, mask_early=False,
             bias_shift=0, dside=0):
    """The header's formula as a composition of F.linear, torch's activations, indexing and masked_fill -- written separately from
    _gemm_ref._epilogue -- with switches for the mutants of (c)."""
    A, W = op["A"].to(dt), op["W"].to(dt)
    M, N = A.shape[0], W.shape[0]
    bias = kw.get("bias")
    if bias is not None:
        bias = torch.roll(bias, -bias_shift).to(dt)                      # bias_shift = 1: column n takes the bias of column n + 1
    y = F.linear(A[:, :-1], W[:, :-1], bias) if drop_k else F.linear(A, W, bias)
    sc = kw.get("side_cols", 0)
    if kw.get("side") is not None and sc > 0:
        sc = min(N, sc + dside)
        y = torch.cat([y[:, :sc] + F.linear(kw["side"].to(dt), kw["side_w"].to(dt)[:sc]), y[:, sc:]], 1)
    r = None
    if kw.get("residual") is not None:
        res, rm = kw["residual"].to(dt), kw.get("res_mod", 0)
        rows = torch.arange(M) + res_shift
        if ignore_mod:
            r = op["table"].to(dt)[rows]                                  # the table read as if it had a row per output row
        else:
            r = res[rows % rm] if rm > 0 else res[rows.clamp_max(M - 1)]
    first = bool(kw.get("res_first", False)) != swap_first
    if r is not None and first:
        y = y + r
    act, ac = kw.get("act"), kw.get("act_cols", 0)
    if act is not None:
        c = N if ac <= 0 else min(N, ac + dact)
        y = torch.cat([TORCH_ACT[act](y[:, :c]), y[:, c:]], 1)
    mask, mc = kw.get("rowmask"), kw.get("mask_cols", 0)

    def apply_mask(y):
        if mask is None or mc <= 0:
            return y
        c = min(N, mc + dmask)
        return torch.cat([y[:, :c].masked_fill(mask[:, None], 0.0), y[:, c:]], 1)
    if mask_early:
        y = apply_mask(y)
    if r is not None and not first:
        y = y + r
    if not mask_early:
        y = apply_mask(y)
    return y


def _side_kw(op, N, side_cols):
    return dict(bias=op["bias"], side=op["side"], side_w=op["side_w"], side_cols=side_cols)


def test_reference_equals_a_composition_of_torch_operators():
    bm, bn, wm = R.tile_geometry(3)
    M, N, K = R.main_shape(bm, bn)
    op = R.operands(M, N, K)
    cases = R.epilogue_cases(M, N, bm, wm, op) + [("side", _side_kw(op, N, 4)), ("side_all", _side_kw(op, N, N))]
    for name, kw in cases:
        ref = R.gemm_ref64(op["A"], op["W"], **kw)
        want = composed(op, kw)
        # (F.linear and A @ W^T may sum in different orders: float64 rounding only; the activation's two spellings likewise)
        assert float((ref - want).abs().max()) < 1e-12, name
        assert torch.equal(ref, R.gemm_ref64(op["A"], op["W"], prod=op["prod"], **kw)), name


def _assert_inside(out, ref, bound, what):
    R.check_within(out, ref, bound, what)


@pytest.mark.parametrize("form,tile", R.FORMS, ids=[f"{f}-t{t}" for f, t in R.FORMS])
def test_float32_evaluation_is_inside_the_bound_linear(form, tile):
    plan = R.linear_plan(tile, (form, tile) in R.FULL_FORMS) + [(s, f"ksplit={ks}", kw) for s, ks, kw in R.splitk_plan(tile)]
    for shape, name, kw in plan:
        op = R.operands(*shape)
        out = R.gemm_eval32(op["A"], op["W"], **kw)
        _assert_inside(out, R.gemm_ref64(op["A"], op["W"], prod=op["prod"], **kw), R.gemm_bound(op["A"], op["W"], absprod=op["absprod"], **kw),
                       f"{shape} {name}")


def test_float32_evaluation_is_inside_the_bound_other_entry_points():
    n = 0
    for what, A, W, kw, extra in R.other_plan():
        ref = R.gemm_ref64(A, W, **kw)
        for mode in extra.get("modes", ("f32",)):
            _assert_inside(R.gemm_eval32(A, W, **kw), ref, R.gemm_bound(A, W, mode=mode, **kw), f"{what} {mode}")
        if "ln" in extra:
            g1, b1, g2, b2 = extra["ln"]
            x32 = R.gemm_eval32(A, W, **kw)
            y32 = F.layer_norm(x32, (256,), g1, b1, 1e-5)
            ref1, bd1 = R.ln_ref64(ref, g1, b1, 1e-5), R.ln_bound(ref, R.gemm_bound(A, W, **kw), g1, b1, 1e-5)
            _assert_inside(y32, ref1, bd1, f"{what} LayerNorm")
            _assert_inside(F.layer_norm(y32, (256,), g2, b2, 1e-5), R.ln_ref64(ref1, g2, b2, 1e-5), R.ln_bound(ref1, bd1, g2, b2, 1e-5),
                           f"{what} second LayerNorm")
        n += 1
    assert n > 50


def test_float32_evaluation_is_inside_the_bound_conv():
    for what, c in R.conv_plan():
        x, w = c["x"], c["w"]
        y32 = F.conv2d(x, w, None, c["stride"], c["pad"]).permute(0, 2, 3, 1).reshape(-1, w.shape[0])
        out = R._epilogue(y32, torch.float32, **{**R.NO_EPILOGUE, **c["kw"]})
        ref = R.gemm_ref64(None, None, prod=c["prod"], **c["kw"])
        _assert_inside(out, ref, R.gemm_bound(None, None, absprod=c["absprod"], K=c["K"], **c["kw"]), what)


MUTANTS = [
    # (mutant, switches of `composed`, the planned case it is applied to)
    ("the last k dropped", dict(drop_k=True), "bias"),
    ("the residual row off by one", dict(res_shift=1), "res_mod=7/first=0"),
    ("the residual row off by one, full residual", dict(res_shift=1), "res_plain"),
    ("res_mod ignored", dict(ignore_mod=True), "res_mod=100/first=0"),
    ("act_cols off by one", dict(dact=1), "gelu/act_cols=5"),
    ("act_cols off by one (all)", dict(dact=1), "all"),
    ("mask_cols off by one", dict(dmask=1), "mask=random/cols=6"),
    ("mask_cols off by one (all)", dict(dmask=1), "all"),
    ("res_first swapped", dict(swap_first=True), "res_before"),
    ("res_first swapped (periodic)", dict(swap_first=True), "res_mod=7/first=1"),
    ("the mask applied before the residual", dict(mask_early=True), "mask+res_after"),
    ("the bias of column n + 1", dict(bias_shift=1), "bias"),
    ("the side term on one column too many", dict(dside=1), "side"),
]


@pytest.mark.parametrize("tile", sorted(R.TILE_DIMS))
@pytest.mark.parametrize("mutant,switches,case", MUTANTS, ids=[m[0].replace(" ", "_") for m in MUTANTS])
def test_mutant_is_outside_the_bound(tile, mutant, switches, case):
    """On the inputs the GPU test uses at this tile's main shape.  The correct composition passes the same check."""
    bm, bn, wm = R.tile_geometry(tile)
    M, N, K = R.main_shape(bm, bn)
    op = R.operands(M, N, K)
    cases = dict(R.epilogue_cases(M, N, bm, wm, op))
    cases["side"] = _side_kw(op, N, 4)
    kw = cases[case]
    ref, bound = R.gemm_ref64(op["A"], op["W"], prod=op["prod"], **kw), R.gemm_bound(op["A"], op["W"], absprod=op["absprod"], **kw)
    assert R.within(composed(op, kw, dt=torch.float32), ref, bound)
    assert not R.within(composed(op, kw, dt=torch.float32, **switches), ref, bound), mutant
    assert not R.within(composed(op, kw, **switches), ref, bound), mutant


def test_check_within_names_the_worst_element_and_rejects_nan():
    ref = torch.zeros(3, 4, dtype=torch.float64)
    bound = torch.full((3, 4), 1e-6, dtype=torch.float64)
    out = torch.zeros(3, 4)
    R.check_within(out, ref, bound)
    out[1, 2] = 1e-5
    with pytest.raises(AssertionError, match=r"worst at \(1, 2\)"):
        R.check_within(out, ref, bound)
    out[1, 2] = float("nan")
    with pytest.raises(AssertionError):
        R.check_within(out, ref, bound)
    # one wrong element whose magnitude is far below the output's largest: an aggregate max-norm would pass it
    ref = torch.tensor([[1000.0, 1e-3]], dtype=torch.float64)
    out = torch.tensor([[1000.0, 2e-3]])
    assert float((out.double() - ref).abs().max() / ref.abs().max()) < 2e-5
    with pytest.raises(AssertionError):
        R.check_within(out, ref, torch.tensor([[1e-4, 1e-9]], dtype=torch.float64))
