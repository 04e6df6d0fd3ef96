"""The MSDA sampling kernels (csrc/msda_fused.hip, csrc/msda.hip, mdqe_sample_levels_mean_f32) against float64 (tests/_msda_ref.py),
element by element, through the C entry points: every kernel instantiation the two dispatchers can launch is launched at the
smallest shape that reaches it (the restated dispatch names it; tests/test_msda_ref_cpu.py shows the lists are complete), a launch
passes only if EVERY element lies within its own derived bound, wrote all of its output view and nothing else -- every output is a
view at a pitch larger than its row inside a sentinel-filled buffer (the scheme of tests/test_gemm_forms_gpu.py) -- and value, offsets
and logits are pitched slices of one wider buffer with random numbers between them, as the engine passes them (the native op and
sample_levels_mean take contiguous tensors only: guard bands before and behind, and base addresses 4 and 8 bytes off).  Switch settings the
code comments declare bit-identical (every v2 map and waves hint, every staged build, the patch walk, the block order) must give equal
bits on the same inputs; the v1 kernel and the frame-major temporal form are held to the bound alone.  The achieved err / bound of
every kernel group goes to the parity-margin table (_golden.record_margin)."""
import ctypes

import pytest
import torch

import _msda_ref as R
from _golden import record_margin
from test_attn_norm_gpu import canary_nd, dense
from test_gemm_forms_gpu import SENT, check_canary

pytestmark = pytest.mark.gpu

WORST, COUNT, RAN = {}, {}, set()
FUSED_CASES = list(dict.fromkeys(n for n, _ in R.FUSED_LAUNCHES))
NATIVE_CASES = list(R.NATIVE_SHAPES)


def set_switches(sw):
    from mdqe_cvpr2023_amd._lib import check, lib
    check(lib.mdqe_debug_msda_variant(sw["variant"]))
    check(lib.mdqe_debug_msda_patch(sw["patch"]))
    check(lib.mdqe_debug_msda_stage_kb(sw["stage_kb"]))
    check(lib.mdqe_debug_msda_dec_stage_kb(sw["dec_stage_kb"]))
    check(lib.mdqe_debug_msda_tp_staged(sw["tp_staged"]))
    check(lib.mdqe_debug_msda_dec_staged(sw["dec_staged"]))
    check(lib.mdqe_debug_msda_dec_wpe8(sw["dec_wpe8"]))
    check(lib.mdqe_debug_msda_xcd_order(sw["xcd_order"]))
    check(lib.mdqe_debug_msda_op_staged(sw["op_staged"]))


@pytest.fixture(autouse=True)
def _restore_switches():
    try:
        yield
    finally:
        set_switches(R.DEFAULT_SWITCHES)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\ntest_msda_forms_gpu: {sum(COUNT.values())} launches compared element by element")
    for inst in sorted(COUNT):
        print(f"    {COUNT[inst]:4d}  {inst}: worst err / bound {WORST[inst]:.3f}")


def compare(inst, out, ref, bound, what):
    """Record the achieved err / bound of the worst element, then hold every element to its bound."""
    out = out.cpu().reshape(ref.shape)
    ratio, err, b = R.worst_ratio(out, ref, bound)
    record_margin("msda " + " ".join(inst.split(" ")[:2]), inst, err, scale=b, tol=1.0)
    WORST[inst] = max(WORST.get(inst, 0.0), ratio)
    COUNT[inst] = COUNT.get(inst, 0) + 1
    R.check_within(out, ref, bound, what)


def fused_device(c):
    """The device operands of a fused case: value, offs and logits as column slices of ONE wider buffer (random numbers in front of,
    between and behind them), the rest contiguous."""
    B, Q, M, D, LP = c["B"], c["Q"], c["M"], c["D"], c["L"] * c["P"]
    C, no, nl = M * D, 2 * M * LP, M * LP
    rows = max(c["value_rows"], B * Q)
    wide = torch.randn(rows, 4 + C + 4 + no + 8 + nl + 4, device="cuda")
    v, o, l = wide[:c["value_rows"], 4:4 + C], wide[:B * Q, 8 + C:8 + C + no], wide[:B * Q, 16 + C + no:16 + C + no + nl]
    v.copy_(c["value"]); o.copy_(c["offs"]); l.copy_(c["logits"])
    return dict(value=v, offs=o, logits=l, ref=c["ref"].cuda(), grid=c["grid"].cuda() if c["grid"] is not None else None,
                vidx=torch.tensor(c["vidx"], dtype=torch.int32, device="cuda") if c["vidx"] is not None else None)


def launch_fused(c, d, what):
    from mdqe_cvpr2023_amd import ops
    B, Q, M, D = c["B"], c["Q"], c["M"], c["D"]
    buf, out = canary_nd((B * Q, M * D), (M * D + 12, 1))
    ops.msda_fused(d["value"], d["offs"], d["logits"], d["ref"], c["levels"], B, Q, M, D, c["L"], c["P"], mode=c["mode"], grid=d["grid"],
                   groups=c["G"], scale=c["scale"], v_brows=c["v_brows"], out=out, vidx=d["vidx"])
    check_canary(buf, out, what)
    return out


def run_fused_case(name):
    c = R.fused_case(name)
    d = fused_device(c)
    first = None
    for n, sw in R.FUSED_LAUNCHES:
        if n != name:
            continue
        r = R.msda_fused_branch(c, sw)
        what = f"msda_fused {name} [{R.switch_label(sw)}] -> {r['inst']} LS={r['LS']} chunk={r['chunk']}"
        set_switches(sw)
        out = launch_fused(c, d, what)
        compare(r["inst"], out, c["out"], c["bound"], what)
        if R.same_bits_family(r["inst"]):
            if first is None:
                first = (out, what)
            else:
                assert torch.equal(out, first[0]), f"{what}: {int((out != first[0]).sum())} of {out.numel()} elements differ in bits from {first[1]}"
    RAN.add(name)


@pytest.mark.parametrize("name", FUSED_CASES)
def test_fused_entry_point(name):
    run_fused_case(name)


def test_tables_that_are_not_one_run_of_tokens_take_the_gather_form():
    """A gap between two coarse levels, levels in descending order: the staged kernel would address them inside ONE staged run of
    tokens, so the dispatcher must hand them to v2 (the default launch then equals the forced-v2 launch bit for bit and meets the
    bound); with the fine level last the staged levels are still back to back and stay staged."""
    for name in ("enc gap before level 3", "enc levels descending", "dec gap before level 2", "enc fine level last"):
        run_fused_case(name)


def native_device(c):
    B, S, M, D, Q, L, P, G = (c[k] for k in ("B", "S", "M", "D", "Q", "L", "P", "G"))

    def at(t, off):
        b = torch.randn(t.numel() + off + 8, device="cuda")
        v = b[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        return v

    H, W, St = c["levels"]
    return dict(value=at(c["value"], c["value_off"]), loc=at(c["loc"], c["la_off"]), attn=at(c["attn"], c["la_off"]),
                shapes=torch.tensor([[h, w] for h, w in zip(H, W)], dtype=torch.int64, device="cuda"),
                starts=torch.tensor(St, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("name", NATIVE_CASES)
def test_native_entry_point(name):
    from mdqe_cvpr2023_amd import ops
    c = R.native_case(name)
    d = native_device(c)
    B, Q, M, D = c["B"], c["Q"], c["M"], c["D"]
    first = None
    for n, sw in R.NATIVE_LAUNCHES:
        if n != name:
            continue
        r = R.msda_native_branch(c, sw)
        what = f"msda {name} [{R.switch_label(sw)}] -> {r['inst']} LS={r['LS']} budget={r['budget']}"
        set_switches(sw)
        buf, out = canary_nd((B, Q, M * D), (Q * M * D, M * D, 1), off=c["out_off"])
        ops.msda(d["value"], d["shapes"], d["starts"], d["loc"], d["attn"], groups=c["G"], scale=c["scale"], out=out)
        check_canary(buf, out, what)
        compare(r["inst"], out, c["out"], c["bound"], what)
        if not r["inst"].startswith("native v1"):             # v3: "same lane mapping and order of operations as v2: equal bits"
            if first is None:
                first = out
            else:
                assert torch.equal(out, first), f"{what}: {int((out != first).sum())} elements differ in bits from the default launch"
    RAN.add("native " + name)


@pytest.mark.parametrize("name", list(R.SLM_SHAPES))
def test_sample_levels_mean_entry_point(name):
    from mdqe_cvpr2023_amd import ops
    c = R.slm_case(name)
    buf, out = dense(tuple(c["out"].shape))
    ops.sample_levels_mean(c["tokens"].cuda(), c["coords"].cuda(), c["shapes"], c["starts"], out=out)
    check_canary(buf, out, f"sample_levels_mean {name}")
    compare("sample_levels_mean", out, c["out"], c["bound"], f"sample_levels_mean {name}")


def _fused_raw(c, d, out, **kw):
    """mdqe_msda_fused_f32 with single arguments replaced (the wrapper hides them)."""
    from mdqe_cvpr2023_amd._lib import cur_stream, lib, ptr
    arr = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])
    H, W, S = kw.get("levels", c["levels"])
    a = dict(value=ptr(d["value"]), ldv=d["value"].stride(0), offs=ptr(d["offs"]), ldo=d["offs"].stride(0), B=c["B"], Q=c["Q"], L=c["L"], P=c["P"], D=c["D"])
    a.update({k: v for k, v in kw.items() if k != "levels"})
    return lib.mdqe_msda_fused_f32(a["value"], a["ldv"], c["v_brows"], ptr(d["vidx"]), a["offs"], a["ldo"], ptr(d["logits"]), d["logits"].stride(0),
                                   ptr(d["ref"]), d["ref"].stride(0) if d["ref"].dim() == 3 else 0, d["ref"].shape[-1], c["mode"], ptr(d["grid"]),
                                   arr(H), arr(W), arr(S), a["B"], c["M"], a["D"], c["G"], a["L"], a["Q"], a["P"], c["scale"], ptr(out), out.stride(0),
                                   c["value_rows"], cur_stream())


def test_empty_and_refused_launches_touch_nothing():
    """B * Q == 0 returns OK; an L, P pair no kernel takes, an `offs` off its 16 bytes and a value pitch that is no multiple of 4
    are refused with an error code -- in every case before anything is launched: the guarded output keeps its sentinel."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import MdqeError, check, cur_stream, lib, ptr
    c = R.fused_case("enc 40 D=32")
    d = fused_device(c)
    buf, out = canary_nd((c["B"] * c["Q"], c["M"] * c["D"]), (c["M"] * c["D"] + 12, 1))
    untouched = lambda what: bool((buf == SENT).all()) or pytest.fail(f"{what}: wrote to the output")
    for kw in (dict(B=0), dict(Q=0)):
        assert _fused_raw(c, d, out, **kw) == 0, kw
        untouched(f"empty launch {kw}")
    lv16 = ([3] * 16, [5] * 16, [0] * 16)
    for what, kw in [(w, dict(kw, levels=lv16)) for w, kw in R.FUSED_REFUSED] + [
            ("offs off its 16 bytes", dict(offs=ptr(d["offs"]) + 4)), ("value pitch no multiple of 4", dict(ldv=d["value"].stride(0) + 1)),
            ("offs pitch no multiple of 4", dict(ldo=d["offs"].stride(0) + 2)), ("D no multiple of 4", dict(D=30))]:
        rc = _fused_raw(c, d, out, **kw)
        assert rc != 0, f"{what}: accepted"
        with pytest.raises(MdqeError):
            check(rc, what)
        untouched(what)
    torch.cuda.synchronize()
    untouched("after synchronising")
    # the native op and sample_levels_mean: empty launches
    n = R.native_case("v2 S < 64")
    nd = native_device(n)
    nbuf, nout = dense((n["B"], n["Q"], n["M"] * n["D"]))
    for B, Q in ((0, n["Q"]), (n["B"], 0)):
        assert lib.mdqe_msda_forward_grouped_f32(ptr(nd["value"]), ptr(nd["shapes"]), ptr(nd["starts"]), ptr(nd["loc"]), ptr(nd["attn"]), B, n["S"], n["M"],
                                                 n["D"], n["G"], n["L"], Q, n["P"], 1.0, ptr(nout), cur_stream()) == 0
    s = R.slm_case("four levels")
    ops.sample_levels_mean(s["tokens"].cuda()[:0], s["coords"].cuda()[:0], s["shapes"], s["starts"], out=nout.view(-1)[:0].view(0, s["coords"].shape[1], 32))
    torch.cuda.synchronize()
    assert bool((nbuf == SENT).all()), "an empty launch of the native op or of sample_levels_mean wrote to its output"


def test_every_instantiation_was_launched():
    """The launch table of this file lists every kernel instantiation named in tests/test_msda_ref_cpu.py with a non-zero count (checked
    when the whole file ran; a selection of its tests proves nothing about the rest)."""
    if not (set(FUSED_CASES) <= RAN and {"native " + n for n in NATIVE_CASES} <= RAN):
        return
    missing = [i for i in R.FUSED_INSTANCES + R.NATIVE_INSTANCES if COUNT.get(i, 0) == 0]
    assert not missing, missing
