"""Every dispatch branch of the attention kernels (mdqe_mha_small_f32, mdqe_window_attn_f32), of LayerNorm (four column templates,
with and without the Swin row map), of NHWC GroupNorm (one chunk, several, the capped count) and the exact Swin data-movement
kernels against float64 (tests/_attn_norm_ref.py), element by element: a launch passes only if EVERY element lies within its own
derived bound and if it wrote all of its output view and nothing else -- every output is a view of a larger buffer pre-filled with
a sentinel bit pattern (the scheme of tests/test_gemm_forms_gpu.py).  tests/test_attn_norm_ref_cpu.py shows on the same cases that
the bounds admit the formulas in float32 and reject sixteen one-off mistakes.  The achieved err / bound of every kernel group goes
to the parity-margin table (_golden.record_margin).

No launch here passes a misaligned pointer: the kernels assume 16-byte rows and do not check the base address."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _attn_norm_ref as R
from _golden import record_margin
from test_gemm_forms_gpu import SENT, check_canary

pytestmark = pytest.mark.gpu

COUNT = {}


@pytest.fixture(autouse=True)
def _restore_switches():
    from mdqe_cvpr2023_amd._lib import lib
    try:
        yield
    finally:
        lib.mdqe_debug_mha_variant(1)
        lib.mdqe_debug_window_attn_variant(1)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print(f"\ntest_attn_norm_gpu: {sum(COUNT.values())} launches compared element by element")
    for branch, n in sorted(COUNT.items()):
        print(f"    {n:5d}  {branch}")


def canary_nd(shape, strides, off=0, tail=8192):
    """A float32 view of the given shape and strides, `256 + off` floats into a sentinel-filled buffer with `tail` floats behind it."""
    front = 256 + off
    extent = sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    buf = torch.full((front + extent + tail,), SENT, dtype=torch.int32, device="cuda")
    return buf, buf.view(torch.float32).as_strided(tuple(shape), tuple(strides), front)


def rows_view(M, N, ld):
    return canary_nd((M, N), (ld, 1))


def dense(shape):
    strides = [1]
    for n in reversed(shape[1:]):
        strides.insert(0, strides[0] * n)
    return canary_nd(shape, strides)


def pitched(t, ld):
    """A device copy of the 2-D CPU tensor t as a view of pitch ld (random numbers between the rows)."""
    b = torch.randn(t.shape[0], ld, device="cuda")
    b[:, :t.shape[1]] = t.cuda()
    return b[:, :t.shape[1]]


def compare(group, stage, branch, out, ref, bound, what):
    """Record the achieved err / bound of the worst element, then hold every element to its bound."""
    out = out.cpu().reshape(ref.shape)
    _, err, b = R.worst_ratio(out, ref, bound)
    record_margin("attn_norm " + group, stage, err, scale=b, tol=1.0)
    R.check_within(out, ref, bound, what)
    COUNT[branch] = COUNT.get(branch, 0) + 1


# ---- mha_small ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,D,nh,B", R.MHA_SHAPES)
def test_mha_small_forms_layouts_and_value_sets(Q, D, nh, B):
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import check, lib
    C = nh * D
    for vs in R.MHA_SETS:
        c = R.mha_case(Q, D, nh, B, vs)
        fused = torch.cat([c["qk"], c["v"]], 1).cuda()                    # one [B*Q, 3C] buffer: q | k | v, pitch 3C
        inputs = {"contiguous": (c["qk"].cuda(), c["v"].cuda()), "fused": (fused[:, :2 * C], fused[:, 2 * C:])}
        inputs["out pitch"] = inputs["contiguous"]
        for variant in R.mha_variants(Q, D):
            check(lib.mdqe_debug_mha_variant(variant))
            for layout in (R.MHA_LAYOUTS if variant in (0, 1) else ("fused",)):
                what = f"mha_small Q={Q} D={D} nh={nh} B={B} {vs} {layout} variant {variant}"
                qk, v = inputs[layout]
                buf, out = rows_view(B * Q, C, C + 8 if layout == "out pitch" else C)
                ops.mha_small(qk, v, B, Q, C, nh, out=out)
                check_canary(buf, out, what)
                branch = R.mha_branch(Q, D, variant)
                compare("mha_small", f"{branch[4:]} {vs}", branch, out, c["ref"], c["bound"], what)


# ---- window_attn ----------------------------------------------------------------------------------------------------------------
def run_window(c, D, variant, what, ld_extra=0, ldo_extra=0, stage=""):
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    nwin, N, C, nh, nW = c["nwin"], c["N"], c["C"], c["nh"], c["nW"]
    qkv = pitched(c["qkv"], 3 * C + ld_extra)
    scale, bias = c["scale"].cuda(), c["bias"].cuda()
    mask = c["mask"].cuda() if c["mask"] is not None else None
    buf, out = rows_view(nwin * N, C, C + ldo_extra)
    check(lib.mdqe_debug_window_attn_variant(variant))
    check(lib.mdqe_window_attn_f32(ptr(qkv), qkv.stride(0), ptr(out), C + ldo_extra, nwin, N, C, nh, ptr(scale), ptr(bias), ptr(mask), nW,
                                   cur_stream()), what)
    check_canary(buf, out, what)
    branch = R.window_branch(D, N, variant)
    compare("window_attn", f"{branch[12:]} {stage}", branch, out, c["ref"], c["bound"], what)


@pytest.mark.parametrize("D,N", R.WIN_SHAPES)
def test_window_attn_forms_and_configurations(D, N):
    for config in R.WIN_CONFIGS:
        c = R.window_case(D, N, config)
        for variant in R.window_variants(D, N):
            run_window(c, D, variant, f"window_attn D={D} N={N} {config} variant {variant}", stage=config)
    for variant in (1, 0):
        if (D, N) in R.WIN_ZERO_ROWS:
            run_window(R.window_case(D, N, "shifted", zero_rows=True), D, variant, f"window_attn D={D} N={N} zero rows variant {variant}",
                       stage="zero rows")
        if (D, N) in R.WIN_PITCH:
            run_window(R.window_case(D, N, "shifted"), D, variant, f"window_attn D={D} N={N} ld = 3C + 4, ldo = C + 4 variant {variant}",
                       ld_extra=4, ldo_extra=4, stage="pitch")


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.LN_C + (R.LN_BIG[1],))
def test_layernorm_templates_and_variations(C):
    from mdqe_cvpr2023_amd import ops
    for rows, C_, kind in R.LN_CASES:
        if C_ != C:
            continue
        c = R.ln_case(rows, C, kind)
        what = f"layernorm rows={rows} C={C} {kind}"
        x, gamma, beta = c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda()
        buf, out = rows_view(rows, C, C)
        if kind == "post":
            ops.layernorm_post(x, gamma, beta, c["post"].cuda(), out=out)
        else:
            ops.layernorm(x, gamma, beta, res=c["res"].cuda() if c["res"] is not None else None, out=out)
        check_canary(buf, out, what)
        compare("layernorm", f"NCH={R.ln_nch(C)} {kind}" + (" two grid trips" if rows > 32768 else ""), f"layernorm NCH={R.ln_nch(C)}", out,
                c["ref"], c["bound"], what)


@pytest.mark.parametrize("shape", R.SWIN_SHAPES)
def test_layernorm_swin_scatter_in_place_and_out_of_place(shape):
    """Against shortcut + window_reverse(LN64(rows)): the rows of the zero padding are dropped (nothing outside the map is written)."""
    from mdqe_cvpr2023_amd import ops
    B, H, W, C, ws, shift = shape
    c = R.swin_case(*shape)
    rows, gamma, beta, x = c["rows"].cuda(), c["gamma"].cuda(), c["beta"].cuda(), c["x"].cuda()
    for in_place in (False, True):
        what = f"layernorm_swin_scatter {shape} in place={in_place}"
        buf, out = dense((B, H, W, C))
        if in_place:
            out.copy_(x)
            ops.layernorm_swin_scatter(rows, gamma, beta, out, ws, shift)
        else:
            ops.layernorm_swin_scatter(rows, gamma, beta, x, ws, shift, out=out)
        check_canary(buf, out, what)
        compare("layernorm_swin_scatter", f"NCH={R.ln_nch(C)} in place={in_place}", f"layernorm NCH={R.ln_nch(C)} with the Swin row map", out,
                c["ln_ref"], c["ln_bound"], what)


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.GN_SHAPES)
def test_groupnorm_layouts_activations_and_mean_over_std(shape):
    from mdqe_cvpr2023_amd import ops
    NI, HW, C, G = shape
    nchunks = R.gn_geometry(HW, C)[0]
    branch = f"groupnorm {'one chunk' if nchunks == 1 else 'the capped 64 chunks' if (HW + 255) // 256 > 64 else 'several chunks'}"
    for ratio in R.GN_RATIOS:
        c = R.gn_case(NI, HW, C, G, ratio)
        xc, gamma, beta = c["x"].cuda(), c["gamma"].cuda(), c["beta"].cuda()
        xp = torch.randn(NI, HW, C + 4, device="cuda")
        xp[:, :, :C] = xc
        for act in R.GN_ACTS:
            for layout in R.GN_LAYOUTS:
                what = f"groupnorm {shape} mean/std {ratio} {act} {layout}"
                x = xc
                if layout == "token slice":            # out = tokens[:, s0:s0 + HW] of an [NI, Ntok, C] buffer (engine: a level of the encoder input)
                    buf, out = canary_nd((NI, HW, C), ((HW + 11) * C, C, 1), off=5 * C)
                elif layout == "x pitch":              # pixel pitch C + 4 on both sides
                    x = xp[:, :, :C]
                    buf, out = canary_nd((NI, HW, C), (HW * (C + 4), C + 4, 1))
                else:
                    buf, out = dense((NI, HW, C))
                if layout == "in place":
                    out.copy_(xc)
                    x = out
                ops.groupnorm_nhwc(x, G, gamma, beta, act=act, out=out)
                check_canary(buf, out, what)
                compare("groupnorm", f"kappa~{1 + ratio * ratio:.0f} {branch[10:]}", branch, out, c["ref"][act], c["bound"][act], what)
        if ratio == R.GN_RATIOS[-1]:                   # what the single-pass variance costs: torch's CPU fp32 on the same input (no assertion)
            y = F.group_norm(c["x"].permute(0, 2, 1), G, c["gamma"], c["beta"], R.EPS).permute(0, 2, 1)
            _, err, b = R.worst_ratio(y, c["ref"][None], c["bound"][None])
            record_margin("attn_norm groupnorm", f"kappa~{1 + ratio * ratio:.0f} {branch[10:]} torch CPU fp32 (diagnostic)", err, scale=b, tol=None)


# ---- the exact data-movement kernels -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SWIN_SHAPES)
def test_swin_window_gather_and_scatter_are_exact(shape):
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    B, H, W, C, ws, shift = shape
    c = R.swin_case(*shape)
    Hp, Wp = R.padded(H, W, ws)
    x, rows = c["x"].cuda(), c["rows"].cuda()
    buf, out = rows_view(B * Hp * Wp, C, C)
    check(lib.mdqe_swin_window_f32(ptr(x), None, ptr(out), B, H, W, C, ws, shift, 0, cur_stream()), "gather")
    check_canary(buf, out, f"swin_window_gather {shape}")
    compare("swin_window", "gather", "swin_window gather", out, c["gather"].double(), torch.zeros(c["gather"].shape, dtype=torch.float64),
            f"swin_window_gather {shape}")
    for in_place in (False, True):
        what = f"swin_window_scatter_add {shape} in place={in_place}"
        buf, out = dense((B, H, W, C))
        if in_place:
            out.copy_(x)
        check(lib.mdqe_swin_window_f32(ptr(rows), ptr(out if in_place else x), ptr(out), B, H, W, C, ws, shift, 1, cur_stream()), what)
        check_canary(buf, out, what)
        compare("swin_window", "scatter_add", "swin_window scatter_add", out, c["scatter"].double(), torch.zeros(c["scatter"].shape, dtype=torch.float64), what)


@pytest.mark.parametrize("geom", R.PATCH_MERGE)
def test_patch_merge_gather_is_exact(geom):
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    B, H, W, C = geom
    x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * W + C))
    ref = R.patch_merge_ref(x)
    xd = x.cuda()
    buf, out = rows_view(ref.shape[0], 4 * C, 4 * C)
    check(lib.mdqe_patch_merge_gather_f32(ptr(xd), ptr(out), B, H, W, C, cur_stream()), "patch_merge_gather")
    check_canary(buf, out, f"patch_merge_gather {geom}")
    compare("patch_merge_gather", "gather", "patch_merge_gather", out, ref.double(), torch.zeros(ref.shape, dtype=torch.float64), f"patch_merge_gather {geom}")


@pytest.mark.parametrize("u8", [True, False], ids=["uint8", "float32"])
@pytest.mark.parametrize("geom", R.PATCH4)
def test_patch4_im2col(geom, u8):
    from mdqe_cvpr2023_amd._lib import check, cur_stream, lib, ptr
    NI, h, w, Hp, Wp = geom
    f = R.patch4_frames(NI, h, w, u8)
    ref = R.patch4_ref(f, Hp, Wp, R.PATCH4_MEAN, R.PATCH4_STD)
    fd = f.cuda()
    buf, out = rows_view(ref.shape[0], 48, 48)
    m, s = (ctypes.c_float * 3)(*R.PATCH4_MEAN), (ctypes.c_float * 3)(*R.PATCH4_STD)
    check(lib.mdqe_patch4_im2col_f32(ptr(fd), int(u8), 3 * h * w, NI, h, w, Hp, Wp, m, s, ptr(out), cur_stream()), "patch4_im2col")
    check_canary(buf, out, f"patch4_im2col {geom} u8={u8}")
    compare("patch4_im2col", "uint8" if u8 else "float32", "patch4_im2col", out, ref, 2 * R.U * ref.abs(), f"patch4_im2col {geom} u8={u8}")


# ---- refusals: MDQE_REQUIRE before any launch ------------------------------------------------------------------------------------
def test_refused_arguments():
    """Each is refused with MdqeError before anything is launched, and nothing is written."""
    from mdqe_cvpr2023_amd import ops
    from mdqe_cvpr2023_amd._lib import MdqeError, check, cur_stream, lib, ptr
    buf, out = rows_view(600, 2052, 2052)
    src = torch.zeros(600 * 2052 * 3, device="cuda")

    def mha(Q, C, nh, ldqk=None):
        check(lib.mdqe_mha_small_f32(ptr(src), ldqk or 2 * C, ptr(src), C, ptr(out), C, 2, Q, C, nh, cur_stream()), "mha_small")

    def gn(C, G, ldy=None):
        ws = torch.zeros(lib.mdqe_groupnorm_workspace_bytes(1, 64), dtype=torch.uint8, device="cuda")
        check(lib.mdqe_groupnorm_nhwc_f32(ptr(src), C, 0, ptr(out), ldy or C, 0, 1, 7, C, G, ptr(src), ptr(src), 1e-5, 0, ptr(ws), cur_stream()), "groupnorm")

    refused = {
        "mha Q = 257": lambda: mha(257, 64, 2),
        "mha D = 12": lambda: mha(16, 24, 2),
        "mha ldqk % 4 != 0": lambda: mha(16, 64, 2, ldqk=130),
        "layernorm C = 2052": lambda: ops.layernorm(src[:4 * 2052].view(4, 2052), src[:2052], src[:2052], out=out),
        "layernorm C = 6": lambda: ops.layernorm(src[:24].view(4, 6), src[:6], src[:6], out=out),
        "groupnorm C = 1028": lambda: gn(1028, 4),
        "groupnorm G = 65": lambda: gn(260, 65),
        "groupnorm C % G != 0": lambda: gn(32, 3),
        "groupnorm ldy < C": lambda: gn(32, 4, ldy=28),
    }
    for what, call in refused.items():
        with pytest.raises(MdqeError):
            call()
        print(f"\nrefused: {what}")
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
