"""The proof that tests/test_attn_norm_gpu.py can fail and need not: on the cases of tests/_attn_norm_ref.py (no GPU), every bound
admits an independent float32 evaluation of the documented formula (torch on the CPU) and rejects sixteen one-off mistakes, each
applied to the float64 reference on a case that exposes it."""
import pytest
import torch
import torch.nn.functional as F

import _attn_norm_ref as R

WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for group, v in sorted(WORST.items()):
        print(f"\ntest_attn_norm_ref_cpu: {group}: worst float32-CPU err / bound {v:.3f}")


def admit(group, out, ref, bound, what):
    ratio, _, _ = R.worst_ratio(out, ref, bound)
    WORST[group] = max(WORST.get(group, 0.0), ratio)
    R.check_within(out, ref, bound, what)
    assert ratio < 1.0, (what, ratio)


def rejected(mutant, ref, bound, what):
    assert mutant.shape == ref.shape
    assert not R.within(mutant, ref, bound), f"{what}: the bound admits this mistake"
    print(f"\nrejected: {what}")


def heads32(x, G, N, nh):
    return x.float().reshape(G, N, nh, -1).permute(0, 2, 1, 3)


def act32(x, act):
    return x if act is None else F.relu(x) if act == "relu" else F.gelu(x)


# ---- the bounds admit float32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,D,nh,B", R.MHA_SHAPES)
def test_mha_bound_admits_float32(Q, D, nh, B):
    C = nh * D
    for vs in R.MHA_SETS:
        c = R.mha_case(Q, D, nh, B, vs)
        q, k, v = heads32(c["qk"][:, :C], B, Q, nh), heads32(c["qk"][:, C:], B, Q, nh), heads32(c["v"], B, Q, nh)
        out = R.unheads(torch.softmax((q * D ** -0.5) @ k.transpose(-1, -2), -1) @ v)
        admit("mha_small", out, c["ref"], c["bound"], f"mha Q={Q} D={D} nh={nh} B={B} {vs}")


def test_mha_reference_is_nn_multihead_attention():
    """The float64 formula against torch's own multi_head_attention_forward with identity projections, in float64."""
    Q, D, nh, B = 17, 24, 2, 3
    C = nh * D
    c = R.mha_case(Q, D, nh, B, "normal")
    q, k, v = (t.double().view(B, Q, C).transpose(0, 1) for t in (c["qk"][:, :C], c["qk"][:, C:], c["v"]))
    eye = torch.eye(C, dtype=torch.float64)
    out, _ = F.multi_head_attention_forward(q, k, v, C, nh, torch.cat([eye, eye, eye]), torch.zeros(3 * C, dtype=torch.float64), None, None, False,
                                            0.0, eye, torch.zeros(C, dtype=torch.float64), need_weights=False)
    assert float((out.transpose(0, 1).reshape(B * Q, C) - c["ref"]).abs().max()) < 1e-12


def window_eval32(c, zero_rows=False):
    nwin, N, C, nh, nW = c["nwin"], c["N"], c["C"], c["nh"], c["nW"]
    q, k, v = (heads32(c["qkv"][:, i * C:(i + 1) * C], nwin, N, nh) for i in range(3))
    t = F.normalize(q, dim=-1) @ F.normalize(k, dim=-1).transpose(-1, -2) * c["scale"].view(1, nh, 1, 1) + c["bias"][None]
    if c["mask"] is not None:
        t = t + c["mask"][torch.arange(nwin) % nW][:, None]
    return R.unheads(torch.softmax(t, -1) @ v)


@pytest.mark.parametrize("D,N", R.WIN_SHAPES)
def test_window_attn_bound_admits_float32(D, N):
    for config in R.WIN_CONFIGS:
        c = R.window_case(D, N, config)
        admit("window_attn", window_eval32(c), c["ref"], c["bound"], f"window_attn D={D} N={N} {config}")
    if (D, N) in R.WIN_ZERO_ROWS:
        c = R.window_case(D, N, "shifted", zero_rows=True)
        admit("window_attn", window_eval32(c), c["ref"], c["bound"], f"window_attn D={D} N={N} zero rows")


@pytest.mark.parametrize("C", R.LN_C + (R.LN_BIG[1],))
def test_layernorm_bound_admits_float32(C):
    for rows, C_, kind in R.LN_CASES:
        if C_ != C:
            continue
        c = R.ln_case(rows, C, kind)
        x = c["x"] + c["res"] if c["res"] is not None else c["x"]
        out = F.layer_norm(x, (C,), c["gamma"], c["beta"], R.EPS)
        if c["post"] is not None:
            out = out + c["post"]
        admit("layernorm", out, c["ref"], c["bound"], f"layernorm rows={rows} C={C} {kind}")


@pytest.mark.parametrize("shape", R.SWIN_SHAPES)
def test_layernorm_swin_scatter_bound_admits_float32(shape):
    B, H, W, C, ws, shift = shape
    c = R.swin_case(*shape)
    out = c["x"] + R.window_reverse_ref(F.layer_norm(c["rows"], (C,), c["gamma"], c["beta"], R.EPS), B, H, W, ws, shift)
    admit("layernorm_swin_scatter", out, c["ln_ref"], c["ln_bound"], f"layernorm_swin_scatter {shape}")


@pytest.mark.parametrize("shape", R.GN_SHAPES)
def test_groupnorm_bound_admits_float32(shape):
    NI, HW, C, G = shape
    for ratio in R.GN_RATIOS:
        c = R.gn_case(NI, HW, C, G, ratio)
        y = F.group_norm(c["x"].permute(0, 2, 1), G, c["gamma"], c["beta"], R.EPS).permute(0, 2, 1)
        for act in R.GN_ACTS:
            admit(f"groupnorm kappa~{1 + ratio * ratio:.0f}", act32(y, act), c["ref"][act], c["bound"][act], f"groupnorm {shape} mean/std {ratio} {act}")


@pytest.mark.parametrize("geom", R.PATCH4)
def test_patch4_bound_admits_float32(geom):
    NI, h, w, Hp, Wp = geom
    for u8 in (True, False):
        f = R.patch4_frames(NI, h, w, u8)
        ref = R.patch4_ref(f, Hp, Wp, R.PATCH4_MEAN, R.PATCH4_STD)
        admit("patch4_im2col", R.patch4_ref(f, Hp, Wp, R.PATCH4_MEAN, R.PATCH4_STD, torch.float32), ref, 2 * R.U * ref.abs(), f"patch4 {geom} u8={u8}")


def test_case_lists_reach_every_dispatch_branch():
    """mdqe_mha_small_f32 and mdqe_window_attn_f32 (the dispatch restated in _attn_norm_ref): every scalar template, every wave
    count of the MFMA forms, the V-from-global forms; the 64 KB of dynamic LDS at Q = N = 256; both sides of Q = 208 / 209."""
    mha = {R.mha_branch(Q, D, v) for Q, D, _, _ in R.MHA_SHAPES for v in R.mha_variants(Q, D)}
    want = {f"mha scalar D={D}" for D in (32, 24, 16, 8)} | {f"mha mfma D={D} {w} waves" for D in (32, 24) for w in (3, 4, 7, 13)}
    want |= {f"mha mfma D={D} V from global, {w} waves" for D in (32, 24) for w in (7, 4, 3)}
    assert mha == want
    assert R.mha_branch(208, 32, 1) != R.mha_branch(209, 32, 1) and {(208, 32), (209, 32), (256, 32), (256, 24)} <= {s[:2] for s in R.MHA_SHAPES}
    win = {R.window_branch(D, N, v) for D, N in R.WIN_SHAPES for v in R.window_variants(D, N)}
    assert win == {f"window_attn scalar D={D}" for D in (32, 24, 16, 8)} | {f"window_attn mfma {w} waves" for w in (3, 5, 9)}
    assert all(R.window_branch(32, N, 1) == "window_attn scalar D=32" for N in (49, 196, 256))
    assert {R.ln_nch(s[3]) for s in R.SWIN_SHAPES} == {1, 2, 4, 8}          # the Swin row map under every LayerNorm template


def test_groupnorm_geometry_reaches_one_several_and_the_capped_chunk_count():
    chunks = {shape: R.gn_geometry(shape[1], shape[2])[0] for shape in R.GN_SHAPES}
    assert 1 in chunks.values() and 2 in chunks.values() and chunks[(1, 16384 + 300, 32, 32)] == 64
    assert (16384 + 300 + 255) // 256 > 64                                  # the cap binds
    assert {R.ln_nch(C) for C in R.LN_C} == {1, 2, 4, 8}
    assert 256 % (192 // 4) != 0 and 256 % (24 // 4) != 0                   # tpr = 256 / (C / 4) with a remainder


# ---- the bounds reject the seeded mistakes ----------------------------------------------------------------------------------------
def test_mha_mistakes_are_rejected():
    Q, D, nh, B = 17, 32, 8, 1
    C = nh * D
    for vs in ("flat", "normal"):
        c = R.mha_case(Q, D, nh, B, vs)
        t, _ = R.mha_logits(c["qk"], B, Q, C, nh)
        vh = R.heads(c["v"], B, Q, nh)
        pad_t = torch.cat([t, torch.zeros_like(t[..., :1])], -1)            # one padded key of the 16-key tile, score 0, value 0
        pad_v = torch.cat([vh, torch.zeros_like(vh[..., :1, :])], -2)
        rejected(R.unheads(R.attend(pad_t, pad_v)), c["ref"], c["bound"], f"mha {vs}: one padded key included with score 0")
        rejected(R.unheads(R.attend(t[..., :-1], vh[..., :-1, :])), c["ref"], c["bound"], f"mha {vs}: the last key dropped")
    c = R.mha_case(Q, D, nh, B, "peaked")                                  # (7 i + 3) % 17 == 16 for i = 14: its peak is the last key
    t, _ = R.mha_logits(c["qk"], B, Q, C, nh)
    vh = R.heads(c["v"], B, Q, nh)
    rejected(R.unheads(R.attend(t[..., :-1], vh[..., :-1, :])), c["ref"], c["bound"], "mha peaked: the last key dropped")
    c = R.mha_case(Q, D, nh, B, "normal")
    t, _ = R.mha_logits(c["qk"], B, Q, C, nh)
    rejected(R.unheads(R.attend(t * D ** 0.5, R.heads(c["v"], B, Q, nh))), c["ref"], c["bound"], "mha: D^-0.5 omitted")


def test_window_attn_mistakes_are_rejected():
    D, N = 32, 36
    c = R.window_case(D, N, "shifted")
    nwin, C, nh, nW, qkv = c["nwin"], c["C"], c["nh"], c["nW"], c["qkv"]
    q, k, vh = (R.heads(qkv[:, i * C:(i + 1) * C], nwin, N, nh) for i in range(3))
    sc, bias = c["scale"].double().view(1, nh, 1, 1), c["bias"].double()[None]
    win = torch.arange(nwin)
    mask = c["mask"].double()
    cos = R.normalize64(q) @ R.normalize64(k).transpose(-1, -2)
    right = cos * sc + bias + mask[win % nW][:, None]
    assert torch.equal(R.unheads(R.attend(right, vh)), c["ref"])            # (the pieces below are the reference's own)
    mutants = {
        "mask[win // nW] instead of win % nW": cos * sc + bias + mask[win // nW][:, None],
        "bias indexed [h, j, i]": cos * sc + bias.transpose(-1, -2) + mask[win % nW][:, None],
        "k not normalised": (R.normalize64(q) @ k.transpose(-1, -2)) * sc + bias + mask[win % nW][:, None],
        "scale applied after the bias": (cos + bias) * sc + mask[win % nW][:, None],
        "one padded key included with score 0": None,
    }
    for what, t in mutants.items():
        v_ = vh
        if t is None:
            t = torch.cat([right, torch.zeros_like(right[..., :1])], -1)
            v_ = torch.cat([vh, torch.zeros_like(vh[..., :1, :])], -2)
        rejected(R.unheads(R.attend(t, v_)), c["ref"], c["bound"], f"window_attn: {what}")
    c = R.window_case(D, N, "plain")                                        # also at scale 1 without a mask
    q, k, vh = (R.heads(c["qkv"][:, i * C:(i + 1) * C], c["nwin"], N, nh) for i in range(3))
    t = (R.normalize64(q) @ k.transpose(-1, -2)) * c["scale"].double().view(1, nh, 1, 1) + c["bias"].double()[None]
    rejected(R.unheads(R.attend(t, vh)), c["ref"], c["bound"], "window_attn plain: k not normalised")


def test_layernorm_mistakes_are_rejected():
    for C in (4, 192):
        c = R.ln_case(5, C, "const")
        x = c["x"].double()
        mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
        noeps = (x - mean) / torch.sqrt(var) * c["gamma"].double() + c["beta"].double()
        rejected(noeps, c["ref"], c["bound"], f"layernorm C={C}: eps omitted on the constant row")
        c = R.ln_case(5, C, "plain")
        x = c["x"].double()
        unb = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=True, keepdim=True) + R.EPS) * c["gamma"].double() + c["beta"].double()
        rejected(unb, c["ref"], c["bound"], f"layernorm C={C}: unbiased variance")
        c = R.ln_case(5, C, "res")
        rejected(R.ln_out64(c["x"], c["res"], None, c["gamma"], c["beta"], res_after=True), c["ref"], c["bound"],
                 f"layernorm C={C}: res added after the norm")


def test_groupnorm_mistakes_are_rejected():
    for shape, ratio in (((2, 63, 192, 24), 3.0), ((2, 240, 256, 8), 10.0), ((2, 300, 1024, 64), 0.0)):
        NI, HW, C, G = shape
        cpg = C // G
        c = R.gn_case(NI, HW, C, G, ratio)
        x, ga, be = c["x"], c["gamma"], c["beta"]
        shifted = R.gn_ref64(torch.roll(x, -1, 2), G, torch.roll(ga, -1), torch.roll(be, -1), "gelu").roll(1, 2)
        rejected(shifted, c["ref"]["gelu"], c["bound"]["gelu"], f"groupnorm {shape}: group boundary shifted by one channel")
        bygroup = R.gn_ref64(x, G, ga[torch.arange(C) // cpg], be[torch.arange(C) // cpg], "gelu")
        rejected(bygroup, c["ref"]["gelu"], c["bound"]["gelu"], f"groupnorm {shape}: gamma / beta indexed by group")
        for act in ("relu", "gelu"):
            xg = x.double().view(NI, HW, G, cpg)
            mean, var = xg.mean((1, 3), keepdim=True), xg.var((1, 3), unbiased=False, keepdim=True)
            xh = ((xg - mean) / torch.sqrt(var + R.EPS)).view(x.shape)
            rejected(R.act64(xh, act) * ga.double() + be.double(), c["ref"][act], c["bound"][act], f"groupnorm {shape}: {act} before the affine")


def test_data_movement_mistakes_are_rejected():
    """Exact kernels: the reference restatement differs from each mistake in at least one element."""
    for shape in R.SWIN_SHAPES:
        B, H, W, C, ws, shift = shape
        if shift == 0:
            continue
        c = R.swin_case(*shape)
        Hp, Wp = R.padded(H, W, ws)
        assert (Hp, Wp) != (H, W)                                           # (every shifted shape also pads)
        plus =torch.roll(F.pad(c["x"], (0, 0, 0, Wp - W, 0, Hp - H)), (shift, shift), (1, 2))
        plus = plus.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)
        assert not torch.equal(plus, c["gather"]), f"{shape}: window shift by +shift is not told apart"
        roll_first = F.pad(torch.roll(c["x"], (-shift, -shift), (1, 2)), (0, 0, 0, Wp - W, 0, Hp - H))
        roll_first = roll_first.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)
        assert not torch.equal(roll_first, c["gather"]), f"{shape}: roll before pad is not told apart"
        back = torch.roll(c["rows"].view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C), (-shift, -shift), (1, 2))
        assert not torch.equal(c["x"] + back[:, :H, :W], c["scatter"]), f"{shape}: reverse shift by -shift is not told apart"
        ln_wrong = c["x"].double() + torch.roll(R.ln_ref64(c["rows"].double(), c["gamma"], c["beta"], R.EPS)
                                                .view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C),
                                                (-shift, -shift), (1, 2))[:, :H, :W]
        rejected(ln_wrong, c["ln_ref"], c["ln_bound"], f"layernorm_swin_scatter {shape}: window shift the wrong way")
        print(f"\nrejected: swin window {shape}: shift by +shift; roll before pad")
    for B, H, W, C in R.PATCH_MERGE:
        if H * W == 1:
            continue
        x = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(H * W))
        xp = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        rowmajor = torch.cat([xp[:, 0::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 0::2], xp[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)
        assert not torch.equal(rowmajor, R.patch_merge_ref(x))
        print(f"\nrejected: patch merge {(B, H, W, C)}: parts in the order (0,0), (0,1), (1,0), (1,1)")


def test_data_movement_references_invert_each_other():
    for shape in R.SWIN_SHAPES:
        B, H, W, C, ws, shift = shape
        c = R.swin_case(*shape)
        assert torch.equal(R.window_reverse_ref(c["gather"], B, H, W, ws, shift), c["x"])
