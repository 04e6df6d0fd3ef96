"""float64 references, per-element error bounds and case lists of the attention and normalisation kernels (a helper, not a
conftest): mdqe_mha_small_f32, mdqe_window_attn_f32, mdqe_layernorm_f32 / _post_f32 / _swin_scatter_f32, mdqe_groupnorm_nhwc_f32
and the exact Swin data-movement kernels.  tests/test_attn_norm_ref_cpu.py shows on these cases that every bound admits the
formula evaluated in float32 on the CPU and rejects sixteen one-off mistakes; tests/test_attn_norm_gpu.py holds the kernels to
them.  U = 2^-24 is the fp32 unit roundoff (as in _gemm_ref).

ATTENTION.  Both kernels compute out = sum_j p_j v_j / sum_j p_j with p_j = exp(t_j - max t) from logits t_j:

    mha_small      t = (q * D^-0.5) . k
    window_attn    t = scale[h] * (q / max(|q|, 1e-12)) . (k / max(|k|, 1e-12)) + bias[h, i, j] + mask[win % nW, i, j]

A computed weight is w_j = p_j (1 + e_j); then, to first order, |out - ref| <= sum_j p_j |e_j - ebar| |v_j| with
ebar = sum_j p_j e_j, which `attend_bound` evaluates in float64 as sum_j p_j (E_j + Ebar) |v_j| for E_j >= |e_j|.  E_j is

    dt_j                          the logit's absolute error (below)
  + 2 U |t_j - max|               the rounding of the subtraction, and the rounding of the log2(e) constant in the forms that
                                  keep their logits in units of log 2 (it scales every difference by the same 1 + delta);
                                  at a logit scale of 100 this term dominates
  + EXP_REL * (1 + R)             the device exponential, once for the weight itself and once for every rescaling exp(m_old -
                                  m_new) behind it in the one-pass ("online") softmax of the scalar forms: R is the number of
                                  times the running maximum of the row rises after its first key, counted on the float64 logits
                                  (the rescalings' argument roundings telescope into the U |t_j - max| above; R = 0 for the
                                  MFMA forms, which take the maximum first, so one bound serves both)

and the two sums add (N + 3) U * sum_j p_j |v_j| (the N products and additions of the numerator, the denominator, the division).
A factor 1.01 stands for second-order terms (E is below 1e-3 at every case here) and 1e-35 for weights that fp32 flushes to
zero where float64 does not.

    EXP_REL = 4 U = 2^-22.   ASSUMED.  The ROCm installation this was written against documents no accuracy for expf or for the
    hardware exp2 (v_exp_f32): no ULP figure appears in its headers (include/hip), its share/doc tree or the OCML bitcode's
    accompanying files.  So, as the plan for this test prescribes for that case: 1 ulp (2 U) for each, times 2 for the log2(e)
    pre-scaling that expf does internally and the MFMA forms do on the logits.  It is not tuned from any kernel's output.

The logit error dt:

    mha_small      (D + 2) U * D^-0.5 * sum_c |q_c| |k_c|  +  U |t|
                   a term of the D-term fp32 product passes its own product rounding, at most D - 1 additions, the rounding of
                   q * scale and of the scale constant; one more rounding for the forms that rescale the finished sum.
    window_attn    ((D + 2) + 2 (D / 2 + 4)) U * |scale| * sum_c |qn_c| |kn_c|  +  3 U (|scale * s| + |bias| + |mask|)
                   the same product of the NORMALISED vectors, plus the normalisation itself, which the plan's sketch left out:
                   |x|^2 is a D-term sum of squares (relative error D U, halved by the square root), then the square root, the
                   division and the product with each element (at most 4 U together, the divide and sqrt being correctly
                   rounded without fast-math): (D / 2 + 4) U per normalised element, for q and for k.  The last term: the
                   roundings of scale * s + bias (+ mask), where the MFMA form adds bias + mask first and folds scale and
                   log2(e) into q -- three roundings at most on each of the summands.

LAYERNORM.  _gemm_ref.ln_bound with dx = U |x + res| (the one rounding of the sum; 0 without `res`), plus U |ref| where `post`
(or the Swin shortcut) is added behind the norm.

GROUPNORM.  The bound is of the documented algorithm (csrc/norm.hip): a thread of gn_partial_kernel sums x and x^2 of
m = ceil(per / tpr) pixels of one channel in fp32 (per = ceil(HW / nchunks) pixels per block, nchunks = min(64, ceil(HW / 256)),
tpr = 256 / (C / 4) pixel rows per block pass); everything after that is double, and var = E[x^2] - mean^2.  With E2 = E[x^2],
ma = E|x| over the group:

    |d mean|  <=  m U ma  +  U |mean|                                (the fp32 sums; the mean kept as a float)
    |d var|   <=  (3 m + 2) U E2                                     (m U E2 from the sum of squares -- m - 1 additions and the
                                                                      square's rounding; 2 |mean| |d mean| <= 2 m U E2 from the
                                                                      mean, which the sketch "kappa (m + 2) U" left out: the two
                                                                      sums round independently, so nothing cancels)
    relative  ev = (3 m + 2) U kappa,   kappa = E2 / (var + eps) = 1 + mean^2 / var
    |d xh|    <=  r (|d mean| + U |x - mean|)  +  |xh| (1.01 ev / 2 + 3 U)          r = 1 / sqrt(var + eps), xh = (x - mean) r
    |d pre|   <=  |gamma| |d xh|  +  3 U (|gamma xh| + |beta|)
    |y - ref| <=  L_act |d pre|  +  a_act  +  U |ref|                                (L_act, a_act: _gemm_ref.ACT_L, ACT_A)

DATA MOVEMENT.  swin_window_gather / scatter_add and patch_merge_gather copy (or add once): exact equality with the restatements
below, which pad FIRST and then roll by -shift (swin_transformer_v2.py:252-282).  patch4_im2col normalises: 2 U relative.
"""
import torch
import torch.nn.functional as F

from _gemm_ref import ACT_A, ACT_L, U, act64, check_within, ln_bound, ln_ref64, within  # noqa: F401  (re-exported)

EXP_REL = 4 * U                     # ASSUMED (module docstring)
FLUSH = 1e-35
EPS = 1e-5
_cache = {}


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 3) * 7919 ** (i % 3) * int(v) for i, v in enumerate(key)) % (2 ** 31))


# ---- attention ------------------------------------------------------------------------------------------------------------------
def heads(x, G, N, nh):
    """[G * N, nh * D] -> [G, nh, N, D] in float64."""
    return x.double().reshape(G, N, nh, -1).permute(0, 2, 1, 3)


def unheads(o):
    G, nh, N, D = o.shape
    return o.permute(0, 2, 1, 3).reshape(G * N, nh * D)


def attend(t, vh):
    return torch.softmax(t, -1) @ vh


def records(t):
    """How often the running maximum of a row rises after its first key: [..., N, 1]."""
    if t.shape[-1] < 2:
        return torch.zeros(t.shape[:-1] + (1,), dtype=torch.float64)
    cm = t.cummax(-1).values
    return (t[..., 1:] > cm[..., :-1]).sum(-1, keepdim=True).double()


def attend_bound(t, dt, vh):
    """Bound of softmax(t) @ vh computed in fp32 from logits that are off by at most dt (module docstring)."""
    N = t.shape[-1]
    p = torch.softmax(t, -1)
    e = dt + 2 * U * (t.max(-1, keepdim=True).values - t) + EXP_REL * (1 + records(t))
    ebar = (p * e).sum(-1, keepdim=True)
    av = vh.abs()
    return 1.01 * ((p * (e + ebar)) @ av + (N + 3) * U * (p @ av)) + FLUSH


def mha_logits(qk, B, Q, C, nh):
    """(t, dt) [B, nh, Q, Q] of mha_small: t = (q * D^-0.5) . k."""
    D = C // nh
    q, k = heads(qk[:, :C], B, Q, nh), heads(qk[:, C:2 * C], B, Q, nh)
    t = (q * D ** -0.5) @ k.transpose(-1, -2)
    dt = (D + 2) * U * D ** -0.5 * (q.abs() @ k.abs().transpose(-1, -2)) + U * t.abs()
    return t, dt


def mha_ref64(qk, v, B, Q, C, nh):
    """softmax((q * D^-0.5) k^T) v;  qk [B * Q, 2C] (q | k), v [B * Q, C] -> [B * Q, C] float64."""
    return unheads(attend(mha_logits(qk, B, Q, C, nh)[0], heads(v, B, Q, nh)))


def mha_bound(qk, v, B, Q, C, nh):
    t, dt = mha_logits(qk, B, Q, C, nh)
    return unheads(attend_bound(t, dt, heads(v, B, Q, nh)))


def normalize64(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)           # F.normalize, eps 1e-12


def window_logits(qkv, nwin, N, C, nh, scale, bias, mask=None, nW=1):
    """(t, dt) [nwin, nh, N, N] of the cosine window attention."""
    D = C // nh
    qn, kn = normalize64(heads(qkv[:, :C], nwin, N, nh)), normalize64(heads(qkv[:, C:2 * C], nwin, N, nh))
    sc = scale.double().view(1, nh, 1, 1)
    s = (qn @ kn.transpose(-1, -2)) * sc
    b = bias.double()[None]
    t = s + b
    extra = s.abs() + b.abs()
    if mask is not None:
        m = mask.double()[torch.arange(nwin) % nW][:, None]
        t = t + m
        extra = extra + m.abs()
    dt = ((D + 2) + 2 * (D / 2 + 4)) * U * sc.abs() * (qn.abs() @ kn.abs().transpose(-1, -2)) + 3 * U * extra
    return t, dt


def window_attn_ref64(qkv, nwin, N, C, nh, scale, bias, mask=None, nW=1):
    t, _ = window_logits(qkv, nwin, N, C, nh, scale, bias, mask, nW)
    return unheads(attend(t, heads(qkv[:, 2 * C:3 * C], nwin, N, nh)))


def window_attn_bound(qkv, nwin, N, C, nh, scale, bias, mask=None, nW=1):
    t, dt = window_logits(qkv, nwin, N, C, nh, scale, bias, mask, nW)
    return unheads(attend_bound(t, dt, heads(qkv[:, 2 * C:3 * C], nwin, N, nh)))


# mha cases: (Q, D, nh, B); B in {1, 3} and nh in {2, 8} alternate
MHA_SHAPES = [(1, 32, 8, 1), (16, 32, 2, 3), (17, 32, 8, 1), (196, 32, 2, 3), (208, 32, 8, 1), (209, 32, 2, 3), (256, 32, 8, 3),
              (17, 24, 2, 3), (196, 24, 8, 1), (256, 24, 2, 3),
              (5, 16, 8, 1), (100, 16, 2, 3), (5, 8, 2, 3), (100, 8, 8, 1)]
MHA_SETS = ("normal", "peaked", "flat")
MHA_LAYOUTS = ("contiguous", "fused", "out pitch")


def mha_variants(Q, D):
    """Debug switch values to run: 1 (the default choice) and 0 (scalar) everywhere; the other wave counts (2 to 5) and the
    V-from-global forms (6 to 8) where the MFMA kernels apply and the issue asks (Q = 196 and 17, D = 32 and 24)."""
    return (1, 0) + ((2, 3, 4, 5, 6, 7, 8) if D in (32, 24) and Q in (196, 17) else ())


def mha_branch(Q, D, variant):
    """Which kernel mdqe_mha_small_f32 launches (csrc/decoder_ops.hip), as the report names it."""
    if D in (32, 24) and Q <= 208 and variant != 0:
        if 6 <= variant <= 8:
            return f"mha mfma D={D} V from global, {({6: 7, 7: 4, 8: 3})[variant]} waves"
        return f"mha mfma D={D} {({2: 3, 3: 7, 4: 13, 5: 4}).get(variant, 7 if D == 32 else 4)} waves"
    return f"mha scalar D={D}"


def window_branch(D, N, variant):
    """Which kernel mdqe_window_attn_f32 launches (csrc/swin.hip)."""
    if D == 32 and N <= 192 and N % 4 == 0 and variant != 0:
        return f"window_attn mfma {({3: 5, 4: 9}).get(variant, 3)} waves"
    return f"window_attn scalar D={D}"


def mha_case(Q, D, nh, B, vs):
    """dict(qk [B*Q, 2C], v [B*Q, C], ref, bound), computed once (callers must not modify it)."""
    key = ("mha", Q, D, nh, B, vs)
    if key not in _cache:
        C = nh * D
        g = _gen(Q, D, nh, B, MHA_SETS.index(vs))
        q = torch.randn(B, Q, nh, D, generator=g) * 2
        k = torch.randn(B, Q, nh, D, generator=g) * 2
        v = torch.randn(B * Q, C, generator=g)
        if vs == "peaked":                       # query i's key (7 i + 3) % Q lies about 60 above what a key at right angles gets
            pi = (7 * torch.arange(Q) + 3) % Q
            kp = k[:, pi]
            q = 0.3 * q + 60.0 * D ** 0.5 * kp / (kp * kp).sum(-1, keepdim=True)
        elif vs == "flat":                       # all keys equal: the softmax is uniform, the output the mean of v
            k = k[:, :1].expand(B, Q, nh, D)
        qk = torch.cat([q.reshape(B * Q, C), k.reshape(B * Q, C)], 1).contiguous()
        _cache[key] = dict(qk=qk, v=v, ref=mha_ref64(qk, v, B, Q, C, nh), bound=mha_bound(qk, v, B, Q, C, nh))
    return _cache[key]


# window_attn cases: every (D, N) in two configurations
WIN_SHAPES = [(32, N) for N in (4, 36, 64, 144, 192)] + [(32, N) for N in (49, 196, 256)] + [(D, N) for D in (24, 16, 8) for N in (16, 49)]
WIN_CONFIGS = {"plain": dict(nW=1, masked=False, scale=1.0), "shifted": dict(nW=6, masked=True, scale=100.0)}
WIN_NH = 2


def window_variants(D, N):
    """1 (MFMA with three waves where it applies) and 0 (scalar) everywhere; 2 to 4 (three, five and nine waves) at N = 144, 36."""
    return (1, 0) + ((2, 3, 4) if D == 32 and N in (144, 36) else ())


def window_case(D, N, config, zero_rows=False):
    """dict(qkv [nwin*N, 3C], nwin, N, C, nh, scale [nh], bias [nh, N, N], mask [nW, N, N] or None, nW, ref, bound)."""
    key = ("win", D, N, config, zero_rows)
    if key not in _cache:
        cf = WIN_CONFIGS[config]
        nh, nW = WIN_NH, cf["nW"]
        C, nwin = nh * D, 2 * nW + 1
        g = _gen(D, N, nW, int(zero_rows), 5)
        qkv = torch.randn(nwin * N, 3 * C, generator=g)
        if zero_rows:                                                   # F.normalize's eps branch: a zero q row, a zero k row
            w = qkv.view(nwin, N, 3 * C)
            w[:, 1, :C] = 0.0
            w[:, 2, C:2 * C] = 0.0
        scale = cf["scale"] * (1.0 - 0.05 * torch.arange(nh) / nh)      # (head 0 at SwinV2's clamp where scale = 100)
        bias = torch.randn(nh, N, N, generator=g)
        mask = None
        if cf["masked"]:                                                # 0 / -100 between tokens of different regions, per window
            region = torch.randint(0, 3, (nW, N), generator=g)
            mask = (region[:, :, None] != region[:, None, :]).float() * -100.0
        a = (qkv, nwin, N, C, nh, scale, bias, mask, nW)
        _cache[key] = dict(qkv=qkv, nwin=nwin, N=N, C=C, nh=nh, scale=scale, bias=bias, mask=mask, nW=nW, ref=window_attn_ref64(*a),
                           bound=window_attn_bound(*a))
    return _cache[key]


WIN_ZERO_ROWS = [(32, 36), (24, 16)]
WIN_PITCH = [(32, 36), (32, 49)]                # ld = 3C + 4, ldo = C + 4


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------
LN_C = (4, 192, 256, 260, 384, 512, 516, 768, 1024, 1028, 1536, 2048)
LN_KINDS = ("plain", "res", "post", "mean1000", "const")
LN_BIG = (32768 + 37, 64)                        # the grid-stride loop's second trip: more rows than 8192 blocks x 4 waves
LN_CASES = [(rows, C, kind) for C in LN_C for rows in (1, 5) for kind in LN_KINDS] + [LN_BIG + ("plain",)]


def ln_nch(C):
    return 1 if C <= 256 else 2 if C <= 512 else 4 if C <= 1024 else 8


def ln_out64(x, res, post, gamma, beta, res_after=False):
    x64 = x.double() + (res.double() if res is not None and not res_after else 0.0)
    y = ln_ref64(x64, gamma, beta, EPS)
    if res is not None and res_after:
        y = y + res.double()
    return y + post.double() if post is not None else y


def ln_out_bound(x, res, post, gamma, beta):
    x64 = x.double() + (res.double() if res is not None else 0.0)
    dx = U * x64.abs() if res is not None else torch.zeros_like(x64)
    b = ln_bound(x64, dx, gamma, beta, EPS)
    return b + U * ln_out64(x, res, post, gamma, beta).abs() if post is not None else b


def ln_case(rows, C, kind):
    key = ("ln", rows, C, kind)
    if key not in _cache:
        g = _gen(rows, C, LN_KINDS.index(kind), 11)
        x = torch.randn(rows, C, generator=g) * 3 + 1
        if kind == "mean1000":
            x = torch.randn(rows, C, generator=g) + 1000.0
        if kind == "const":
            x[rows // 2] = 3.0
        res = torch.randn(rows, C, generator=g) if kind == "res" else None
        post = torch.randn(rows, C, generator=g) * 2 if kind == "post" else None
        gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
        _cache[key] = dict(x=x, res=res, post=post, gamma=gamma, beta=beta, ref=ln_out64(x, res, post, gamma, beta),
                           bound=ln_out_bound(x, res, post, gamma, beta))
    return _cache[key]


# (B, H, W, C, ws, shift): the shapes of test_swin_window_partition_fused_into_gemm_and_norm_is_bit_identical and one tiny one
# (and that one at the widths of the other three LayerNorm templates, which Swin-L's norm1 takes)
SWIN_SHAPES = [(3, 15, 27, 96, 6, 0), (2, 15, 27, 96, 6, 3), (2, 30, 54, 192, 12, 6), (1, 8, 14, 48, 4, 2), (1, 5, 3, 32, 4, 1),
               (1, 5, 3, 384, 4, 1), (1, 5, 3, 768, 4, 1), (1, 5, 3, 1536, 4, 1)]


def padded(H, W, ws):
    return (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws


def window_gather_ref(x, ws, shift):
    """[B, H, W, C] -> window rows [B * Hp * Wp, C]: zero pad, THEN roll by -shift, then partition."""
    B, H, W, C = x.shape
    Hp, Wp = padded(H, W, ws)
    x = F.pad(x, (0, 0, 0, Wp - W, 0, Hp - H))
    x = torch.roll(x, (-shift, -shift), (1, 2))
    return x.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, C)


def window_reverse_ref(rows, B, H, W, ws, shift):
    """Window rows [B * Hp * Wp, C] -> [B, H, W, C]: reverse the partition, roll back by +shift, crop the padding."""
    Hp, Wp = padded(H, W, ws)
    x = rows.view(B, Hp // ws, Wp // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, -1)
    return torch.roll(x, (shift, shift), (1, 2))[:, :H, :W].contiguous()


def patch_merge_ref(x):
    """[B, H, W, C] -> [B * H2 * W2, 4C] = (x[0::2, 0::2] | x[1::2, 0::2] | x[0::2, 1::2] | x[1::2, 1::2]) of the map padded to even."""
    B, H, W, C = x.shape
    x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).reshape(-1, 4 * C)


def patch4_ref(frames, Hp, Wp, mean, std, dtype=torch.float64):
    """(x - mean) / std, zero pad to (Hp, Wp), 4x4 / stride-4 patches with k = c * 16 + kh * 4 + kw: [NI * Hp/4 * Wp/4, 48].
    mean and std are the fp32 numbers the C ABI is handed (float[3]): the subtraction and the division round once each, 2 U."""
    NI, _, h, w = frames.shape
    mean, std = (torch.tensor(t, dtype=torch.float32).to(dtype).view(1, 3, 1, 1) for t in (mean, std))
    x = (frames.to(dtype) - mean) / std
    x = F.pad(x, (0, Wp - w, 0, Hp - h))
    return F.unfold(x, 4, stride=4).transpose(1, 2).reshape(-1, 48)


def swin_case(B, H, W, C, ws, shift):
    """The inputs of the gather / scatter kernels and of layernorm_swin_scatter at one shape, with their references."""
    key = ("swin", B, H, W, C, ws, shift)
    if key not in _cache:
        g = _gen(B, H, W, C, ws, shift)
        Hp, Wp = padded(H, W, ws)
        x = torch.randn(B, H, W, C, generator=g)
        rows = torch.randn(B * Hp * Wp, C, generator=g) * 2 + 0.5
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
        ln = ln_ref64(rows.double(), gamma, beta, EPS)
        ln_ref = x.double() + window_reverse_ref(ln, B, H, W, ws, shift)
        lnb = window_reverse_ref(ln_bound(rows.double(), torch.zeros_like(ln), gamma, beta, EPS), B, H, W, ws, shift) + U * ln_ref.abs()
        _cache[key] = dict(x=x, rows=rows, gamma=gamma, beta=beta, gather=window_gather_ref(x, ws, shift),
                           scatter=x + window_reverse_ref(rows, B, H, W, ws, shift), ln_ref=ln_ref, ln_bound=lnb)
    return _cache[key]


PATCH_MERGE = [(2, 4, 6, 8), (2, 5, 7, 8), (3, 1, 1, 8)]                 # (B, H, W, C)
PATCH4 = [(2, 13, 18, 16, 20), (1, 9, 7, 16, 12)]                       # (NI, h, w, Hp, Wp): h, w no multiples of 4; whole padded patches
PATCH4_MEAN, PATCH4_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def patch4_frames(NI, h, w, u8):
    g = _gen(NI, h, w, int(u8), 17)
    f = torch.randint(0, 256, (NI, 3, h, w), generator=g, dtype=torch.uint8)
    return f if u8 else f.float() + torch.rand(NI, 3, h, w, generator=g)


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------
GN_SHAPES = [(1, 1, 4, 1), (2, 7, 24, 24), (2, 63, 192, 24), (1, 65, 256, 32), (2, 300, 1024, 64), (1, 16384 + 300, 32, 32), (2, 240, 256, 8)]
GN_ACTS = (None, "relu", "gelu")
GN_RATIOS = (0.0, 3.0, 10.0)                     # per-group |mean| / std: kappa about 1, 10, 100
GN_LAYOUTS = ("contiguous", "in place", "token slice", "x pitch")


def gn_geometry(HW, C):
    """(nchunks, per, tpr, m) of gn_partial_kernel: m pixels go through one thread's fp32 sums."""
    nchunks = min(64, max(1, (HW + 255) // 256))
    per = (HW + nchunks - 1) // nchunks
    tpr = 256 // (C // 4)
    return nchunks, per, tpr, (per + tpr - 1) // tpr


def _gn_parts(x, G):
    NI, HW, C = x.shape
    xg = x.double().view(NI, HW, G, C // G)
    mean = xg.mean((1, 3), keepdim=True)
    var = xg.var((1, 3), unbiased=False, keepdim=True)
    return xg, mean, var


def gn_ref64(x, G, gamma, beta, act, eps=EPS):
    """x [NI, HW, C] channels-last; nn.GroupNorm (biased variance, eps inside the root), then the activation."""
    xg, mean, var = _gn_parts(x, G)
    xh = ((xg - mean) / torch.sqrt(var + eps)).view(x.shape)
    return act64(xh * gamma.double() + beta.double(), act)


def gn_kappa(x, G, eps=EPS):
    xg, mean, var = _gn_parts(x, G)
    return float(((xg * xg).mean((1, 3), keepdim=True) / (var + eps)).max())


def gn_bound(x, G, gamma, beta, act, eps=EPS):
    NI, HW, C = x.shape
    m = gn_geometry(HW, C)[3]
    xg, mean, var = _gn_parts(x, G)
    E2, ma = (xg * xg).mean((1, 3), keepdim=True), xg.abs().mean((1, 3), keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    ev = (3 * m + 2) * U * E2 * r * r
    xh = (xg - mean) * r
    dxh = r * (m * U * ma + U * mean.abs() + U * (xg - mean).abs()) + xh.abs() * (1.01 * ev / 2 + 3 * U)
    g_, b_ = gamma.double(), beta.double()
    xh, dxh = xh.view(x.shape), dxh.reshape(x.shape)
    dpre = g_.abs() * dxh + 3 * U * ((g_ * xh).abs() + b_.abs())
    return ACT_L[act] * dpre + ACT_A[act] + U * act64(xh * g_ + b_, act).abs()


def gn_case(NI, HW, C, G, ratio):
    """dict(x, gamma, beta, kappa, ref[act], bound[act]) of one shape and mean / std ratio."""
    key = ("gn", NI, HW, C, G, ratio)
    if key not in _cache:
        g = _gen(NI, HW, C, G, int(ratio))
        std = torch.rand(NI, 1, G, 1, generator=g) * 1.5 + 0.5
        sign = torch.randint(0, 2, (NI, 1, G, 1), generator=g).float() * 2 - 1
        x = (torch.randn(NI, HW, G, C // G, generator=g) * std + sign * ratio * std).view(NI, HW, C).contiguous()
        gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
        _cache[key] = dict(x=x, gamma=gamma, beta=beta, kappa=gn_kappa(x, G),
                           ref={a: gn_ref64(x, G, gamma, beta, a) for a in GN_ACTS}, bound={a: gn_bound(x, G, gamma, beta, a) for a in GN_ACTS})
    return _cache[key]


def worst_ratio(out, ref, bound):
    """(err / bound at the element where that ratio is largest, its |err|, its bound): what _golden.record_margin is given."""
    err = (out.double() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
    return float(ratio.flatten()[i]), float(err.flatten()[i]), float(bound.flatten()[i])
