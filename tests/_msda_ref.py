"""float64 references, per-element error bounds, the restated dispatch and the case lists of the multi-scale deformable attention
(MSDA) sampling kernels (a helper, not a conftest): mdqe_msda_fused_f32 (csrc/msda_fused.hip), mdqe_msda_forward_grouped_f32
(csrc/msda.hip) and mdqe_sample_levels_mean_f32 (csrc/decoder_ops.hip).  tests/test_msda_ref_cpu.py shows on these cases that every
bound admits the formula evaluated in float32 on the CPU and rejects the seeded one-off mistakes, and that the case lists reach every
kernel instantiation the two dispatchers can launch; tests/test_msda_forms_gpu.py holds the kernels to the bounds.  U = 2^-24 is the
fp32 unit roundoff (as in _gemm_ref).

THE OPERATION (kernel headers; ms_deform_attn.py:141-170 / 198-235 of the reference module).  For a query q of batch element b, head
m, channel d, with a level table of G * L entries (H, W, first row) indexed g * L + l and sample i = l * P + p of the L * P samples:

    out = scale * sum_g sum_i w_i * S_{g*L+l(i)}(x_i, y_i)           l(i) = i / P
    S_t(x, y)    bilinear interpolation of level t of the element's value block at pixel (X, Y) = (x W_t - 0.5, y H_t - 0.5); a
                 corner outside [0, H) x [0, W) counts as zero (so S is zero for X <= -1, X >= W, Y <= -1, Y >= H)
    native op    (x, y) = loc, w = attn: both inputs
    fused mode 0 (x, y) = ref_xy + off / 8                                        w = softmax over the L * P logits
    fused mode 1 (x, y) = ref_xy + (grid * 0.5 * wh + clamp(delta, +-8 wh)) / 8   w = the same;  ref = (x, y, w, h)
    value block  rows vidx[b] * v_brows .. of the [rows, M * D] value matrix (vidx = identity if absent); `ref` is [Q, .]
                 (broadcast over b) or [B, Q, .]

mdqe_sample_levels_mean_f32 is grid_sample(bilinear, padding_mode=border, align_corners=False) on every level, averaged:
(X, Y) = (x W - 0.5, y H - 0.5) clamped to [0, W - 1] x [0, H - 1], then the same interpolation (every corner exists), mean over levels.

WHY A FLOAT64 BOUND EXISTS.  S_t is piecewise bilinear in (X, Y) and CONTINUOUS everywhere -- also across the cell borders, where
floor() jumps (the weight of the corners that change is zero there), and at X = -1, X = W, Y = -1, Y = H, where the kernels' `inside`
test flips (all four weights of the existing corners vanish there).  So a location that fp32 rounds into the neighbouring cell, or
to the other side of the `inside` test, changes the sample by at most (Lipschitz constant) x (location error), and the fp32 result
can be held to the float64 one element by element.  The border-clamped form is continuous for the same reason (clamping is).

THE BOUND, term by term (fused_ref_bound, native_ref_bound, slm_ref_bound; everything evaluated in float64 on the fp32 inputs).  Write
A_i = sum_g sum_corners (bilinear weight) |v_corner| for the absolute sum behind sample i; |S| <= A.

  softmax weight   _attn_norm_ref's model: a computed weight is w_i (1 + e_i) with |e_i| <= E_i = 2 U |t_i - max| + EXP_REL (the
                   subtraction's rounding scaled by the exponential, and the device exponential: EXP_REL = 4 U, ASSUMED there, for
                   the reasons written there; the maximum is taken first, so no rescaling: R = 0), which moves the output by at
                   most sum_i w_i (E_i + Ebar) A_i with Ebar = sum_i w_i E_i; the sum of the exponentials and the division add
                   (L P + 2) U sum_i w_i A_i.  Native op: the weights are inputs, this term is zero.
  location         in normalised units.  mode 0: off / 8 is exact (a power of two), the addition rounds once: d = U |x|.
                   mode 1: 8 wh and the clamp are exact (the clamp selects one of its fp32 arguments), grid * 0.5 is exact,
                   (grid * 0.5) * wh rounds once, the sum with the clamped delta once, / 8 is exact, the addition to ref_xy once:
                   d = (U |grid * 0.5 * wh| + U |grid * 0.5 * wh + clamp|) / 8 + U |x|.  Native op: d = 0.
                   Carried into pixels: dX = W d + U |x W| + U |x W - 0.5| (the product and the subtraction); the same in y.
                   (A compiler that contracts any of these into an fma rounds less often, never more.)
  sampling         |S(X', Y') - S(X, Y)| <= Lx dX + Ly dY with Lx (Ly) the largest |difference| of horizontally (vertically)
                   adjacent values in the zero-padded 4 x 4 corner neighbourhood rows floor(Y) - 1 .. floor(Y) + 2, columns
                   floor(X) - 1 .. floor(X) + 2: the cell of the float64 location and every cell next to it, since the fp32
                   location (dX, dY far below one pixel) may fall in the next cell.  Weighted: sum_g sum_i w_i (Lx dX + Ly dY).
                   A sample more than a pixel outside its map has an all-zero neighbourhood: it must contribute EXACTLY zero.
  interpolation    lh = Y' - floor(Y') is exact relative to the fp32 location; 1 - lh rounds once, a corner weight is a product of
                   two such factors (one rounding) times the attention weight (one more): 3 U on each weight; then 4 L P G
                   multiply-adds in fp32, each term passing its own product rounding and at most 4 L P G - 1 additions:
                   (4 L P G + 4) U sum_i w_i A_i.
  scale            the final product: U |out|.

    bound = |scale| * 1.01 * (softmax + sampling + interpolation) + U |out| + FLUSH

1.01 stands for second-order terms (every first-order term is below 1e-3 relative) and FLUSH = 1e-35 for weights that fp32 flushes
to zero where float64 does not.  The bound is set from the algorithm alone; no kernel output was read while writing it.
sample_levels_mean: the same with dX = 4 U (|x| W + 1) (2x, -1, +1, * W, -1, * 0.5: four roundings at most on a quantity below
|x| W + 1; the clamp is 1-Lipschitz), replicate padding in the neighbourhood, 3 U on each corner weight, 4 n multiply-adds and the
division by n: (4 n + 5) U mean_l A_l.

INPUT CATEGORIES, counted on the float64 locations per (sample, level) look-up (`categories`): `interior` (all four corners inside),
`edge` (off one edge: TWO corners outside), `corner` (off a corner of the map: THREE corners outside, one inside), `outside` (no
corner inside: exactly zero), `lattice` (X or Y an exact integer: the offsets are exact eighths of dyadic references), and in mode 1
`clamp_x`, `clamp_y` (|delta| > 8 w or 8 h) and `unclamped`.  A bilinear sample cannot have exactly ONE corner outside its map (a
column or a row of corners leaves together), so the counts are two and three.
"""
import math

import torch

from _attn_norm_ref import EXP_REL, FLUSH, worst_ratio  # noqa: F401  (re-exported)
from _gemm_ref import U, check_within, within  # noqa: F401  (re-exported)

_cache = {}
CATEGORIES0 = ("interior", "edge", "corner", "outside", "lattice")
CATEGORIES1 = CATEGORIES0 + ("clamp_x", "clamp_y", "unclamped")
MIN_SHARE = 0.05


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 5) * 6007 ** (i % 3) * int(v) for i, v in enumerate(key)) % (2 ** 31))


def contiguous_starts(shapes, first=0):
    s = [first]
    for h, w in shapes[:-1]:
        s.append(s[-1] + h * w)
    return s


# ---- the sampling core: sum_g sum_i w_i S(x_i, y_i), in any dtype, with the seeded mistakes -----------------------------------------
def _corner(value3, rows, valid, mcol):
    """value3 [R, M, D]; rows, valid [B, Q, M, LP] -> [B, Q, M, LP, D] (zero where not valid)."""
    v = value3[rows.clamp(0, value3.shape[0] - 1), mcol]
    return v * valid.unsqueeze(-1).to(v.dtype)


def sample_sum(value3, base, loc, w, levels, G, L, P, dtype=torch.float64, mistake=None, pad="zeros", dloc=None, detail=False):
    """acc [B, Q, M, D] = sum_g sum_i w_i S_{g L + i / P}(loc_i) on value3 [R, M, D], element b's block starting at row base[b].
    loc [B, Q, M, LP, 2], w [B, Q, M, LP] (already `dtype`).  detail (float64): also (A, LOC) of the module docstring -- the weighted
    absolute sum and the weighted sampling term, [B, Q, M, D] -- and the per-look-up facts [G, B, Q, M, LP] for the categories."""
    Hs, Ws, Ss = levels
    B, Q, M, LP, _ = loc.shape
    mcol = torch.arange(M).view(1, 1, M, 1).expand(B, Q, M, LP)
    brow = torch.as_tensor(base, dtype=torch.long).view(B, 1, 1, 1)
    i = torch.arange(LP)
    lev = (i % L) if mistake == "level_mod" else (i // P)
    acc = torch.zeros(B, Q, M, value3.shape[-1], dtype=dtype)
    A = torch.zeros_like(acc)
    LOC = torch.zeros_like(acc)
    facts = []
    for g in range(G):
        if mistake == "drop_group" and g == G - 1:
            continue
        t = g * L + lev
        Hi, Wi = torch.tensor(Hs)[t], torch.tensor(Ws)[t]
        St = torch.tensor(Ss)[t] + (1 if mistake == "start_off1" else 0) * (t == t.max()).long()
        H, W = Hi.to(dtype), Wi.to(dtype)
        lx, ly = loc[..., 0], loc[..., 1]
        half = 0.0 if mistake == "no_half" else 0.5
        if mistake == "swap_WH":
            X, Y = lx * H - half, ly * W - half
        elif mistake == "align_corners":
            X, Y = lx * (W - 1), ly * (H - 1)
        else:
            X, Y = lx * W - half, ly * H - half
        if pad == "border":
            X, Y = torch.minimum(torch.maximum(X, torch.zeros_like(X)), W - 1), torch.minimum(torch.maximum(Y, torch.zeros_like(Y)), H - 1)
        x0, y0 = torch.floor(X), torch.floor(Y)
        fx, fy = X - x0, Y - y0
        x0, y0 = x0.long(), y0.long()

        def fetch(dy, dx):
            yy, xx = y0 + dy, x0 + dx
            if pad == "border":
                yy, xx = torch.minimum(yy.clamp_min(0), Hi - 1), torch.minimum(xx.clamp_min(0), Wi - 1)
                ok = torch.ones_like(yy, dtype=torch.bool)
            else:
                ok = (yy >= 0) & (yy < Hi) & (xx >= 0) & (xx < Wi)
            return _corner(value3, brow + St + yy * Wi + xx, ok, mcol), ok

        wy, wx = (1 - fy, fy), (1 - fx, fx)
        s = torch.zeros_like(acc).unsqueeze(3).expand(B, Q, M, LP, acc.shape[-1]).clone()
        sa = torch.zeros_like(s)
        nout = torch.zeros(B, Q, M, LP, dtype=torch.long)
        for dy in (0, 1):
            for dx in (0, 1):
                v, ok = fetch(dy, dx)
                cw = (wy[dx] * wx[dy]) if (mistake == "swap_corners" and dy != dx) else wy[dy] * wx[dx]
                s = s + cw.unsqueeze(-1) * v
                if detail:
                    sa = sa + cw.unsqueeze(-1) * v.abs()
                    nout += (~ok).long()
        acc = acc + (w.unsqueeze(-1) * s).sum(3)
        if detail:
            A = A + (w.unsqueeze(-1) * sa).sum(3)
            facts.append(dict(nout=nout, lattice=((fx == 0) | (fy == 0)) & (nout < 4)))
        if detail is True:                        # (detail = "abs": the absolute sum only)
            # Lipschitz constants over the 4 x 4 neighbourhood, row by row
            Lx = torch.zeros_like(s)
            Ly = torch.zeros_like(s)
            prev = None
            for dy in (-1, 0, 1, 2):
                row = [fetch(dy, dx)[0] for dx in (-1, 0, 1, 2)]
                for a, b_ in zip(row[:-1], row[1:]):
                    Lx = torch.maximum(Lx, (b_ - a).abs())
                if prev is not None:
                    for a, b_ in zip(prev, row):
                        Ly = torch.maximum(Ly, (b_ - a).abs())
                prev = row
            d = dloc if dloc is not None else torch.zeros_like(loc)
            if pad == "border":
                dX, dY = 4 * U * (lx.abs() * W + 1), 4 * U * (ly.abs() * H + 1)
            else:
                dX = W * d[..., 0] + U * (lx * W).abs() + U * (lx * W - 0.5).abs()
                dY = H * d[..., 1] + U * (ly * H).abs() + U * (ly * H - 0.5).abs()
            LOC = LOC + (w.unsqueeze(-1) * (Lx * dX.unsqueeze(-1) + Ly * dY.unsqueeze(-1))).sum(3)
    if detail:
        return acc, A, LOC, facts
    return acc


# ---- the fused op ----------------------------------------------------------------------------------------------------------------------
def fused_locations(c, dtype, mistake=None):
    """(loc [B, Q, M, LP, 2], dloc, clamped [B, Q, M, LP, 2] or None) of a fused case."""
    B, Q, M, L, P = c["B"], c["Q"], c["M"], c["L"], c["P"]
    LP = L * P
    offs = c["offs"].to(dtype).view(B, Q, M, LP, 2)
    ref = c["ref"].to(dtype)
    if ref.dim() == 3 and mistake == "ref_broadcast":
        ref = ref[0]
    r = (ref[None].expand(B, Q, -1) if ref.dim() == 2 else ref).view(B, Q, 1, 1, -1)
    rxy = r[..., :2]
    if mistake == "swap_xy":
        offs = offs.flip(-1)
    div = 1.0 if mistake == "no_div8" else 8.0
    if c["mode"] == 0:
        loc = rxy + offs / div
        return loc, U * loc.abs(), None
    wh = r[..., 2:4]
    gr = c["grid"].to(dtype).view(1, 1, M, LP, 2)
    gterm = gr * (1.0 if mistake == "grid_full" else 0.5) * wh
    lim = 8 * wh
    clamp = lambda v: torch.minimum(torch.maximum(v, -lim), lim)
    if mistake == "clamp_after":
        o = clamp(gterm + offs)
    elif mistake == "no_clamp":
        o = gterm + offs
    else:
        o = gterm + clamp(offs)
    loc = rxy + o / div
    dloc = (U * gterm.abs() + U * o.abs()) / 8 + U * loc.abs()
    return loc, dloc, offs.abs() > lim


def fused_weights(c, dtype, mistake=None):
    B, Q, M, L, P = c["B"], c["Q"], c["M"], c["L"], c["P"]
    t = c["logits"].to(dtype).view(B, Q, M, L * P)
    if mistake == "softmax_P":
        return torch.softmax(t.view(B, Q, M, L, P), -1).reshape(B, Q, M, L * P)
    return torch.softmax(t, -1)


def _value3(c, dtype):
    return c["value"].to(dtype).view(c["value"].shape[0], c["M"], c["D"])


def _base(c, mistake=None):
    B = c["B"]
    idx = list(range(B)) if (c.get("vidx") is None or mistake == "no_vidx") else c["vidx"]
    return [int(i) * c["v_brows"] for i in idx]


def fused_eval(c, dtype=torch.float64, mistake=None):
    """The fused op's formula in `dtype` -> [B * Q, M * D]."""
    loc, _, _ = fused_locations(c, dtype, mistake)
    acc = sample_sum(_value3(c, dtype), _base(c, mistake), loc, fused_weights(c, dtype, mistake), c["levels"], c["G"], c["L"], c["P"], dtype, mistake)
    out = acc if mistake == "no_scale" else acc * c["scale"]
    return out.reshape(c["B"] * c["Q"], c["M"] * c["D"])


def fused_ref_bound(c):
    """(ref, bound, category counts) of a fused case, float64."""
    B, Q, M, L, P, G = c["B"], c["Q"], c["M"], c["L"], c["P"], c["G"]
    LP = L * P
    loc, dloc, clamped = fused_locations(c, torch.float64)
    w = fused_weights(c, torch.float64)
    acc, A, LOC, facts = sample_sum(_value3(c, torch.float64), _base(c), loc, w, c["levels"], G, L, P, torch.float64, dloc=dloc, detail=True)
    # the softmax term needs sum_i w_i E_i A_i with E per sample: one more pass with the weights w_i (E_i + Ebar)
    t = c["logits"].double().view(B, Q, M, LP)
    E = 2 * U * (t.max(-1, keepdim=True).values - t) + EXP_REL
    ebar = (w * E).sum(-1, keepdim=True)
    _, soft, _, _ = sample_sum(_value3(c, torch.float64), _base(c), loc, w * (E + ebar), c["levels"], G, L, P, torch.float64, detail="abs")
    soft = soft + (LP + 2) * U * A
    interp = (4 * LP * G + 4) * U * A
    out = acc * c["scale"]
    bound = abs(c["scale"]) * 1.01 * (soft + LOC + interp) + U * out.abs() + FLUSH
    return out.reshape(B * Q, M * c["D"]), bound.reshape(B * Q, M * c["D"]), categories(facts, clamped)


def categories(facts, clamped=None):
    """Counts per category over the (sample, level) look-ups; `n` is their number."""
    nout = torch.stack([f["nout"] for f in facts])
    lat = torch.stack([f["lattice"] for f in facts])
    cnt = dict(n=nout.numel(), interior=int(((nout == 0) & ~lat).sum()), edge=int((nout == 2).sum()), corner=int((nout == 3).sum()),
               outside=int((nout == 4).sum()), lattice=int(lat.sum()))
    if clamped is not None:
        k = len(facts)
        cnt.update(clamp_x=int(clamped[..., 0].sum()) * k, clamp_y=int(clamped[..., 1].sum()) * k, unclamped=int((~clamped.any(-1)).sum()) * k)
    return cnt


# ---- the native op -----------------------------------------------------------------------------------------------------------------------
def native_eval(c, dtype=torch.float64, mistake=None):
    """value [B, S, M, D], loc [B, Q, M, L, P, 2], attn [B, Q, M, L, P] -> [B, Q, M * D]."""
    B, Q, M, L, P, S = c["B"], c["Q"], c["M"], c["L"], c["P"], c["S"]
    loc = c["loc"].to(dtype).view(B, Q, M, L * P, 2)
    if mistake == "swap_xy":
        loc = loc.flip(-1)
    acc = sample_sum(c["value"].to(dtype).view(B * S, M, c["D"]), [b * S for b in range(B)], loc, c["attn"].to(dtype).view(B, Q, M, L * P),
                     c["levels"], c["G"], L, P, dtype, mistake)
    return (acc if mistake == "no_scale" else acc * c["scale"]).reshape(B, Q, M * c["D"])


def native_ref_bound(c):
    B, Q, M, L, P, S, G = c["B"], c["Q"], c["M"], c["L"], c["P"], c["S"], c["G"]
    loc = c["loc"].double().view(B, Q, M, L * P, 2)
    a = c["attn"].double().view(B, Q, M, L * P)
    v3 = c["value"].double().view(B * S, M, c["D"])
    base = [b * S for b in range(B)]
    acc, _, _, facts = sample_sum(v3, base, loc, a, c["levels"], G, L, P, torch.float64, detail="abs")
    _, A, LOC, _ = sample_sum(v3, base, loc, a.abs(), c["levels"], G, L, P, torch.float64, detail=True)       # (attn may be negative)
    out = acc * c["scale"]
    bound = abs(c["scale"]) * 1.01 * (LOC + (4 * L * P * G + 4) * U * A) + U * out.abs() + FLUSH
    return out.reshape(B, Q, -1), bound.reshape(B, Q, -1), categories(facts)


# ---- sample_levels_mean --------------------------------------------------------------------------------------------------------------------
def slm_eval(c, dtype=torch.float64, mistake=None):
    """tokens [NI, N, C], coords [NI, Q, 2], shapes, starts -> [NI, Q, C]: border-clamped bilinear samples, mean over the levels."""
    NI, N, C = c["tokens"].shape
    Q, n = c["coords"].shape[1], len(c["shapes"])
    levels = ([s[0] for s in c["shapes"]], [s[1] for s in c["shapes"]], list(c["starts"]))
    loc = c["coords"].to(dtype).view(NI, Q, 1, 1, 2).expand(NI, Q, 1, n, 2)
    w = torch.full((NI, Q, 1, n), 1.0, dtype=dtype)
    pad = "zeros" if mistake == "zero_pad" else "border"
    acc = sample_sum(c["tokens"].to(dtype).view(NI * N, 1, C), [b * N for b in range(NI)], loc, w, levels, 1, n, 1, dtype,
                     mistake if mistake != "zero_pad" else None, pad=pad)
    return (acc / n).reshape(NI, Q, C)


def slm_ref_bound(c):
    NI, N, C = c["tokens"].shape
    Q, n = c["coords"].shape[1], len(c["shapes"])
    levels = ([s[0] for s in c["shapes"]], [s[1] for s in c["shapes"]], list(c["starts"]))
    loc = c["coords"].double().view(NI, Q, 1, 1, 2).expand(NI, Q, 1, n, 2)
    w = torch.ones(NI, Q, 1, n, dtype=torch.float64)
    acc, A, LOC, _ = sample_sum(c["tokens"].double().view(NI * N, 1, C), [b * N for b in range(NI)], loc, w, levels, 1, n, 1, torch.float64,
                                pad="border", detail=True)
    out = acc / n
    bound = 1.01 * (LOC + (4 * n + 5) * U * A) / n + FLUSH
    return out.reshape(NI, Q, C), bound.reshape(NI, Q, C)


# ---- the dispatch restated ---------------------------------------------------------------------------------------------------------------
DEFAULT_SWITCHES = dict(variant=-1, patch=0, stage_kb=0, dec_stage_kb=0, tp_staged=1, dec_staged=1, dec_wpe8=0, xcd_order=1, op_staged=1)


def switches(**kw):
    s = dict(DEFAULT_SWITCHES)
    s.update(kw)
    return s


def desc_bytes(nt):
    """LDS of the sample descriptors: per wave 8 groups x (8 + 1) samples x 4 corners x (offset + weight) x 4 bytes."""
    return (nt // 64) * 8 * (8 + 1) * 4 * 2 * 4


def threads_for(Q):
    """(runs, chunk, threads) of the decoder and temporal forms: even runs of at most 128 queries, threads to match."""
    runs = (Q + 127) // 128
    chunk = (Q + runs - 1) // runs
    return runs, chunk, 512 if chunk <= 64 else 832 if chunk <= 104 else 1024


def staged_levels(hw, D, desc, budget):
    """(LS, px): the coarsest levels of hw = [H * W per level] that fit `budget` bytes beside the descriptors; level 0 never."""
    LS, px = len(hw), 0
    while LS > 1 and (px + hw[LS - 1] + 1) * D * 4 + desc <= budget:
        LS -= 1
        px += hw[LS]
    return LS, px


def chunk_for(px, D):
    staged = (px + 1) * D * 4
    return 128 if staged < 45 * 1024 else 256 if staged < 80 * 1024 else 512


def two_blocks_fit(smem):
    return 2 * smem + 1024 <= 160 * 1024


def msda_fused_branch(s, sw=None, contiguity_rule=True):
    """What mdqe_msda_fused_f32 launches for shape s (dict: B, Q, M, D, G, L, P, mode, ref_dim, vidx (bool), levels) under the debug
    switches sw: dict(inst = the kernel instantiation's name, LS, chunk, threads, two_blocks, patch), or inst = "EINVAL".
    contiguity_rule=False restates the dispatcher BEFORE the staged branch required contiguous ascending levels [LS, L)."""
    sw = sw or DEFAULT_SWITCHES
    B, Q, M, D, G, L, P, mode, ref_dim = (s[k] for k in ("B", "Q", "M", "D", "G", "L", "P", "mode", "ref_dim"))
    H, W, S = s["levels"]
    variant = sw["variant"]
    stage_kb = sw["stage_kb"] if sw["stage_kb"] > 0 else 150
    dec_kb = sw["stage_kb"] if sw["stage_kb"] > 0 else 72
    if sw["dec_stage_kb"] > 0:
        dec_kb = sw["dec_stage_kb"]
    res = dict(inst="EINVAL", LS=None, chunk=None, threads=256, two_blocks=False, patch=False)
    if not (G * L <= 16 and D % 4 == 0 and (mode == 0 or ref_dim == 4)):
        return res
    if B * Q == 0:
        return dict(res, inst="none")
    span = max(S[i] + H[i] * W[i] for i in range(G * L))          # (the dispatcher multiplies by the value pitch; M * D at the least)
    if D in (32, 24) and L * P == 16 and (span * M * D + M * D) * 4 < 0xF0000000:
        ntok = sum(H[l] * W[l] for l in range(L))
        var = variant if variant >= 0 else ((1 | 8) if mode == 0 else 8)
        enc_form = mode == 0 and ntok == Q and not s["vidx"] and ref_dim == 2
        dec_form = mode == 1 and ref_dim == 4 and bool(sw["dec_staged"]) and (D == 32 or stage_kb != 150)
        if (var & 8) and G == 1 and L == 4 and P == 4 and (enc_form or dec_form):
            nt = 512 if (variant >= 0 and (variant & 128)) else 1024
            chunk = 0
            if dec_form:
                _, chunk, nt = threads_for(Q)
            desc = desc_bytes(nt)
            budget = (dec_kb if dec_form and stage_kb > dec_kb else stage_kb) * 1024
            LS, px = staged_levels([H[l] * W[l] for l in range(L)], D, desc, budget)
            contig = all(S[l + 1] == S[l] + H[l] * W[l] for l in range(LS, L - 1))
            if LS < L and (contig or not contiguity_rule):
                smem = (px + 1) * D * 4 + desc
                if chunk == 0:
                    chunk = chunk_for(px, D)
                if variant >= 0 and ((variant >> 4) & 7):
                    chunk = 32 << (((variant >> 4) & 7) - 1)
                patch = enc_form and nt == 1024 and chunk % 128 == 0 and not (variant >= 0 and (variant & 2048)) and bool(sw["patch"])
                wpe8 = not (variant >= 0 and (variant & 256)) and two_blocks_fit(smem)
                two = nt == 1024 and wpe8
                lsc = LS if (variant >= 0 and (variant & 1024) and LS in (2, 3)) else -1
                if lsc < 0:
                    build = "two blocks" if two else "8 waves" if (nt == 832 and sw["dec_wpe8"] and D == 32) else "natural"
                else:
                    build = f"level {lsc} at compile time"
                return dict(inst=f"fused v3 D={D} threads={nt} {build}", LS=LS, chunk=chunk, threads=nt, two_blocks=two, patch=patch)
        if (var & 8) and sw["tp_staged"] and mode == 1 and ref_dim == 4 and G == 4 and L == 4 and P == 4 and s["vidx"] and Q <= 4096:
            ok = True
            for g in range(G):
                for f in range(L):
                    ok = ok and H[g * L + f] == H[g * L] and W[g * L + f] == W[g * L]
                    if g + 1 < G:
                        ok = ok and S[(g + 1) * L + f] == S[g * L + f] + H[g * L] * W[g * L]
            _, chunk, nt = threads_for(Q)
            desc = desc_bytes(nt)
            LS, px = staged_levels([H[g * L] * W[g * L] for g in range(G)], D, desc, 72 * 1024) if ok else (G, 0)
            if ok and LS < G:
                lsc = LS if (variant >= 0 and (variant & 1024) and LS in (2, 3)) else -1
                if nt == 832 and sw["dec_wpe8"] in (1, 2) and D == 32 and lsc < 0:
                    build = "8 waves" if sw["dec_wpe8"] == 1 else "7 waves"
                else:
                    build = "natural" if lsc < 0 else f"level {lsc} at compile time"
                return dict(inst=f"fused temporal D={D} threads={nt} {build}", LS=LS, chunk=chunk, threads=nt, two_blocks=False, patch=False)
        mp = var & 3
        if mp == 2 and not (mode == 0 and G == 1 and ntok == Q):
            mp = 1 if mode == 0 else 0
        mp = min(mp, 2)                           # (3 takes the launch macro's `else`: the map-2 kernel)
        if (L, P) in ((4, 4), (2, 8)):
            return dict(res, inst=f"fused v2 L{L}P{P} map={mp} waves hint={8 if var & 4 else 1} D={D}")
    if P == 4 and 1 <= L <= 4:
        return dict(res, inst=f"fused v1 L={L}")
    return res


def msda_native_branch(s, sw=None):
    """What mdqe_msda_forward_grouped_f32 launches: s = dict(B, S, M, D, G, L, Q, P, levels, value_off, out_off, la_off) with the
    offsets (in floats, from a 16-byte-aligned base) of value / out / loc and attn."""
    sw = sw or DEFAULT_SWITCHES
    B, S, M, D, G, L, Q, P = (s[k] for k in ("B", "S", "M", "D", "G", "L", "Q", "P"))
    res = dict(inst="none", LS=None, chunk=None, budget=None)
    if B * Q == 0:
        return res
    al16 = s.get("value_off", 0) % 4 == 0 and s.get("out_off", 0) % 4 == 0
    al8 = s.get("value_off", 0) % 2 == 0 and s.get("out_off", 0) % 2 == 0
    vbytes = B * S * M * D * 4
    if D == 32 and L * P == 16 and L in (4, 2) and G * L <= 16 and al16 and 0 < vbytes < 0xF0000000 and s.get("la_off", 0) % 4 == 0:
        if sw["op_staged"] and G == 1 and L == 4 and S >= 64:
            budget = min(S // 16 + 8, 960)
            H, W, _ = s["levels"]
            LS, px = L, 0
            while LS > 0 and H[LS - 1] * W[LS - 1] > 0 and px + H[LS - 1] * W[LS - 1] <= budget:
                LS -= 1
                px += H[LS] * W[LS]
            return dict(inst="native v3", LS=LS, chunk=chunk_for(budget, 32), budget=budget)
        return dict(res, inst=f"native v2 L{L}P{P}")
    vec = 4 if (D % 4 == 0 and al16) else 2 if (D % 2 == 0 and al8) else 1
    return dict(res, inst=f"native v1 VEC={vec} {'L4P4' if (L, P) == (4, 4) else 'runtime L, P'}")


FUSED_INSTANCES = (
    [f"fused v1 L={L}" for L in (1, 2, 3, 4)]
    + [f"fused v2 {lp} map={mp} waves hint={wp} D={D}" for lp in ("L4P4", "L2P8") for mp in (0, 1, 2) for wp in (1, 8) for D in (32, 24)]
    + [f"fused v3 D={D} threads={nt} {b}" for D in (32, 24) for nt in (512, 832, 1024)
       for b in ("natural", "level 2 at compile time", "level 3 at compile time")]
    + ["fused v3 D=32 threads=1024 two blocks", "fused v3 D=24 threads=1024 two blocks", "fused v3 D=32 threads=832 8 waves"]
    + [f"fused temporal D={D} threads={nt} {b}" for D in (32, 24) for nt in (512, 832, 1024)
       for b in ("natural", "level 2 at compile time", "level 3 at compile time")]
    + ["fused temporal D=32 threads=832 8 waves", "fused temporal D=32 threads=832 7 waves"])
NATIVE_INSTANCES = ([f"native v1 VEC={v} {f}" for v in (4, 2, 1) for f in ("L4P4", "runtime L, P")]
                    + ["native v2 L4P4", "native v2 L2P8", "native v3"])


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def _lattice_candidates(n):
    """Dyadic x = k / 64 in [-0.25, 1.25] whose pixel coordinate x n - 0.5 is an exact integer in [-1, n]."""
    return [k / 64.0 for k in range(-16, 81) if (k * n) % 64 == 32 and -1 <= k * n / 64.0 - 0.5 <= n]


def _axis_target(g, n, kind, shape):
    """Pixel coordinates on an axis of n pixels: kind 0 inside [0, n - 1], 1 within a pixel outside an end, 2 further out, 3 anywhere."""
    u = torch.rand(shape, generator=g)
    side = torch.randint(0, 2, shape, generator=g).bool()
    inside = u * (n - 1)
    near = torch.where(side, -0.95 + 0.9 * u, n - 1 + 0.05 + 0.9 * u)
    far = torch.where(side, -3.0 + 1.9 * u, n + 0.1 + 1.9 * u)
    anyw = -1 + u * (n + 1)
    return torch.where(kind == 0, inside, torch.where(kind == 1, near, torch.where(kind == 2, far, anyw)))


def _targets(g, B, Q, M, L, P, G, levels, dyadic_q):
    """Normalised target locations [B, Q, M, LP, 2] for a mix of categories on the level table; dyadic_q [B, Q] marks the queries whose
    reference point is dyadic: their `lattice` samples get dyadic targets (others fall back to interior)."""
    Hs, Ws, _ = levels
    LP = L * P
    shape = (B, Q, M)
    out = torch.zeros(B, Q, M, LP, 2)
    for i in range(LP):
        gsel = int(torch.randint(0, G, (1,), generator=g))
        t = gsel * L + i // P
        H, W = Hs[t], Ws[t]
        cat = torch.multinomial(torch.tensor([0.30, 0.20, 0.17, 0.13, 0.20]), B * Q * M, replacement=True, generator=g).view(shape)
        axis = torch.randint(0, 2, shape, generator=g)                                   # which axis leaves the map (edge / outside)
        kx = torch.where(cat == 1, (axis == 0).long(), torch.where(cat == 2, torch.ones_like(cat), torch.where(cat == 3, torch.where(axis == 0, 2, 3), torch.zeros_like(cat))))
        ky = torch.where(cat == 1, (axis == 1).long(), torch.where(cat == 2, torch.ones_like(cat), torch.where(cat == 3, torch.where(axis == 1, 2, 3), torch.zeros_like(cat))))
        tx = (_axis_target(g, W, kx, shape) + 0.5) / W
        ty = (_axis_target(g, H, ky, shape) + 0.5) / H
        lat = (cat == 4) & dyadic_q.view(B, Q, 1)
        for n, tt in ((W, tx), (H, ty)):
            cand = _lattice_candidates(n)
            if cand:
                pick = torch.tensor(cand)[torch.randint(0, len(cand), shape, generator=g)]
                tt[lat] = pick[lat]
        out[..., i, 0], out[..., i, 1] = tx, ty
    return out


def _ref_points(g, B, Q, batched):
    """Reference points [B or 1, Q, 2] and the mask of the dyadic ones: a third dyadic (k / 64), a third on or near the borders of the
    image, the rest anywhere inside."""
    nb = B if batched else 1
    kind = torch.randint(0, 3, (nb, Q), generator=g)
    dy = torch.randint(0, 65, (nb, Q, 2), generator=g).float() / 64.0
    u = torch.rand(nb, Q, 2, generator=g)
    border = torch.where(torch.rand(nb, Q, 2, generator=g) < 0.7, torch.where(u < 0.5, -0.05 + 0.2 * u, 0.95 + 0.2 * (u - 0.5)), u)
    xy = torch.where((kind == 0)[..., None], dy, torch.where((kind == 1)[..., None], border, 0.1 + 0.8 * u))
    return xy, (kind == 0)


def fused_inputs(s, seed):
    """The tensors of a fused case from its shape dict s (adds value, offs, logits, ref, grid, vidx list, v_brows, value_rows)."""
    B, Q, M, D, G, L, P, mode = (s[k] for k in ("B", "Q", "M", "D", "G", "L", "P", "mode"))
    LP = L * P
    g = _gen(seed, B, Q, M, D, G * 16 + L, mode)
    Hs, Ws, Ss = s["levels"]
    span = max(Ss[i] + Hs[i] * Ws[i] for i in range(G * L))
    c = dict(s)
    if s["vidx"]:
        NF = max(B, 3) + 2
        vidx = [(7 * b + 3) % NF for b in range(B)]                    # neither the identity nor sorted
        v_brows = s.get("v_brows") or span
        rows = max(vidx) * v_brows + span
        c["vidx"] = vidx
    else:
        v_brows = s.get("v_brows") or span
        rows = (B - 1) * v_brows + span
        c["vidx"] = None
    c["v_brows"], c["value_rows"] = v_brows, rows
    c["value"] = torch.randn(rows, M * D, generator=g)
    batched = bool(s.get("ref_batched"))
    xy, dyadic = _ref_points(g, B, Q, batched)
    dq = dyadic.expand(B, Q) if not batched else dyadic
    tgt = _targets(g, B, Q, M, L, P, G, s["levels"], dq)
    rxy = xy.view(-1, Q, 1, 1, 2)
    lscale = s.get("logit_scale", 1.0)
    c["logits"] = (torch.randn(B * Q, M * LP, generator=g) * lscale)
    if mode == 0:
        offs = 8.0 * (tgt - rxy)
        # a share of free offsets: whatever they hit
        free = torch.rand(B, Q, M, LP, 1, generator=g) < 0.15
        offs = torch.where(free, torch.randn(B, Q, M, LP, 2, generator=g) * 2.0, offs)
        ref = xy
        if s["ref_dim"] == 4:
            ref = torch.cat([xy, torch.rand(xy.shape, generator=g)], -1)
        c["grid"] = None
    else:
        nb = xy.shape[0]
        wh = 0.05 + 0.45 * torch.rand(nb, Q, 2, generator=g)
        dyw = torch.tensor([[0.25, 0.5], [0.5, 0.125], [0.125, 0.25], [0.5, 0.25]])[torch.randint(0, 4, (nb, Q), generator=g)]
        wh = torch.where(dyadic[..., None], dyw, wh)
        grid = torch.randn(M, LP, 2, generator=g)
        pmask = (torch.arange(LP) % P < 2).view(1, LP, 1)
        grid = torch.where(pmask, torch.round(grid * 4) / 4, grid)                      # dyadic at the points 0 and 1 of every level
        whb = wh.view(-1, Q, 1, 1, 2)
        gterm = grid.view(1, 1, M, LP, 2) * 0.5 * whb
        delta = 8.0 * (tgt - rxy) - gterm
        free = torch.rand(B, Q, M, LP, 1, generator=g) < 0.45
        small = (torch.rand(B, Q, M, LP, 2, generator=g) * 1.8 - 0.9) * 8.0 * whb
        offs = torch.where(free, small, delta)
        # lattice samples of mode 1: at the dyadic queries, the points 0 and 1 of a level go to the lattice position nearest the
        # reference point (so that the delta stays inside its clamp where the box allows): every term is dyadic, fp32 is exact
        Hs, Ws, _ = s["levels"]
        near = rxy.expand(-1, Q, M, LP, 2).clone()
        for i in range(LP):
            for ax, n in ((0, Ws[i // P]), (1, Hs[i // P])):
                cand = torch.tensor(_lattice_candidates(n) or [0.5])
                near[:, :, :, i, ax] = cand[(cand.view(1, 1, -1) - xy[..., ax, None]).abs().argmin(-1)][:, :, None]
        lat = (dyadic.view(-1, Q, 1, 1, 1) & pmask.view(1, 1, 1, LP, 1)).expand(B, Q, M, LP, 1) & (torch.rand(B, Q, M, 1, 1, generator=g) < 0.8)
        offs = torch.where(lat, 8.0 * (near - rxy) - gterm, offs)
        ref = torch.cat([xy, wh], -1)
        c["grid"] = grid.reshape(-1).contiguous()
    c["offs"] = offs.reshape(B * Q, M * LP * 2).float().contiguous()
    c["ref"] = (ref if batched else ref[0]).float().contiguous()
    return c


def fused_case(name):
    """The inputs, float64 reference, bound and category counts of a fused case, computed once (callers must not modify them)."""
    if name not in _cache:
        s = FUSED_SHAPES[name]
        c = fused_inputs(s, sorted(FUSED_SHAPES).index(name))
        c["name"] = name
        c["out"], c["bound"], c["cats"] = fused_ref_bound(c)
        _cache[name] = c
    return _cache[name]


def native_case(name):
    key = "native " + name
    if key not in _cache:
        s = dict(NATIVE_SHAPES[name])
        B, S, M, D, G, L, Q, P = (s[k] for k in ("B", "S", "M", "D", "G", "L", "Q", "P"))
        g = _gen(sorted(NATIVE_SHAPES).index(name), B, S, M, D, G * 16 + L, Q)
        s["value"] = torch.randn(B, S, M, D, generator=g)
        dq = torch.rand(B, Q, generator=g) < 0.5
        s["loc"] = _targets(g, B, Q, M, L, P, G, s["levels"], dq).view(B, Q, M, L, P, 2).float().contiguous()
        lg = torch.randn(B, Q, M, L * P, generator=g) * s.get("logit_scale", 1.0)
        s["attn"] = torch.softmax(lg, -1).view(B, Q, M, L, P).contiguous()
        s["name"] = name
        s["out"], s["bound"], s["cats"] = native_ref_bound(s)
        _cache[key] = s
    return _cache[key]


def slm_case(name):
    key = "slm " + name
    if key not in _cache:
        NI, C, Q, shapes, gap = SLM_SHAPES[name]
        g = _gen(sorted(SLM_SHAPES).index(name), NI, C, Q, len(shapes))
        starts = contiguous_starts(shapes, gap)
        N = starts[-1] + shapes[-1][0] * shapes[-1][1] + gap
        coords = torch.rand(NI, Q, 2, generator=g) * 1.3 - 0.15                       # in front of, on and behind the borders
        coords[:, ::5] = torch.randint(0, 65, (NI, len(range(0, Q, 5)), 2), generator=g).float() / 64.0     # dyadic, 0 and 1 among them
        coords[:, 0] = torch.tensor([0.0, 1.0])
        c = dict(tokens=torch.randn(NI, N, C, generator=g), coords=coords.contiguous(), shapes=shapes, starts=starts, name=name)
        c["out"], c["bound"] = slm_ref_bound(c)
        _cache[key] = c
    return _cache[key]


# ---- case lists ------------------------------------------------------------------------------------------------------------------------------
def table(shapes, first=0, gap_before=None, order=None, G=1, frames=None):
    """(H, W, start) lists.  order: the order in which the levels lie in memory (default ascending); gap_before = (level, rows): a gap
    in front of that level.  frames = (list of frame indices, rows per frame): the temporal table [level g][frame f]."""
    order = order or list(range(len(shapes)))
    start, at = {}, first
    for l in order:
        if gap_before and gap_before[0] == l:
            at += gap_before[1]
        start[l] = at
        at += shapes[l][0] * shapes[l][1]
    H, W, S = [s[0] for s in shapes], [s[1] for s in shapes], [start[l] for l in range(len(shapes))]
    if frames is None:
        return H, W, S
    fr, N = frames
    return ([h for h in H for _ in fr], [w for w in W for _ in fr], [f * N + s for s in S for f in fr])


T40 = [(4, 5), (3, 4), (2, 3), (1, 2)]                                   # 40 tokens
T40B = [(4, 5), (2, 3), (3, 4), (1, 2)]                                  # no pyramid: the third level larger than the second
FINE, BLOCK = (3, 5), (16, 37)                                           # 15 tokens; 592 tokens: never fits beside the two below it
Y77, Y78 = (7, 11), (6, 13)
X210, X264, X354, X575 = (10, 21), (12, 22), (6, 59), (23, 25)


def _shape(mode, B, Q, M, D, levels, G=1, L=4, P=4, ref_dim=None, vidx=None, ref_batched=None, scale=1.0, logit_scale=1.0, v_brows=None):
    dec = mode == 1
    return dict(mode=mode, B=B, Q=Q, M=M, D=D, G=G, L=L, P=P, levels=levels, ref_dim=ref_dim or (4 if dec else 2),
                vidx=dec if vidx is None else vidx, ref_batched=dec if ref_batched is None else ref_batched, scale=scale,
                logit_scale=logit_scale, v_brows=v_brows)


def _ntok(shapes):
    return sum(h * w for h, w in shapes)


def _tp_levels(shapes, nfr=4, unlike=False):
    N = _ntok(shapes)
    H, W, S = table(shapes, frames=(list(range(nfr)), N))
    if unlike:                                                            # frame 1 carries its coarsest level transposed
        i = (len(shapes) - 1) * nfr + 1
        H[i], W[i] = W[i], H[i]
    return H, W, S


def _tp(B, Q, M, D, shapes, **kw):
    s = _shape(1, B, Q, M, D, _tp_levels(shapes, unlike=kw.pop("unlike", False)), G=4, L=4, scale=0.25, v_brows=_ntok(shapes), **kw)
    return s


FUSED_SHAPES = {}
FUSED_LAUNCHES = []                     # (case name, switches, note)


def _add(name, shape, *sws):
    FUSED_SHAPES[name] = shape
    for sw in (sws or (switches(),)):
        FUSED_LAUNCHES.append((name, sw))


V2_VARIANTS = (0, 1, 2, 4, 5, 6)
# v1: every L, head widths the cooperative kernels do not take, both modes, groups, ref_dim 4 in mode 0
_add("v1 L=4 D=16", _shape(0, 2, 37, 3, 16, table(T40)))
_add("v1 L=3 mode 1", _shape(1, 3, 21, 1, 32, table(T40[:3]), L=3, logit_scale=30.0))
_add("v1 L=2 two groups D=8", _shape(0, 1, 65, 8, 8, table([(5, 7), (3, 4), (4, 9), (2, 5)]), G=2, L=2, ref_dim=4, scale=0.5, ref_batched=True))
_add("v1 L=1 D=64", _shape(0, 2, 9, 3, 64, table([(6, 5)]), L=1))
# the encoder form on the 40-token table: default (two blocks), every v2 map and waves hint, natural / 512-thread / compile-time builds,
# forced budgets for LS = 1, 2, 3 and "nothing fits", the patch walk, the chunk sweep bits
def forced_budget(shape, LS, **sw):
    """The smallest mdqe_debug_msda_stage_kb value under which the staged form takes `shape` with its first staged level = LS."""
    for kb in range(1, 161):
        r = msda_fused_branch(shape, switches(stage_kb=kb, **sw))
        if r["inst"].startswith("fused v3") and r["LS"] == LS:
            return switches(stage_kb=kb, **sw)
    raise AssertionError(f"no budget stages levels {LS}.. of {shape}")


for D_, T_ in ((32, T40), (24, T40), (24, T40B)):                        # (D = 24: no whole-KB budget stages level 3 alone on T40)
    sh_ = _shape(0, 2, 40, 3, D_, table(T_), logit_scale=30.0 if D_ == 24 else 1.0)
    ls_ = [ls for ls in (1, 2, 3) if not (D_ == 24 and ls == (3 if T_ is T40 else 2))]
    _add(f"enc 40{'B' if T_ is T40B else ''} D={D_}", sh_,
         switches(), *[switches(variant=v) for v in V2_VARIANTS], switches(variant=8 | 256), switches(variant=8 | 128), switches(patch=1),
         switches(variant=8 | 16), switches(variant=8 | 48), switches(stage_kb=36),
         *[forced_budget(sh_, ls) for ls in ls_],
         *[forced_budget(sh_, ls, variant=8 | 1024 | extra) for ls in ls_ if ls > 1 for extra in (0, 128)])
_add("enc L2P8 D=32", _shape(0, 2, 47, 3, 32, table([(5, 7), (3, 4)]), L=2, P=8), switches(), *[switches(variant=v) for v in V2_VARIANTS])
_add("enc L2P8 D=24", _shape(0, 2, 47, 1, 24, table([(5, 7), (3, 4)]), L=2, P=8), switches(), *[switches(variant=v) for v in V2_VARIANTS])
_add("v2 two groups", _shape(0, 2, 40, 3, 32, table(T40 + T40B), G=2, scale=0.5), switches())
_add("v2 mode 0 with boxes", _shape(0, 2, 33, 3, 32, table(T40), ref_dim=4, vidx=True, ref_batched=True), switches())
# B on both sides of the XCD-aware block order, with it and without, staged and gather forms
for B_ in (1, 15, 16, 17):
    _add(f"enc 40 B={B_}", _shape(0, B_, 40, 1, 32, table(T40)), switches(), switches(xcd_order=0), switches(variant=1), switches(variant=1, xcd_order=0),
         switches(variant=0), switches(variant=2, xcd_order=0))
    _add(f"dec B={B_}", _shape(1, B_, 9, 1, 32, table(T40)), switches(), switches(dec_staged=0))
# the encoder's capacity thresholds at the default 150 KB: staged rows 347 | 348 (two blocks), 358 | 359 and 638 | 639 (chunk), 911 | 912 (LS)
for L1_, L2_, tag in (((4, 15), X210, "two blocks"), ((5, 10), (11, 21), "chunk 128|256"), ((2, 17), (17, 31), "chunk 256|512"), ((8, 12), (18, 41), "911|912")):
    for Y_ in (Y77, Y78):
        sh = [FINE, L1_, L2_, Y_]
        _add(f"enc {tag} {_ntok(sh[1:])} rows", _shape(0, 1, _ntok(sh), 1, 32, table(sh)), switches())
# the decoder's box-level form: every thread count and run split; 72 KB on both sides at every thread count; D = 24 under a forced budget
for Q_ in (1, 64, 65, 104, 105, 128, 129, 208, 209):
    _add(f"dec Q={Q_}", _shape(1, 2, Q_, 1, 32, table(T40), logit_scale=30.0 if Q_ == 65 else 1.0), switches(), switches(variant=0))
_add("dec 832 builds", _shape(1, 3, 104, 3, 32, table(T40)), switches(), switches(dec_wpe8=1), switches(dec_stage_kb=30), switches(stage_kb=31),
     switches(variant=8 | 1024, stage_kb=30), switches(variant=8 | 1024, stage_kb=31), switches(variant=8 | 256))
_add("dec 1024 natural", _shape(1, 2, 128, 1, 32, table(T40)), switches(variant=8 | 256))
for Q_, X_ in ((128, X210), (104, X264), (64, X354)):
    for Y_ in (Y77, Y78):
        sh = [FINE, BLOCK, X_, Y_]
        _add(f"dec 72 KB threads={threads_for(Q_)[2]} {_ntok(sh[2:])} rows", _shape(1, 1, Q_, 1, 32, table(sh)), switches(), switches(variant=8 | 1024))
for Q_ in (64, 104, 128):
    for T_ in (T40, T40B):
        sh_ = _shape(1, 2, Q_, 1, 24, table(T_))
        _add(f"dec D=24 Q={Q_}{' B' if T_ is T40B else ''}", sh_, switches(), switches(stage_kb=100), switches(stage_kb=100, variant=8 | 256),
             forced_budget(sh_, 3 if T_ is T40B else 2, variant=8 | 1024))
# gapped and re-ordered tables: legal for v1 / v2, never staged
_add("enc gap before level 3", _shape(0, 2, 40, 3, 32, table(T40, gap_before=(3, 5))), switches(), switches(variant=1))
_add("enc levels descending", _shape(0, 2, 40, 3, 32, table(T40, order=[3, 2, 1, 0])), switches(), switches(variant=1))
_add("enc fine level last", _shape(0, 2, 40, 3, 32, table(T40, order=[1, 2, 3, 0])), switches(), switches(variant=1))
_add("dec gap before level 2", _shape(1, 2, 70, 1, 32, table(T40, first=3, gap_before=(2, 7))), switches(), switches(variant=0))
# the temporal form
for Q_ in (1, 64, 65, 104, 105, 128, 129, 208, 209):
    _add(f"tp Q={Q_}", _tp(1, Q_, 1, 32, T40), switches())
_add("tp builds", _tp(3, 104, 3, 32, T40, logit_scale=30.0), switches(), switches(dec_wpe8=1), switches(dec_wpe8=2), switches(tp_staged=0), switches(variant=0))
for D_ in (32, 24):
    for Q_ in (64, 104, 128):
        _add(f"tp D={D_} Q={Q_} LS=2", _tp(1, Q_, 1, D_, [FINE, BLOCK, X210, Y77]), switches(), switches(variant=8 | 1024))
        _add(f"tp D={D_} Q={Q_} LS=3", _tp(1, Q_, 1, D_, [FINE, BLOCK, X575, Y77]), switches(), switches(variant=8 | 1024))
for Q_, X_ in ((128, X210), (104, X264), (64, X354)):
    _add(f"tp 72 KB threads={threads_for(Q_)[2]} {_ntok([X_, Y78])} rows", _tp(1, Q_, 1, 32, [FINE, BLOCK, X_, Y78]), switches())
    if X_ is not X210:
        _add(f"tp 72 KB threads={threads_for(Q_)[2]} {_ntok([X_, Y77])} rows", _tp(1, Q_, 1, 32, [FINE, BLOCK, X_, Y77]), switches())
_add("tp nothing fits", _tp(1, 64, 1, 32, [FINE, (2, 3), (3, 4), (12, 37)]), switches())
_add("tp unlike pyramids", _tp(2, 64, 1, 32, T40, unlike=True), switches())
_add("tp D=24 gather", _tp(2, 33, 3, 24, T40), switches(tp_staged=0), switches())
_add("tp Q=4097", _tp(1, 4097, 1, 32, T40), switches())

FUSED_REFUSED = [("L=3 P=8", dict(L=3, P=8, D=32)), ("L=2 P=8 D=16", dict(L=2, P=8, D=16)), ("L=5 P=4", dict(L=5, P=4, D=16))]

# switch settings whose launches the code comments declare bit-identical: everything but the v1 kernel and the temporal form
def same_bits_family(inst):
    return inst.startswith("fused v2") or inst.startswith("fused v3")


def _nshape(B, S, M, D, Q, shapes, G=1, L=4, P=4, value_off=0, out_off=0, la_off=0, scale=1.0, levels=None):
    lv = levels or table(shapes)
    H, W, St = lv
    assert max(St[i] + H[i] * W[i] for i in range(G * L)) <= S
    return dict(B=B, S=S, M=M, D=D, G=G, L=L, Q=Q, P=P, levels=lv, value_off=value_off, out_off=out_off, la_off=la_off, scale=scale)


PYR = [(12, 20), (6, 11), (3, 5), (2, 3)]                                 # 327 tokens
NATIVE_SHAPES = {
    "VEC=4 D=16": _nshape(2, 40, 3, 16, 37, T40),
    "VEC=4 runtime L=3 P=2": _nshape(2, 38, 3, 8, 19, T40[:3], L=3, P=2),
    "VEC=2 D=6": _nshape(2, 40, 3, 6, 21, T40, G=1),
    "VEC=2 D=6 runtime L=1 P=3": _nshape(1, 20, 3, 6, 33, T40[:1], L=1, P=3),
    "VEC=2 base at 8 bytes": _nshape(2, 40, 1, 32, 9, T40, value_off=2, out_off=2),
    "VEC=1 base at 4 bytes": _nshape(2, 40, 1, 32, 9, T40, value_off=1, out_off=1),
    "VEC=1 out at 4 bytes, runtime": _nshape(1, 38, 3, 8, 9, T40[:3], L=3, P=2, out_off=1),
    "VEC=1 D=5": _nshape(2, 40, 3, 5, 17, T40),
    "VEC=1 D=5 runtime": _nshape(1, 38, 8, 5, 17, T40[:3], L=3, P=5),
    "VEC=4 D=32 loc at 8 bytes": _nshape(2, 40, 3, 32, 9, T40, la_off=2),
    "v2 S < 64": _nshape(3, 40, 3, 32, 37, T40),
    "v2 S = 63": _nshape(1, 63, 1, 32, 5, T40),
    "v2 two groups": _nshape(2, 80, 3, 32, 37, None, G=2, scale=0.5, levels=table(T40 + T40B)),
    "v2 L2P8": _nshape(2, 47, 3, 32, 37, [(5, 7), (3, 4)], L=2, P=8),
    "v3 S = 64": _nshape(2, 64, 3, 32, 37, T40),
    "v3 all levels staged": _nshape(2, 1000, 3, 32, 37, None, levels=table(T40, first=7)),
    "v3 pyramid": _nshape(17, 327, 1, 32, 129, PYR),
    "v3 nothing fits": _nshape(1, 100, 1, 32, 9, [(2, 3), (3, 4), (4, 5), (3, 13)]),
    "v3 gap and descending": _nshape(1, 120, 3, 32, 37, None, levels=table(T40, first=2, order=[3, 2, 1, 0], gap_before=(1, 9))),
    "v3 budget 358": _nshape(1, 5615, 1, 32, 130, [(70, 75), (15, 20), (5, 9), (3, 4)]),
    "v3 budget 359": _nshape(1, 5616, 1, 32, 130, [(70, 75), (15, 20), (5, 9), (3, 4)]),
    "v3 budget 638": _nshape(1, 10095, 1, 32, 257, [(90, 100), (20, 29), (5, 9), (3, 4)]),
    "v3 budget 639": _nshape(1, 10096, 1, 32, 257, [(90, 100), (20, 29), (5, 9), (3, 4)]),
    "v3 budget 959": _nshape(1, 15231, 1, 32, 513, [(108, 130), (29, 31), (4, 14), (1, 4)]),
    "v3 budget capped at 960": _nshape(1, 20000, 1, 32, 513, [(108, 130), (29, 31), (4, 14), (1, 4)]),
}
NATIVE_LAUNCHES = [(n, switches()) for n in NATIVE_SHAPES] + [(n, switches(op_staged=0)) for n in ("v3 pyramid", "v3 all levels staged",
                                                                                                  "v3 gap and descending", "v3 budget 359")]

SLM_SHAPES = {                                                           # (NI, C, Q, level shapes, rows in front of / behind the levels)
    "four levels": (3, 32, 37, T40, 0),
    "one level C=4": (1, 4, 9, [(5, 3)], 2),
    "eight levels C=256": (2, 256, 300, T40 + T40B, 3),
    "single pixels": (2, 8, 11, [(1, 1), (1, 4), (3, 1)], 0),
}


def switch_label(sw):
    d = {k: v for k, v in sw.items() if v != DEFAULT_SWITCHES[k]}
    return ", ".join(f"{k}={v}" for k, v in sorted(d.items())) or "default"


def lds_bytes(px, D, nt):
    return (px + 1) * D * 4 + desc_bytes(nt)


assert math.isclose(U, 2.0 ** -24)
