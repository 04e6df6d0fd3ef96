"""float64 restatements, per-element error bounds, decision margins and case lists of the stage between the encoder's class map and
a clip's selected instances (a helper, not a conftest):

    csrc/decoder_ops.hip   score_max, cell_argmax (mdqe_query_select_f32), sample_levels_mean
    csrc/clip_ops.hip      clip_assoc<16/32/64>, clip_gather_init, box_refine, box_head_refine, add_rows, time_fuse, time_fuse_dot,
                           clip_rank, clip_gram, clip_dedup (mdqe_clip_select_f32), dyn_mask<24/32>, mask_stats_reduce, mask_gram,
                           mask_iou (mdqe_dyn_mask_nms_f32), clip_finalize, rows_gather
    csrc/mask.hip          mask_row_stats
    csrc/image_ops.hip     image_mask_stats, image_final_masks

tests/test_select_ref_cpu.py shows on these cases, without a GPU, that every check below admits the formula evaluated in float32 on
the CPU, rejects a list of one-off mistakes (MISTAKES) and leaves at most 1 % of the decisions of any case undecided;
tests/test_select_forms_gpu.py holds the kernels to the same checks.  Every group has an `*_eval(case, dtype, mut)` (the formula in
float64: the reference; in float32: what the bound must admit; with `mut`: one named mistake) and a `*_verify(case, outputs)` that
raises AssertionError unless EVERY element is inside its bound and every decision obeys the margin rule, and returns the achieved
(err, bound) of the worst element per quantity.  U = 2^-24 (as in _gemm_ref); no bound is tuned from a kernel's output.

THE MARGIN RULE.  Nearly every kernel here ends in a decision (an arg-max, a threshold, a mask bit, a rank).  The float64 reference
yields the quantity x behind it, its bound b, and a margin: |x - thr| for a threshold, x_best - x_j for an arg-max.  A threshold is
DECIDED when its margin exceeds 2 b (or b = 0: the quantity is exact); candidate j of an arg-max is a CONTENDER when
x_best - x_j <= b_best + b_j (what "twice the bound" is for two quantities with bounds of their own), and the arg-max is decided
when the float64 winner is the only contender.  A decided output must equal the float64 decision; an undecided one may be either
side of the threshold, or any contender.  A count of such bits (stats[2], stats[4], n_keep, a box edge) must lie in the interval
the undecided bits allow.  Ranks (clip_rank's order, clip_finalize's sel) are held to exact equality, and the cases are built so
that NO rank decision is undecided (the CPU test asserts it): clip_rank compares inputs, which are exact.

ASSUMED ACCURACIES.  EXP_REL = 4 U (of _attn_norm_ref: 1 ulp for expf, times 2 for its internal log2(e) scaling).  LOG_REL = 4 U,
ASSUMED by the same rule: this ROCm tree documents no accuracy for logf or v_log_f32 either; 1 ulp (2 U) for the function, times 2
for the ln(2) scaling of the hardware log2.  Divisions and square roots are correctly rounded (no fast-math).

SIGMOID.  s = 1 / (1 + expf(-z)) of an argument that is off by dz:  e = exp(-z) (1 + eps), |eps| <= EXP_REL + dz, and ds / s =
(1 - s) eps, plus the roundings of the sum and the quotient:   |ds| <= 1.01 s (1 - s) (EXP_REL + dz) + 2 U s + FLUSH   (sig_bound).

BILINEAR READS (cell_argmax, sample_levels_mean, image_final_masks).  A read at source position (fy, fx) of a map m is
sum_ij w_ij m_ij with four non-negative weights of sum 1.  Its fp32 error has two parts.  (i) The weights' arithmetic: 1 - l, two
products and two sums per term, at most 8 U * sum w |m| <= 8 U A, A the largest |m| near the read.  (ii) The position itself:
fy = (o + 0.5) * (H / H_out) - 0.5 rounds the scale, the product and the difference: |dfy| <= 3 U H (5 U H for grid_sample's
((2 c - 1 + 1) H - 1) / 2, which rounds twice more).  The read is continuous and piecewise linear in fy, so it moves by at most
|dfy| * GY, GY the largest |m[y + 1, x] - m[y, x]| near the read -- also when fy crosses a pixel row and the kernel reads other
pixels than float64 does.  "Near" is the 5 x 5 pixels around the float64 read's top-left pixel (`slopes`).  So
    |dv| <= 1.01 (dfy GY + dfx GX) + 8 U A + (what the map itself is off by).
image_mask_stats reads at (p - f/2) / f with f a power of two: positions and weights are exact, only (i) remains, and
sum w |m| is aligned_bilinear(|m|) exactly.

QUERY SELECTION (transformer_dec.py:81-109).  score = max_k sigmoid(conf) = sigmoid(max_k conf), sig_bound with dz = 0.  The
resized map: the bilinear bound with the score's own bound in it.  Arg-max per cell by the margin rule, first maximum on exact
ties.  The coordinates are checked at the pixel the kernel chose, with the reference's true division: x = fmod(i, W_up) / W_up
(one rounding, U x), y = (i / W_up) / H_up (two, 2.02 U y).

SAMPLING (:171-179).  mean over levels of grid_sample(border, align_corners=False): per level the bilinear bound with 5 U, then
n_levels - 1 sums and a division: (n + 2) U mean_l A_l.

ASSOCIATION (:111-145).  sim = e_t[q] . e_ct[k], E products: (E + 2) U |e_t[q]| . |e_ct[k]|; arg-max over the admissible q by the
margin rule (the kernel's fp32-softmax tie path moves the winner only among values within 2^-23, far inside 2 b here).

BOXES (:473-480, :492-503; util/misc.py:478-482; util/box_ops.py:8-19).  inv = log(a / b), a = max(x, 1e-5), b = max(1 - x, 1e-5)
(fp32 constants): 1 - x and the quotient round once each, an absolute 2.02 U on the logarithm, and logf adds LOG_REL |inv|.
z = delta + inv rounds once.  dz = d_delta + 2.02 U + LOG_REL |inv| + U |z|, then sig_bound.  d_delta = 0 for box_refine and the
GEMM bound (K + 8) U (|h| |W|^T + |bias|) for box_head_refine.  A clamped corner c = x -+ w / 2 is off by dx + dw / 2 + U |c|; min
and max over the frames [t0, t1) are 1-Lipschitz in the largest such error; the centre and the size add one rounding each.

TIME FUSION (:374-376).  softmax over t of T weights times the frame queries: _attn_norm_ref.attend_bound with N = T, logit error
0 (time_fuse) or the GEMM bound with K = 256 (time_fuse_dot); out + pos rounds once more.

CLIP SELECT (mdqe/mdqe.py:373-379).  order and n_thr are decisions on inputs: exact.  inv_norm = 1 / max(|e|, 1e-12): C squares
and sums in any order, a square root, a quotient: (C + 3) U relative.  sim = e_p . e_q: (C + 2) U |e_p| . |e_q|.  cos = sim *
inv_p * inv_q: the three bounds and two roundings; max_p(cos) against 0.99 (fp32) by the margin rule; kept = order[keep][:max_keep].

DYNAMIC MASKS AND NMS (:384-408).  logit = coef . feats over M channels: (M + 2) U |coef| . |feats|.  soft = sigmoid: sig_bound.
hard = soft > 0.5 and any = logit > 0: margin rule.  Sums over P pixels run per wave (6 butterfly steps), over 4 waves, then over
ceil(P / 256) tiles in order (mask_row_stats: ceil(P / 256) per thread first): at most D = ceil(P / 256) + 10 roundings per term:
    stats[1], stats[3]   sum of the terms' bounds + D U sum + (s + bound) of every undecided bit that may join or leave the sum
    stats[2], stats[4]   integers in the interval the undecided bits allow
num[p, q] = soft_h[p] . hard_h[q] over Ph half-resolution pixels in any order: sum_k b_soft[p, k] hard[q, k] + (Ph + 2) U num, plus
(soft + bound) at q's undecided bits.  iou = num / (S3[p] + S4[q] - num + 1):
    |d iou| <= 1.01 (d num + iou (d S3 + d S4 + d num)) / (den + 1) + 4 U iou,      mi[q] = max over p < q, p not blank (max is
1-Lipschitz in the largest error).  The cases keep every blank test decided.

FINALIZE (:408-419).  value = (cls * (1 - mi)) * (stats[1] / (stats[2] + 1e-6)): five roundings, 5 U |value|.  alive is a decision
on inputs (exact); label, count above thr and the order are held exactly and the cases keep them decided.

IMAGE BRANCH (:509-548; util/misc.py:485-507).  aligned_bilinear (pad, interpolate with align_corners=True, shift by factor / 2),
crop, sigmoid; hard and box by the margin rule; then F.interpolate(bilinear, align_corners=False) of the crop, > 0 by the margin rule.

KERNELS OF THIS STAGE THAT STAY WITH THEIR EXISTING TESTS.  The tracker kernels (csrc/tracker*.hip) are held to the oracle by whole
sequences (tests/test_tracker*.py): their state is a recurrence, a per-launch bound says little.  The final-mask family
(csrc/final_mask.hip and the output forms built on it) is held bit for bit by the geometry and label-map tests.
"""
import torch
import torch.nn.functional as F

from _attn_norm_ref import EXP_REL, FLUSH, attend_bound, worst_ratio  # noqa: F401  (re-exported)
from _gemm_ref import U, check_within, within  # noqa: F401  (re-exported)

LOG_REL = 4 * U                     # ASSUMED (module docstring)
F64, F32 = torch.float64, torch.float32


def f32(v):
    """The fp32 number a C `float` constant or argument holds, as a Python float."""
    return float(torch.tensor(v, dtype=F32))


EPS5, EPS12, EPS6, COS_THR, TENTH = f32(1e-5), f32(1e-12), f32(1e-6), f32(0.99), f32(0.1)
_cache = {}

MISTAKES = {                        # name -> kernel group; tests/test_select_ref_cpu.py rejects every one by name
    "align_corners=True in the cell resize": "query_select", "last maximum instead of first": "query_select",
    "H_up without the +1": "query_select", "last pixel of every cell dropped": "query_select", "floor division in y": "query_select",
    "grid_sample with zero padding": "sample_levels_mean", "mean over n_levels + 1": "sample_levels_mean",
    "window not scaled by |t - ct|": "clip_assoc", "inverse_sigmoid without the clamps": "box_refine",
    "clip box over all T frames": "box_refine", "time softmax over q": "time_fuse", "> in the rank step": "clip_select",
    "cosine without one normalisation": "clip_select", "max_keep before the duplicate test": "clip_select",
    "t_step = 2 at T >= 4": "dyn_mask_nms", "half grid at odd pixels": "dyn_mask_nms", "IoU denominator without the + 1": "dyn_mask_nms",
    "blank rows take part in the NMS": "dyn_mask_nms", "best >= thr in the final count": "clip_finalize",
    "aligned_bilinear without the shift": "image_mask_stats", "final masks from the uncropped map": "image_final_masks",
}


def gen(*key):
    return torch.Generator().manual_seed(sum((i + 5) * 104729 ** (i % 3) * int(v) for i, v in enumerate(key)) % (2 ** 31))


# ---- the margin rule ------------------------------------------------------------------------------------------------------------
def threshold(x, thr, bound, ge=False):
    """(bit, decided) of x > thr (x >= thr when `ge`) for a float64 quantity x with error bound `bound`."""
    bound = torch.as_tensor(bound, dtype=F64).expand_as(x)
    return (x >= thr if ge else x > thr), ((x - thr).abs() > 2 * bound) | (bound == 0)


def contenders(v, bound, dim=-1):
    """(first arg-max, contender mask, decided) along `dim`; -inf entries never contend."""
    first = v.argmax(dim, keepdim=True)
    vmax, bmax = v.gather(dim, first), bound.gather(dim, first)
    finite = v > float("-inf")
    cont = finite & ((vmax - torch.where(finite, v, vmax)) <= bmax + bound)
    cont.scatter_(dim, first, True)
    return first.squeeze(dim), cont, cont.sum(dim) == 1


def gap_of(res, name, v, bound, first, got, dim=-1):
    """The decision's own err / bound into res[name]: how far below the float64 maximum the chosen candidate lies, over the sum of
    the two bounds (<= 1 for a contender, 0 where float64's choice was made)."""
    g = lambda a, i: a.gather(dim, i.unsqueeze(dim)).squeeze(dim)
    gap, b = g(v, first) - g(v, got), g(bound, first) + g(bound, got)
    ratio = torch.where(gap > 0, gap / b.clamp_min(1e-300), torch.zeros_like(gap)).flatten()
    i = int(ratio.argmax()) if ratio.numel() else 0
    if ratio.numel():
        res[name] = (float(gap.flatten()[i]), float(b.flatten()[i]) if float(gap.flatten()[i]) > 0 else 1.0)


def need(ok, what):
    if not bool(ok):
        raise AssertionError(what)


def need_bits(got, bit, dec, what):
    bad = (got.bool() != bit) & dec
    need(not bad.any(), f"{what}: {int(bad.sum())} decided bits differ from float64")


def need_interval(got, bit, dec, dims, what):
    lo = (bit & dec).sum(dims).double()
    hi = lo + (~dec).sum(dims)
    need(((got.double() >= lo) & (got.double() <= hi)).all(), f"{what}: count outside the interval the undecided bits allow")


def need_within(res, name, out, ref, bound, what):
    """Every element within its bound; the worst (err, bound) goes to res[name]."""
    need(out.numel() == ref.numel(), f"{what} {name}: {tuple(out.shape)} where {tuple(ref.shape)} is due")
    out = out.double().reshape(ref.shape)
    if ref.numel():
        _, err, b = worst_ratio(out, ref, bound)
        if name not in res or err * res[name][1] > res[name][0] * b:
            res[name] = (err, b)
    check_within(out, ref, bound, f"{what} {name}")


def sig_bound(s, dz):
    return 1.01 * s * (1 - s) * (EXP_REL + dz) + 2 * U * s + FLUSH


def sig64(z):
    return torch.sigmoid(z)


# ---- bilinear reads -------------------------------------------------------------------------------------------------------------
def _pool5(a):
    return F.max_pool2d(a, 5, 1, 2)


def slopes(m):
    """m [N, C, H, W] float64 -> (GY, GX, A): the largest |vertical step|, |horizontal step| and |m| in the 5 x 5 pixels around each pixel."""
    dy = F.pad((m[:, :, 1:] - m[:, :, :-1]).abs(), (0, 0, 0, 1))
    dx = F.pad((m[..., 1:] - m[..., :-1]).abs(), (0, 1))
    return _pool5(dy), _pool5(dx), _pool5(m.abs())


def resize_src(n_out, n_in):
    """Top-left source pixel of F.interpolate(bilinear, align_corners=False) per output pixel, from the float64 position."""
    f = ((torch.arange(n_out, dtype=F64) + 0.5) * n_in / n_out - 0.5).clamp_min(0.0)
    return f.floor().long().clamp_max(n_in - 1)


def resize_bound(m, Ho, Wo, extra):
    """Bound [N, C, Ho, Wo] of the fp32 bilinear resize of m [N, C, H, W] (float64), whose own elements are off by `extra` (same shape)."""
    H, W = m.shape[-2:]
    GY, GX, A = slopes(m)
    E = _pool5(extra)
    y0, x0 = resize_src(Ho, H), resize_src(Wo, W)
    pick = lambda a: a[:, :, y0][:, :, :, x0]
    return 1.01 * (3 * U * H * pick(GY) + 3 * U * W * pick(GX)) + 8 * U * pick(A) + pick(E) + FLUSH


# ---- query_select ---------------------------------------------------------------------------------------------------------------
QS_SHAPES = [(2, 7, 7, 3, 2), (3, 8, 12, 7, 4), (2, 9, 13, 5, 4), (2, 48, 80, 7, 14), (1, 23, 37, 1, 14)]       # (NI, H, W, K, nb)
QS_SETS = ("normal", "offset")      # unit normal x 2; the same with a common offset of -3 (logits stay within about +-8)
QS_EXACT = ("zero", "peak")


def qs_up(n, nb):
    return (2 * n // nb + 1) * nb


def qs_branch(H, W, nb):
    px = (qs_up(H, nb) // nb) * (qs_up(W, nb) // nb)
    return f"cell_argmax {'one pass' if px <= 64 else 'several passes'} of the wave"


def qs_conf(NI, H, W, K, nb, vs):
    g = gen(NI, H, W, K, nb, 3)
    if vs == "normal":
        return torch.randn(NI, H, W, K, generator=g) * 2
    if vs == "offset":
        return (torch.randn(NI, H, W, K, generator=g) * 1.5 - 3.0).clamp(-8, 8)
    conf = torch.full((NI, H, W, K), -1e4)                   # sigmoid(-1e4) is exactly 0 in fp32 and in float64
    if vs == "peak":                                          # one source pixel at logit 0 (score exactly 0.5), just below and right of
        r, t = qs_up(H, nb) // nb, qs_up(W, nb) // nb          # where the last pixel of cell 0 reads: that pixel's weight on it is the cell's largest
        fy, fx = (r - 0.5) * H / qs_up(H, nb) - 0.5, (t - 0.5) * W / qs_up(W, nb) - 0.5
        conf[:, int(-(-fy // 1)), int(-(-fx // 1)), K - 1] = 0.0
    return conf


def qs_eval(conf, nb, dt, mut=None):
    """dict(score [NI, H, W], cells [NI, nb^2, r t] (the resized map, cell by cell), idx [NI, nb^2] (pixel in the cell), coords [NI, nb^2, 2])."""
    NI, H, W, K = conf.shape
    s = torch.sigmoid(conf.to(dt)).amax(-1)
    plus = 0 if mut == "H_up without the +1" else 1
    H_up, W_up = (2 * H // nb + plus) * nb, (2 * W // nb + plus) * nb
    up = F.interpolate(s[:, None], size=(H_up, W_up), mode="bilinear", align_corners=mut == "align_corners=True in the cell resize")[:, 0]
    r, t = H_up // nb, W_up // nb
    cells = up.view(NI, nb, r, nb, t).permute(0, 1, 3, 2, 4).reshape(NI, nb * nb, r * t)
    if mut == "last maximum instead of first":
        p = r * t - 1 - cells.flip(-1).argmax(-1)
    elif mut == "last pixel of every cell dropped":
        p = cells[..., :-1].argmax(-1)
    else:
        p = cells.argmax(-1)
    cell = torch.arange(nb * nb)
    row, col = (cell // nb) * r + p // t, (cell % nb) * t + p % t
    idx = (row * W_up + col).to(dt)
    y = torch.floor(idx / W_up) / H_up if mut == "floor division in y" else (idx / W_up) / H_up
    return dict(score=s, cells=cells, idx=p, coords=torch.stack([torch.fmod(idx, W_up) / W_up, y], -1))


def qs_case(NI, H, W, K, nb, vs):
    key = ("qs", NI, H, W, K, nb, vs)
    if key not in _cache:
        conf = qs_conf(NI, H, W, K, nb, vs)
        ref = qs_eval(conf, nb, F64)
        s = ref["score"]
        bs = sig_bound(s, 0.0)
        H_up, W_up = qs_up(H, nb), qs_up(W, nb)
        bu = resize_bound(s[:, None], H_up, W_up, bs[:, None])[:, 0] if vs in QS_SETS else torch.zeros(NI, H_up, W_up, dtype=F64)
        r, t = H_up // nb, W_up // nb
        bcell = bu.view(NI, nb, r, nb, t).permute(0, 1, 3, 2, 4).reshape(NI, nb * nb, r * t)
        first, cont, dec = contenders(ref["cells"], bcell)
        _cache[key] = dict(conf=conf, nb=nb, exact=vs in QS_EXACT, ref=ref, score_bound=bs, cont=cont, decided=dec, dims=(H_up, W_up, r, t),
                           cell_bound=bcell)
    return _cache[key]


def qs_verify(c, score, coords):
    res, nb = {}, c["nb"]
    H_up, W_up, r, t = c["dims"]
    what = f"query_select {tuple(c['conf'].shape)} nb={nb}"
    need_within(res, "score", score, c["ref"]["score"], c["score_bound"], what)
    co = coords.double()
    need(co.shape == c["ref"]["coords"].shape and bool(torch.isfinite(co).all()), f"{what}: coords shape / finite")
    col = torch.round(co[..., 0] * W_up).long()
    row = torch.floor(co[..., 1] * H_up + 0.5 / W_up).long()
    cell = torch.arange(nb * nb)
    need(((row // r == cell // nb) & (col // t == cell % nb) & (row >= 0) & (col >= 0)).all(), f"{what}: a coordinate lies outside its cell")
    p = (row % r) * t + col % t
    if c["exact"]:
        need((p == c["ref"]["idx"]).all(), f"{what}: exact case, not the first maximum of the cell")
    need(c["cont"].gather(-1, p[..., None]).all(), f"{what}: a cell's pixel is no contender for its maximum")
    gap_of(res, "cell arg-max gap", c["ref"]["cells"], c["cell_bound"], c["ref"]["idx"], p)
    idx = (row * W_up + col).double()
    x, y = torch.fmod(idx, W_up) / W_up, (idx / W_up) / H_up
    need_within(res, "coords", co, torch.stack([x, y], -1), torch.stack([U * x, 2.02 * U * y], -1), what)
    return res


# ---- sample_levels_mean ---------------------------------------------------------------------------------------------------------
SLM_LEVELS = {"four": [(12, 20), (6, 10), (3, 5), (2, 3)], "one 1x1": [(1, 1)],
              "eight": [(12, 20), (6, 10), (3, 5), (2, 3), (1, 1), (5, 2), (1, 7), (4, 4)]}
SLM_CASES = [("four", 4, 0), ("four", 64, 7), ("four", 256, 0), ("one 1x1", 4, 3), ("one 1x1", 64, 0), ("eight", 4, 0), ("eight", 64, 5),
             ("eight", 256, 2)]    # (levels, C, token rows before the first level)
SLM_SETS = ("normal", "offset")     # unit normal; the same plus 100


def slm_eval(tok, coords, shapes, starts, dt, mut=None):
    NI, N, C = tok.shape
    g = (2 * coords.to(dt) - 1).view(NI, 1, -1, 2)
    acc = 0
    for (H, W), st in zip(shapes, starts):
        lvl = tok[:, st:st + H * W].to(dt).view(NI, H, W, C).permute(0, 3, 1, 2)
        acc = acc + F.grid_sample(lvl, g, mode="bilinear", padding_mode="zeros" if mut == "grid_sample with zero padding" else "border",
                                  align_corners=False)[:, :, 0]
    return (acc / (len(shapes) + (1 if mut == "mean over n_levels + 1" else 0))).permute(0, 2, 1)


def slm_bound(tok, coords, shapes, starts):
    NI, N, C = tok.shape
    c = coords.double()
    b, a = 0, 0
    for (H, W), st in zip(shapes, starts):
        lvl = tok[:, st:st + H * W].double().view(NI, H, W, C).permute(0, 3, 1, 2)
        GY, GX, A = slopes(lvl)
        x0 = (c[..., 0] * W - 0.5).clamp(0, W - 1).floor().long()
        y0 = (c[..., 1] * H - 0.5).clamp(0, H - 1).floor().long()
        pick = lambda m: torch.stack([m[i][:, y0[i], x0[i]] for i in range(NI)])          # [NI, C, Qn]
        b = b + 1.01 * (5 * U * H * pick(GY) + 5 * U * W * pick(GX)) + 8 * U * pick(A)
        a = a + pick(A)
    n = len(shapes)
    return ((b + (n + 2) * U * a) / n).permute(0, 2, 1) + FLUSH


def slm_case(levels, C, front, vs):
    key = ("slm", levels, C, front, vs)
    if key not in _cache:
        shapes = SLM_LEVELS[levels]
        g = gen(len(shapes), C, front, SLM_SETS.index(vs))
        starts, n = [], front
        for H, W in shapes:
            starts.append(n)
            n += H * W
        NI = 2
        tok = torch.randn(NI, n + 3, C, generator=g) + (100.0 if vs == "offset" else 0.0)
        H0, W0 = shapes[0]
        pts = [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)]
        pts += [((j + 0.5) / W0, (i + 0.5) / H0) for i, j in ((0, 0), (H0 - 1, W0 - 1), (H0 // 2, W0 // 3))]          # pixel centres
        pts += [(j / W0, i / H0) for i, j in ((1 % (H0 + 1), 1 % (W0 + 1)), (H0 // 2, W0 // 2), (H0, W0 // 2))]         # pixel edges
        coords = torch.cat([torch.tensor(pts, dtype=F32), torch.rand(26, 2, generator=g)])[None].repeat(NI, 1, 1).contiguous()
        coords[1] = coords[1].flip(0)
        _cache[key] = dict(tok=tok, coords=coords, shapes=shapes, starts=starts, ref=slm_eval(tok, coords, shapes, starts, F64),
                           bound=slm_bound(tok, coords, shapes, starts))
    return _cache[key]


# ---- clip_assoc, clip_gather_init -----------------------------------------------------------------------------------------------
# (E, Q, T, window, Bc): every E with every block count (Q = 16: one block; 81: two, the last partial; 196: four, the last partial; 256: four full), every T,
# every window
ASSOC_CASES = [(16, 16, 1, 2.5, 2), (16, 81, 2, 0.0, 2), (16, 196, 3, 2.5, 2), (32, 16, 5, 100.0, 3), (32, 81, 3, 2.5, 2), (32, 256, 2, 2.5, 1),
               (64, 16, 3, 0.0, 2), (64, 81, 5, 2.5, 2), (64, 196, 2, 100.0, 1), (64, 256, 5, 2.5, 1), (32, 196, 1, 100.0, 2)]
ASSOC_SETS = ("normal", "scaled")   # unit normal; the same x 30 (similarities of order 1e4)


def assoc_sim(emb, fidx, ct, wdw, nb, dt, mut=None):
    """Masked similarities [Bc, T, Q (candidates q), Q (centre queries k)]."""
    e = emb.to(dt)[fidx.long()]
    sim = torch.einsum("btqe,bke->btqk", e, e[:, ct])
    Q = e.shape[2]
    qi, qj = torch.arange(Q) // nb, torch.arange(Q) % nb
    rel = torch.maximum((qi[:, None] - qi[None]).abs(), (qj[:, None] - qj[None]).abs()).double()
    for t in range(e.shape[1]):
        w = wdw if mut == "window not scaled by |t - ct|" else wdw * abs(t - ct)
        sim[:, t].masked_fill_(rel > w, float("-inf"))
    return sim


def assoc_case(E, Q, T, wdw, Bc, vs):
    key = ("assoc", E, Q, T, wdw, Bc, vs)
    if key not in _cache:
        g = gen(E, Q, T, int(wdw), Bc, ASSOC_SETS.index(vs))
        nf = Bc + T
        nb, ct = int(round(Q ** 0.5)), (T - 1) // 2
        emb = torch.randn(nf, Q, E, generator=g) * (30.0 if vs == "scaled" else 1.0)
        fidx = torch.stack([(torch.arange(T - 1, -1, -1) + b) if b % 2 else torch.arange(T) // 2 + b for b in range(Bc)]).int()   # descending; repeated
        sim = assoc_sim(emb, fidx, ct, wdw, nb, F64)
        e = emb.double().abs()[fidx.long()]
        bound = (E + 2) * U * torch.einsum("btqe,bke->btqk", e, e[:, ct])
        first, cont, dec = contenders(sim, bound, dim=2)
        C = 8
        content, coords = torch.randn(nf, Q, C, generator=g), torch.rand(nf, Q, 2, generator=g)
        _cache[key] = dict(emb=emb, fidx=fidx, ct=ct, wdw=wdw, nb=nb, ref=first, cont=cont, decided=dec, content=content, coords=coords,
                           sim=sim, bound=bound)
    return _cache[key]


def assoc_verify(c, idx):
    idx = idx.long()
    Q = c["emb"].shape[1]
    need(idx.shape == c["ref"].shape and bool(((idx >= 0) & (idx < Q)).all()), "clip_assoc: index out of range")
    need(c["cont"].gather(2, idx[:, :, None, :]).all(), "clip_assoc: an index is no contender for the arg-max")
    res = {}
    gap_of(res, "arg-max gap", c["sim"], c["bound"], c["ref"], idx, dim=2)
    return res


def gather_init_ref(content, coords, fidx, idx, ct):
    """x [Bc, T, Q, C], ref [Bc, T, Q, 4], x_inst [Bc, Q, C]; idx None: identity."""
    Bc, T = fidx.shape
    Q = content.shape[1]
    q = idx.long() if idx is not None else torch.arange(Q).expand(Bc, T, Q)
    f = fidx.long()[:, :, None].expand(Bc, T, Q)
    x = content[f, q]
    ref = torch.cat([coords[f, q], torch.full((Bc, T, Q, 2), TENTH)], -1)
    return x, ref, x[:, ct].clone()


# ---- box_refine, box_head_refine ------------------------------------------------------------------------------------------------
BOX_CASES = [(2, 3, 37, "0,T"), (1, 3, 300, "1,T+1"), (2, 5, 16, "0,1"), (1, 5, 70, "1,T+1"), (3, 1, 5, "0,T")]       # (Bc, T, Q, frames)
BOX_SETS = ("normal", "scaled")     # delta unit normal; delta up to +-30
HEAD_CASES = [(2, 3, 9, 256, 260, "0,T"), (1, 5, 130, 512, 520, "1,T+1"), (1, 2, 6, 512, 512, "0,1")]                  # (Bc, T, Q, K, ldh, frames)
PREV_EDGES = (0.0, 1.0, 1e-5, 1 - 1e-5, -0.25, 1.5, 0.5, 3e-6)


def frames(T, which):
    return {"0,T": (0, T), "1,T+1": (1, T + 1), "0,1": (0, 1)}[which]


def inv_sigmoid(x, mut=None):
    x = x.clamp(0, 1)
    if mut == "inverse_sigmoid without the clamps":
        return torch.log(x / (1 - x))
    return torch.log(x.clamp_min(EPS5) / (1 - x).clamp_min(EPS5))


def box_eval(delta, prev, t0, t1, dt, mut=None):
    """(boxes [Bc, T, Q, 4], ibox [Bc, Q, 4]) from delta (in dt already, or fp32) and prev."""
    o = torch.sigmoid(delta.to(dt) + inv_sigmoid(prev.to(dt), mut))
    T = o.shape[1]
    ob = o if mut == "clip box over all T frames" else o[:, t0:min(t1, T)]
    lo = (ob[..., :2] - 0.5 * ob[..., 2:]).clamp(0, 1).amin(1)
    hi = (ob[..., :2] + 0.5 * ob[..., 2:]).clamp(0, 1).amax(1)
    return o, torch.cat([(lo + hi) / 2, hi - lo], -1)


def box_bound(delta64, ddelta, prev, t0, t1):
    inv = inv_sigmoid(prev.double())
    z = delta64 + inv
    o = torch.sigmoid(z)
    bo = sig_bound(o, ddelta + 2.02 * U + LOG_REL * inv.abs() + U * z.abs())
    T = o.shape[1]
    ob, bb = o[:, t0:min(t1, T)], bo[:, t0:min(t1, T)]
    lo, hi = (ob[..., :2] - 0.5 * ob[..., 2:]).clamp(0, 1), (ob[..., :2] + 0.5 * ob[..., 2:]).clamp(0, 1)
    bc = bb[..., :2] + 0.5 * bb[..., 2:]
    blo, bhi = (bc + U * lo).amax(1), (bc + U * hi).amax(1)
    lo, hi = lo.amin(1), hi.amax(1)
    return bo, torch.cat([(blo + bhi) / 2 + 2 * U * (lo + hi) / 2, blo + bhi + U * (hi - lo)], -1)


def _prev(Bc, T, Q, g):
    prev = torch.rand(Bc, T, Q, 4, generator=g)
    flat = prev.view(-1)
    flat[:len(PREV_EDGES) * 5:5] = torch.tensor(PREV_EDGES, dtype=F32)[:(flat.numel() + 4) // 5]
    return prev


def box_case(Bc, T, Q, which, vs):
    key = ("box", Bc, T, Q, which, vs)
    if key not in _cache:
        g = gen(Bc, T, Q, len(which), BOX_SETS.index(vs))
        delta = torch.randn(Bc, T, Q, 4, generator=g) if vs == "normal" else (torch.rand(Bc, T, Q, 4, generator=g) * 60 - 30)
        prev = _prev(Bc, T, Q, g)
        t0, t1 = frames(T, which)
        ref = box_eval(delta, prev, t0, t1, F64)
        _cache[key] = dict(delta=delta, prev=prev, t0=t0, t1=t1, ref=ref, bound=box_bound(delta.double(), 0.0, prev, t0, t1))
    return _cache[key]


def head_case(Bc, T, Q, K, ldh, which):
    key = ("head", Bc, T, Q, K, ldh, which)
    if key not in _cache:
        g = gen(Bc, T, Q, K, ldh)
        h = torch.randn(Bc * T * Q, K, generator=g)
        W, bias = torch.randn(4, K, generator=g) / K ** 0.5 * 3, torch.randn(4, generator=g)
        prev = _prev(Bc, T, Q, g)
        t0, t1 = frames(T, which)
        d64 = (h.double() @ W.double().t() + bias.double()).view(Bc, T, Q, 4)
        dd = ((K + 8) * U * (h.double().abs() @ W.double().abs().t() + bias.double().abs())).view(Bc, T, Q, 4)
        _cache[key] = dict(h=h, W=W, bias=bias, prev=prev, t0=t0, t1=t1, ldh=ldh, ref=box_eval(d64, prev, t0, t1, F64),
                           bound=box_bound(d64, dd, prev, t0, t1))
    return _cache[key]


def box_verify(c, boxes, ibox, what):
    res = {}
    need_within(res, "boxes", boxes, c["ref"][0], c["bound"][0], what)
    need_within(res, "ibox", ibox, c["ref"][1], c["bound"][1], what)
    return res


# ---- time_fuse, time_fuse_dot ---------------------------------------------------------------------------------------------------
FUSE_CASES = [(2, 1, 5, 4), (1, 2, 37, 64), (2, 4, 9, 256), (1, 8, 70, 4), (1, 8, 3, 256), (3, 4, 2, 64)]             # (Bc, T, Q, C)
FUSE_DOT_CASES = [(2, 1, 5), (1, 2, 37), (2, 4, 9), (1, 8, 6)]                                                           # (Bc, T, Q); C = 256
FUSE_SETS = ("normal", "equal", "scaled")      # weights unit normal; all equal; x 30


def fuse_eval(w, x, pos, dt, mut=None):
    """w [Bc, T, Q] (in dt already, or fp32), x [Bc, T, Q, C], pos [Bc, Q, C] -> (out, out + pos)."""
    p = torch.softmax(w.to(dt), 2 if mut == "time softmax over q" else 1)
    out = (p[..., None] * x.to(dt)).sum(1)
    return out, out + pos.to(dt)


def fuse_bound(w64, dw, x, pos):
    t = w64.permute(0, 2, 1)[:, :, None, :]
    dwt = dw.permute(0, 2, 1)[:, :, None, :] if torch.is_tensor(dw) else torch.zeros_like(t)
    b = attend_bound(t, dwt, x.double().permute(0, 2, 1, 3))[:, :, 0]
    out, out2 = fuse_eval(w64, x, pos, F64)
    return b + U * out.abs(), b + U * out.abs() + U * out2.abs()


def fuse_case(Bc, T, Q, C, vs):
    key = ("fuse", Bc, T, Q, C, vs)
    if key not in _cache:
        g = gen(Bc, T, Q, C, FUSE_SETS.index(vs))
        w = torch.randn(Bc, T, Q, generator=g) * (30.0 if vs == "scaled" else 1.0)
        if vs == "equal":
            w = w[:, :1].expand(Bc, T, Q).contiguous()
        x, pos = torch.randn(Bc, T, Q, C, generator=g), torch.randn(Bc, Q, C, generator=g)
        _cache[key] = dict(w=w, x=x, pos=pos, ref=fuse_eval(w, x, pos, F64), bound=fuse_bound(w.double(), 0.0, x, pos))
    return _cache[key]


def fuse_dot_case(Bc, T, Q, vs):
    key = ("fuse_dot", Bc, T, Q, vs)
    if key not in _cache:
        C = 256
        g = gen(Bc, T, Q, 77, FUSE_SETS.index(vs))
        xw, src = torch.randn(Bc, T, Q, C, generator=g), torch.randn(Bc, T, Q, C, generator=g)
        wt = torch.randn(C, generator=g) / 16 * (30.0 if vs == "scaled" else 1.0)
        if vs == "equal":
            wt = torch.zeros(C)
        bt = torch.randn(1, generator=g)
        w64 = xw.double() @ wt.double() + bt.double()
        dw = (C + 8) * U * (xw.double().abs() @ wt.double().abs() + bt.double().abs())
        zero = torch.zeros(Bc, Q, C)
        _cache[key] = dict(xw=xw, wt=wt, bt=bt, src=src, ref=fuse_eval(w64, src, zero, F64)[0], bound=fuse_bound(w64, dw, src, zero)[0])
    return _cache[key]


# ---- clip_select ----------------------------------------------------------------------------------------------------------------
# (Q, K, C, n_thr wanted per clip (B = 3), max_keep)
SELECT_CASES = [(16, 1, 4, (1, 5, 16), 100), (100, 5, 24, (64, 65, 100), 40), (196, 25, 64, (128, 129, 1), 1000),
                (256, 5, 256, (256, 65, 129), 50), (256, 1, 24, (64, 128, 2), 3)]
SELECT_SETS = ("normal", "scaled")  # embeddings unit normal; x 1000
SELECT_THR = 0.3


def select_eval(cls, emb, thr, max_keep, dt, mut=None):
    """Per clip: dict(order [Q], n_thr, inv_norm [Q] (rank order), sim [Q, Q] (rank order), cos, ms [n_thr], kept [n_keep])."""
    out, thr = [], f32(thr)
    for b in range(cls.shape[0]):
        s = cls[b].to(dt).amax(-1)
        order = torch.argsort(s, descending=True, stable=True)
        ss = s[order]
        lim = min(thr, float(ss[0]))
        n = int((ss > lim).sum() if mut == "> in the rank step" else (ss >= lim).sum())
        e = emb[b].to(dt)[order]
        inv = 1.0 / e.norm(dim=-1).clamp_min(EPS12)
        sim = e @ e.t()
        cos = sim * inv[None] if mut == "cosine without one normalisation" else sim * inv[:, None] * inv[None]
        m = min(n, max_keep) if mut == "max_keep before the duplicate test" else n
        keep = torch.ones(m, dtype=torch.bool)
        ms = torch.zeros(m, dtype=dt)
        if m > 1:
            ms = torch.triu(cos[:m, :m], 1).amax(0)
            keep = ms < COS_THR
        out.append(dict(order=order, n_thr=n, inv_norm=inv, sim=sim, cos=cos, ms=ms, kept=order[:m][keep][:max_keep]))
    return out


def select_case(Q, K, C, n_want, max_keep, vs):
    key = ("select", Q, K, C, n_want, max_keep, vs)
    if key not in _cache:
        g = gen(Q, K, C, max_keep, SELECT_SETS.index(vs))
        B = len(n_want)
        cls = torch.rand(B, Q, K, generator=g) * 0.2                                  # everything below thr - 0.1 ...
        emb = torch.randn(B, Q, C, generator=g)
        for b, n in enumerate(n_want):
            top = torch.randperm(Q, generator=g)[:n]
            if n > 1 or b == 1:                                                       # ... but n queries (n == 1 on clip 0: nothing reaches thr)
                cls[b, top, torch.randint(0, K, (n,), generator=g)] = 0.4 + 0.5 * torch.rand(n, generator=g)
            if n >= 5:
                cls[b, top[1], :] = cls[b, top[0], :]                                  # equal class scores: ranked by query index
                cls[b, top[3], :] = cls[b, top[0], :]
                d = torch.randn(2, C, generator=g)
                d -= (d @ emb[b, top[2]])[:, None] * emb[b, top[2]] / emb[b, top[2]].norm() ** 2
                d *= (emb[b, top[2]].norm() / d.norm(dim=-1))[:, None]
                emb[b, top[4]] = 3.0 * (emb[b, top[2]] + 0.05 * d[0])                  # cosine 0.99875 with top[2]: a duplicate
                emb[b, top[0]] = 0.5 * (emb[b, top[2]] + 0.25 * d[1])                  # cosine 0.970: none
                cls[b, top[2], 0], cls[b, top[4], 0] = 0.97, 0.96                      # ranks 0 and 1: the duplicate sits inside any max_keep
                if n >= 6:
                    emb[b, top[5]] = 0.0                                               # a zero embedding: the 1e-12 clamp
        if vs == "scaled":
            emb = emb * 1000.0
        ref = select_eval(cls, emb, SELECT_THR, max_keep, F64)
        for b, r in enumerate(ref):
            e = emb[b].double()[r["order"]]
            inv, n = r["inv_norm"], r["n_thr"]
            binv = (C + 3) * U * inv
            bsim = (C + 2) * U * (e.abs() @ e.abs().t())
            bcos = bsim * inv[:, None] * inv[None] + r["cos"].abs() * 2 * ((C + 3) * U + U) * 1.01
            r["b_inv"], r["b_sim"] = binv, bsim
            r["b_ms"] = torch.triu(bcos[:n, :n], 1).amax(0) if n > 1 else torch.zeros(n, dtype=F64)
            bit, dec = threshold(r["ms"], COS_THR, r["b_ms"]) if n > 1 else (torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool))
            r["keep"], r["decided"] = ~bit & (r["ms"] != COS_THR) if n > 1 else torch.ones(n, dtype=torch.bool), dec
            tp = torch.arange(Q) // 64
            r["computed"] = (torch.arange(Q)[:, None] < n) & (torch.arange(Q)[None] < n) & (tp[None] >= tp[:, None])
        _cache[key] = dict(cls=cls, emb=emb, thr=SELECT_THR, max_keep=max_keep, ref=ref)
    return _cache[key]


def select_verify(c, order, n_thr, inv_norm, sim, kept, n_keep):
    """order [B, Q], n_thr [B], inv_norm [B, Q], sim [B, Q, Q], kept [B, Q], n_keep [B] (what lies outside the written part is the caller's)."""
    res = {}
    for b, r in enumerate(c["ref"]):
        what = f"clip_select clip {b}"
        need((order[b].long() == r["order"]).all(), f"{what}: order")
        need(int(n_thr[b]) == r["n_thr"], f"{what}: n_thr {int(n_thr[b])} != {r['n_thr']}")
        need_within(res, "inv_norm", inv_norm[b], r["inv_norm"], r["b_inv"], what)
        m = r["computed"]
        need_within(res, "sim", sim[b][m], r["sim"][m], r["b_sim"][m], what)
        nk, j = int(n_keep[b]), 0
        need(0 <= nk <= min(r["n_thr"], c["max_keep"]), f"{what}: n_keep out of range")
        for rank in range(r["n_thr"]):
            if j >= c["max_keep"]:
                break
            q = int(r["order"][rank])
            hit = j < nk and int(kept[b, j]) == q
            if r["decided"][rank]:
                need(hit == bool(r["keep"][rank]), f"{what}: rank {rank} (query {q}) {'missing from' if r['keep'][rank] else 'wrongly in'} kept")
            j += int(hit)
        need(j == nk, f"{what}: kept holds {nk} entries, {j} of them explained")
    return res


# ---- dyn_mask_nms, mask_row_stats -----------------------------------------------------------------------------------------------
# (M, T, H, W, Q, kept counts per clip): P = T H W below 256 / off a multiple / a multiple of 256; Ph % 4 zero and not; both t_steps;
# one-tile and multi-tile mask_gram (32-row tiles); 66 clips: two launches of 64
DYN_CASES = [(8, 1, 2, 2, 16, tuple([0, 1, 2, 3] * 16 + [2, 1])), (24, 4, 5, 7, 64, (33, 0, 2)), (32, 5, 16, 24, 100, (65, 1, 31)),
             (8, 6, 5, 7, 32, (32,)), (32, 4, 16, 24, 16, (2,)), (24, 1, 5, 7, 16, (3, 1, 0))]
DYN_SETS = ("normal", "scaled")     # coefficients unit normal / sqrt(M); x 8
ROW_CASES = [(3, 5, 7, 6), (4, 5, 7, 5), (5, 7, 9, 4), (5, 16, 24, 3)]                                                    # (T, H, W, n)


def t_step_of(T, mut=None):
    return 2 if T >= (4 if mut == "t_step = 2 at T >= 4" else 5) else 1


def dyn_branch(M, T, H, W, counts):
    Ph = -(-T // t_step_of(T)) * (H // 2) * (W // 2)
    nt = (max(counts) + 31) // 32
    return [f"dyn_mask<{24 if M == 24 else 32}> M={M}", f"t_step={t_step_of(T)}", f"mask_gram {'vector' if Ph % 4 == 0 else 'scalar'} loads",
            f"mask_gram {'one tile' if nt <= 1 else 'several tiles'}"] + (["second launch of 64 clips"] if len(counts) > 64 else [])


def stats_eval(logits, dt, mut=None):
    """logits [n, T, H, W] in dt -> (soft_h [n, Ph], hard_h [n, Ph], stats [n, 5])."""
    n, T, H, W = logits.shape
    step, o = t_step_of(T, mut), 1 if mut == "half grid at odd pixels" else 0
    s = torch.sigmoid(logits)
    hard = s > 0.5
    sh = torch.sigmoid(logits[:, ::step, o:2 * (H // 2):2, o:2 * (W // 2):2]).flatten(1)
    hh = sh > 0.5
    stats = torch.stack([(logits > 0).flatten(1).any(1).to(dt), (s * hard).flatten(1).sum(1), hard.flatten(1).sum(1).to(dt), sh.sum(1),
                         hh.sum(1).to(dt)], 1)
    return sh, hh.to(dt), stats


def nms_eval(sh, hh, stats, mut=None):
    """max soft-IoU of every row with the non-blank rows before it: mi [n]."""
    n = sh.shape[0]
    if n < 2:
        return torch.zeros(n, dtype=sh.dtype)
    num = sh @ hh.t()
    den = stats[:, 3][:, None] + stats[:, 4][None] - num + (0 if mut == "IoU denominator without the + 1" else 1)
    iou = torch.triu(num / den, 1)
    if mut != "blank rows take part in the NMS":
        iou = iou * (stats[:, 0] > 0).to(iou.dtype)[:, None]
    return iou.amax(0)


def dyn_logits(coef, kept, feats, b, n, f0, T, dt):
    c = coef[b, kept[b, :n].long()].to(dt)
    return torch.einsum("qm,thwm->qthw", c, feats[f0:f0 + T].to(dt))


def dyn_eval(c, dt, mut=None):
    """Per clip (logits, soft_h, hard_h, stats, mi)."""
    out = []
    for b, n in enumerate(c["counts"]):
        lg = dyn_logits(c["coef"], c["kept"], c["feats"], b, n, c["f0"][b], c["T"], dt)
        sh, hh, st = stats_eval(lg, dt, mut)
        out.append((lg, sh, hh, st, nms_eval(sh, hh, st, mut)))
    return out


def stats_bounds(lg, dv):
    """Everything stats_verify needs, from the float64 logits [n, T, H, W] and their bound dv (same shape)."""
    n, T, H, W = lg.shape
    step, P = t_step_of(T), T * H * W
    D = -(-P // 256) + 10
    s = torch.sigmoid(lg)
    bs = sig_bound(s, dv)
    hard, hdec = threshold(s, 0.5, bs)
    pos, pdec = threshold(lg, 0.0, dv)
    half = lambda a: a[:, ::step, 0:2 * (H // 2):2, 0:2 * (W // 2):2].flatten(1)
    sh, bsh, hh, hhdec = half(s), half(bs), half(hard), half(hdec)
    any_true, any_dec = (pos & pdec).flatten(1).any(1), (pos & pdec).flatten(1).any(1) | pdec.flatten(1).all(1)
    maybe = lambda x, b, bit, dec: ((b * (bit & dec)) + (x + b) * ~dec).flatten(1).sum(1) + D * U * (x * (bit | ~dec)).flatten(1).sum(1)
    b1 = maybe(s, bs, hard, hdec)
    b3 = bsh.sum(1) + D * U * sh.sum(1)
    return dict(s=s, bs=bs, hard=hard, hdec=hdec, sh=sh, bsh=bsh, hh=hh, hhdec=hhdec, any=any_true, any_dec=any_dec, b1=b1, b3=b3,
                share=float(((~hdec).sum() + (~pdec).sum()) / max(1, 2 * lg.numel())))


def nms_bounds(sb, st):
    """(mi float64, its bound) of one clip from stats_bounds' dict and the float64 stats."""
    n, Ph = sb["sh"].shape
    if n < 2:
        return torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    sh, bsh, hh, und = sb["sh"], sb["bsh"], sb["hh"].double(), (~sb["hhdec"]).double()
    num = sh @ hh.t()
    may = hh.clamp_min(und)
    bnum = bsh @ may.t() + (sh + bsh) @ und.t() + (Ph + 2) * U * (sh @ may.t())
    den1 = st[:, 3][:, None] + st[:, 4][None] - num + 1
    iou = num / den1
    biou = 1.01 * (bnum + iou * (sb["b3"][:, None] + und.sum(1)[None] + bnum)) / den1 + 4 * U * iou
    live = (st[:, 0] > 0).double()[:, None]
    return torch.triu(iou, 1).mul(live).amax(0), torch.triu(biou, 1).mul(live).amax(0)


def dyn_case(M, T, H, W, Q, counts, vs):
    key = ("dyn", M, T, H, W, Q, counts, vs)
    if key not in _cache:
        g = gen(M, T, H, W, Q, len(counts), DYN_SETS.index(vs))
        B = len(counts)
        nf = T + 3
        feats = torch.randn(nf, H, W, M, generator=g)
        feats[..., 0] = feats[..., 0].abs() + 1.0                                      # channel 0 is positive: -e_0 is a blank mask
        coef = torch.randn(B, Q, M, generator=g) / M ** 0.5 * (8.0 if vs == "scaled" else 1.0)
        kept = torch.stack([torch.randperm(Q, generator=g) for _ in range(B)]).int()
        f0 = [(3 - b) % 4 for b in range(B)]                                           # descending, overlapping windows of the cache
        for b, n in enumerate(counts):
            k = kept[b].long()
            if n >= 3:
                coef[b, k[1]] = 0.0
                coef[b, k[1], 0] = -1.0                                                # one blank row, before the end
                coef[b, k[2]] = coef[b, k[0]]                                          # two identical rows
            elif n == 2 and b % 2:
                coef[b, k[1]] = coef[b, k[0]]
        c = dict(M=M, T=T, H=H, W=W, Q=Q, counts=counts, coef=coef, kept=kept, feats=feats, f0=f0,
                 row0=[sum(counts[:b]) for b in range(B)])
        ref, bounds = dyn_eval(c, F64), []
        for b, n in enumerate(counts):
            ca = coef[b, kept[b, :n].long()].double().abs()
            dv = (M + 2) * U * torch.einsum("qm,thwm->qthw", ca, feats[f0[b]:f0[b] + T].double().abs())
            sb = stats_bounds(ref[b][0], dv)
            sb["dv"] = dv
            sb["mi"], sb["bmi"] = nms_bounds(sb, ref[b][3])
            bounds.append(sb)
        c.update(ref=ref, bounds=bounds)
        _cache[key] = c
    return _cache[key]


def stats_verify(res, sb, ref_stats, soft_h, hard_h, stats, what):
    need_within(res, "soft_h", soft_h, sb["sh"], sb["bsh"], what)
    need(((hard_h == 0) | (hard_h == 1)).all(), f"{what}: hard_h is not 0 / 1")
    need_bits(hard_h.reshape(sb["hh"].shape), sb["hh"], sb["hhdec"], f"{what} hard_h")
    st = stats.double()
    need(sb["any_dec"].all(), f"{what}: the case leaves a blank test undecided")
    need((st[:, 0] == sb["any"].double()).all(), f"{what}: stats[0] (not blank)")
    need_within(res, "stats[1]", st[:, 1], ref_stats[:, 1], sb["b1"], what)
    need_interval(st[:, 2], sb["hard"].flatten(1), sb["hdec"].flatten(1), 1, f"{what} stats[2]")
    need_within(res, "stats[3]", st[:, 3], ref_stats[:, 3], sb["b3"], what)
    need_interval(st[:, 4], sb["hh"], sb["hhdec"], 1, f"{what} stats[4]")


def dyn_verify(c, b, logits, soft_h, hard_h, stats, mi):
    """One clip's rows of every output of mdqe_dyn_mask_nms_f32."""
    res, sb, ref = {}, c["bounds"][b], c["ref"][b]
    what = f"dyn_mask_nms M={c['M']} T={c['T']} {c['H']}x{c['W']} clip {b} ({c['counts'][b]} rows)"
    need_within(res, "logits", logits, ref[0], sb["dv"], what)
    stats_verify(res, sb, ref[3], soft_h, hard_h, stats, what)
    need_within(res, "mi", mi, sb["mi"], sb["bmi"], what)
    return res


def row_case(T, H, W, n, vs):
    key = ("row", T, H, W, n, vs)
    if key not in _cache:
        g = gen(T, H, W, n, DYN_SETS.index(vs))
        lg = torch.randn(n, T, H, W, generator=g) * (8.0 if vs == "scaled" else 1.0)
        lg[n - 1] = -lg[n - 1].abs() - 0.5                                              # a blank row
        _cache[key] = dict(logits=lg, ref=stats_eval(lg.double(), F64), bounds=stats_bounds(lg.double(), torch.zeros(n, T, H, W, dtype=F64)))
    return _cache[key]


# ---- clip_finalize --------------------------------------------------------------------------------------------------------------
FIN_THR = 0.25
FIN_CASES = [(16, 1, 4, (1, 0, 5)), (64, 5, 8, (33, 2, 1)), (256, 3, 4, (256,)), (40, 25, 64, (7, 33))]                  # (Q, K, C, counts)
FIN_KINDS = ("random", "exact", "none above", "none alive")


def fin_eval(c, dt, mut=None):
    """Per clip dict(n_sel, sel [n_sel] (instance rows), out [n_sel, 2 + K + C], values [n, K], best, alive)."""
    out, thr = [], f32(c["thr"])
    for b, n in enumerate(c["counts"]):
        rows = slice(c["row0"][b], c["row0"][b] + n)
        st, m = c["stats"][rows].to(dt), c["mi"][rows].to(dt)
        src = c["kept"][b, :n].long()
        v = (c["cls"][b, src].to(dt) * (1 - m)[:, None]) * (st[:, 1] / (st[:, 2] + EPS6))[:, None]
        best, lab = v.max(-1) if n else (torch.zeros(0, dtype=dt), torch.zeros(0, dtype=torch.long))
        alive = (st[:, 0] > 0) & (m < 0.5)
        above = alive & ((best >= thr) if mut == "best >= thr in the final count" else (best > thr))
        k = min(max(int(above.sum()), 1), int(alive.sum()))
        sc = torch.where(alive, best, torch.full_like(best, -1.0))
        o = torch.argsort(sc, descending=True, stable=True)[:k]
        out.append(dict(n_sel=k, sel=c["row0"][b] + o, values=v, best=best, alive=alive, lab=lab, order=o,
                        out=torch.cat([sc[o, None], lab[o, None].to(dt), v[o], c["emb"][b, src[o]].to(dt)], 1)))
    return out


def fin_case(Q, K, C, counts, kind):
    key = ("fin", Q, K, C, counts, kind)
    if key not in _cache:
        g = gen(Q, K, C, len(counts), FIN_KINDS.index(kind))
        B, rows = len(counts), sum(counts)
        cls, emb = torch.rand(B, Q, K, generator=g) * 0.9 + 0.05, torch.randn(B, Q, C, generator=g)
        kept = torch.stack([torch.randperm(Q, generator=g) for _ in range(B)]).int()
        den = torch.randint(1, 500, (rows,), generator=g).float()
        stats = torch.stack([torch.ones(rows), den * (0.5 + 0.5 * torch.rand(rows, generator=g)), den, torch.rand(rows, generator=g) * 90,
                             torch.randint(0, 90, (rows,), generator=g).float()], 1)
        mi = torch.rand(rows, generator=g) * 0.6
        if kind != "random":                                   # both factors exactly 1: the value is the class score, every decision is on inputs
            mi[:] = 0.0
            stats[:, 2] = 0.0                                   # (0 + 1e-6f is exact, so the quotient is exactly 1 in fp32 and in float64)
            stats[:, 1] = EPS6
            cls = (cls * 64).round() / 64                       # many equal scores: ties go by rank
        thr = FIN_THR
        for b, n in enumerate(counts):
            r0 = sum(counts[:b])
            src = kept[b, :n].long()
            if kind == "exact" and n >= 5:
                cls[b, src[0], :] = thr                          # a score exactly at thr does not count
                mi[r0 + 1] = 0.5                                 # suppressed: 0.5 is not < 0.5
                mi[r0 + 2] = f32(0.5 - 2.0 ** -25)               # just below: alive (its value is no multiple of 1/64: it ties with nothing)
                cls[b, src[2], :] = 0.9
                stats[r0 + 3, 0] = 0.0                           # blank
                cls[b, src[4], :] = 0.0
                cls[b, src[4], K - 1] = 0.75
            if kind == "none above":
                cls[b] = cls[b] * 0.25                           # nothing above thr: exactly one row is selected
            if kind == "none alive":
                stats[r0:r0 + n, 0] = (torch.arange(n) % 2 == 0).float()
                mi[r0:r0 + n] = torch.where(torch.arange(n) % 2 == 0, torch.tensor(0.5), torch.tensor(0.0))
        c = dict(Q=Q, K=K, C=C, counts=counts, row0=[sum(counts[:b]) for b in range(B)], cls=cls, emb=emb, kept=kept, stats=stats, mi=mi,
                 thr=thr, exact=kind != "random")
        c["ref"] = fin_eval(c, F64)
        und = tot = 0
        for r in c["ref"]:                                     # the decisions this case asks for, and how many the margin rule leaves open
            bv = 5 * U * r["values"].abs()
            if r["values"].numel() and not c["exact"]:         # (the exact kinds' values are the fp32 inputs themselves: ties are meant)
                und += int((~contenders(r["values"], bv)[2]).sum())
                bb = bv.gather(1, r["lab"][:, None])[:, 0]
                und += int((~threshold(r["best"], f32(thr), bb)[1] & r["alive"]).sum())
                a = r["best"][r["alive"]].sort(descending=True)
                ba = bb[r["alive"]][a.indices]
                und += int(((a.values[:-1] - a.values[1:]) <= ba[:-1] + ba[1:]).sum())
                tot += 3 * r["values"].shape[0]
        c["undecided"], c["decisions"] = und, tot
        _cache[key] = c
    return _cache[key]


def fin_verify(c, n_sel, sel, out):
    """n_sel [B], sel [rows], out [rows, 2 + K + C]; rows past n_sel[b] of a clip are the caller's to check."""
    res, K = {}, c["K"]
    for b, r in enumerate(c["ref"]):
        what = f"clip_finalize clip {b}"
        k, r0 = r["n_sel"], c["row0"][b]
        need(int(n_sel[b]) == k, f"{what}: n_sel {int(n_sel[b])} != {k}")
        need((sel[r0:r0 + k].long() == r["sel"]).all(), f"{what}: sel")
        o = out[r0:r0 + k].double()
        need((o[:, 1] == r["out"][:, 1]).all(), f"{what}: labels")
        need((o[:, 2 + K:] == r["out"][:, 2 + K:]).all(), f"{what}: embeddings")
        ref = torch.cat([r["out"][:, :1], r["out"][:, 2:2 + K]], 1)
        need_within(res, "values", torch.cat([o[:, :1], o[:, 2:2 + K]], 1), ref, 5 * U * ref.abs(), what)
    return res


# ---- image_mask_stats, image_final_masks ----------------------------------------------------------------------------------------
IMG_CASES = [(16, 24, 4, 60, 90, 120, 180), (16, 24, 4, 64, 96, 64, 96), (8, 12, 4, 30, 45, 17, 23), (5, 7, 1, 5, 6, 11, 9),
             (6, 5, 2, 11, 9, 7, 30), (3, 4, 8, 21, 30, 40, 13)]                      # (Hm, Wm, factor, h, w, Ho, Wo)
IMG_SETS = ("normal", "offset")     # unit normal x 2; the same minus 3 (few pixels set)
IMG_N = 5


def aligned_bilinear(t, f, mut=None):
    """util/misc.py:485-507 on t [n, 1, Hm, Wm]: replicate-pad by one, interpolate with align_corners=True, shift by f // 2."""
    if f == 1:
        return t
    h, w = t.shape[-2:]
    t = F.interpolate(F.pad(t, (0, 1, 0, 1), mode="replicate"), size=(f * h + 1, f * w + 1), mode="bilinear", align_corners=True)
    if mut != "aligned_bilinear without the shift":
        t = F.pad(t, (f // 2, 0, f // 2, 0), mode="replicate")
    return t[:, :, :f * h, :f * w]


def box_of(bits):
    """bits [h, w] -> (xmin, ymin, xmax, ymax), inclusive; (w, h, -1, -1) when empty."""
    h, w = bits.shape
    if not bool(bits.any()):
        return (w, h, -1, -1)
    ys, xs = torch.nonzero(bits.any(1))[:, 0], torch.nonzero(bits.any(0))[:, 0]
    return (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))


def img_stats_eval(lg, f, h, w, dt, mut=None):
    """lg [n, Hm, Wm] -> (the cropped up-sampled logits [n, h, w], stats [n, 6] = (num, den, xmin, ymin, xmax, ymax))."""
    up = aligned_bilinear(lg.to(dt)[:, None], f, mut)[:, 0, :h, :w]
    s = torch.sigmoid(up)
    hard = s > 0.5
    box = torch.tensor([box_of(u > 0) for u in up], dtype=dt).view(-1, 4)
    return up, torch.cat([(s * hard).flatten(1).sum(1)[:, None], hard.flatten(1).sum(1)[:, None].to(dt), box], 1)


def img_final_eval(lg, idx, f, h, w, Ho, Wo, dt, mut=None):
    """-> (resized logits [len(idx), Ho, Wo], their > 0)."""
    up = aligned_bilinear(lg.to(dt)[:, None], f)
    up = up if mut == "final masks from the uncropped map" else up[:, :, :h, :w]
    v = F.interpolate(up[idx.long()], size=(Ho, Wo), mode="bilinear", align_corners=False)[:, 0]
    return v, v > 0


def img_case(Hm, Wm, f, h, w, Ho, Wo, vs):
    key = ("img", Hm, Wm, f, h, w, Ho, Wo, vs)
    if key not in _cache:
        g = gen(Hm, Wm, f, h, w, Ho, IMG_SETS.index(vs))
        n = IMG_N
        lg = torch.randn(n, Hm, Wm, generator=g) * 2 - (3.0 if vs == "offset" else 0.0)
        lg[3] = -lg[3].abs() - 0.25                                                    # all negative: the box comes back empty
        # mask 4: only the bottom-right pixel of the crop is positive, where one source pixel weighs more there than on any other crop pixel
        wts = aligned_bilinear(torch.eye(Hm * Wm, dtype=F64).view(-1, 1, Hm, Wm), f)[:, 0, :h, :w].flatten(1)
        last = wts[:, -1].clone()
        rest = wts[:, :-1].amax(1)
        j = int((last - rest).argmax())
        corner = bool(last[j] > rest[j] + 1e-9)
        if not corner:                                         # (the replicated border: the last source pixel fills a block that ends there)
            lg[4] = -1.0
            lg[4, Hm - 1, Wm - 1] = 2.9                      # (no dyadic weight puts a pixel on zero)
        else:
            p = 0.5 * ((1 - last[j]) / last[j] + ((1 - rest[j]) / rest[j] if rest[j] > 0 else (1 - last[j]) / last[j] + 4))
            lg[4] = -1.0
            lg[4].view(-1)[j] = float(p)
        idx = torch.tensor([4, 0, 2, 2, 3, 1, 0], dtype=torch.int32)                   # permuted, repeated
        up, st = img_stats_eval(lg, f, h, w, F64)
        dv = 8 * U * aligned_bilinear(lg.double().abs()[:, None], f)[:, 0, :h, :w]
        s = torch.sigmoid(up)
        bs = sig_bound(s, dv)
        hard, hdec = threshold(s, 0.5, bs)
        pos, pdec = threshold(up, 0.0, dv)
        D = -(-h * w // 256) + 9
        bnum = (bs * (hard & hdec) + (s + bs) * ~hdec).flatten(1).sum(1) + D * U * (s * (hard | ~hdec)).flatten(1).sum(1)
        v, bits = img_final_eval(lg, idx, f, h, w, Ho, Wo, F64)
        bv = resize_bound(up[:, None], Ho, Wo, dv[:, None])[idx.long(), 0]
        _cache[key] = dict(lg=lg, f=f, h=h, w=w, Ho=Ho, Wo=Wo, idx=idx, corner=corner, up=up, stats=st, bnum=bnum, hard=hard, hdec=hdec, pos=pos,
                           pdec=pdec, bits=bits, bdec=threshold(v, 0.0, bv)[1], v=v, bv=bv)
    return _cache[key]


def img_stats_verify(c, stats):
    res, st = {}, stats.double()
    what = f"image_mask_stats {tuple(c['lg'].shape)} f={c['f']} crop {c['h']}x{c['w']}"
    need_within(res, "num", st[:, 0], c["stats"][:, 0], c["bnum"], what)
    need_interval(st[:, 1], c["hard"].flatten(1), c["hdec"].flatten(1), 1, f"{what} den")
    for k in range(st.shape[0]):
        inner, outer = box_of(c["pos"][k] & c["pdec"][k]), box_of(c["pos"][k] | ~c["pdec"][k])
        got = tuple(float(x) for x in st[k, 2:])
        ok = outer[0] <= got[0] <= inner[0] and outer[1] <= got[1] <= inner[1] and inner[2] <= got[2] <= outer[2] and inner[3] <= got[3] <= outer[3]
        need(ok, f"{what}: box of mask {k} {got} not between {inner} and {outer}")
    if c["corner"]:
        need(tuple(st[4, 2:].tolist()) == (c["w"] - 1, c["h"] - 1, c["w"] - 1, c["h"] - 1), f"{what}: the bottom-right pixel's box")
    need(tuple(st[3, 2:].tolist()) == (c["w"], c["h"], -1, -1) and float(st[3, 1]) == 0, f"{what}: the empty mask's box")
    return res


def img_final_verify(c, masks):
    what = f"image_final_masks {tuple(c['lg'].shape)} f={c['f']} crop {c['h']}x{c['w']} -> {c['Ho']}x{c['Wo']}"
    need(((masks == 0) | (masks == 1)).all(), f"{what}: not 0 / 1")
    need_bits(masks.reshape(c["bits"].shape), c["bits"], c["bdec"], what)
    flipped = masks.reshape(c["bits"].shape).bool() != c["bits"]                      # (undecided ones only, by now): |v| over its 2 b
    ratio = torch.where(flipped, c["v"].abs() / (2 * c["bv"]), torch.zeros_like(c["v"])).flatten()
    i = int(ratio.argmax())
    return {"mask bit": (float(c["v"].abs().flatten()[i]) if bool(flipped.any()) else 0.0, float(2 * c["bv"].flatten()[i]))}


# ---- how much of every case the margin rule leaves open -------------------------------------------------------------------------
def undecided_shares():
    """[(case name, undecided decisions, decisions)] over every case list above, from the float64 references alone."""
    rows = []
    for shape in QS_SHAPES:
        for vs in QS_SETS:
            d = qs_case(*shape, vs)["decided"]
            rows.append((f"query_select {shape} {vs}", int((~d).sum()), d.numel()))
    for case in ASSOC_CASES:
        for vs in ASSOC_SETS:
            d = assoc_case(*case, vs)["decided"]
            rows.append((f"clip_assoc {case} {vs}", int((~d).sum()), d.numel()))
    for case in SELECT_CASES:
        for vs in SELECT_SETS:
            ref = select_case(*case, vs)["ref"]
            rows.append((f"clip_select {case[:3]} {vs}", sum(int((~r["decided"]).sum()) for r in ref), sum(r["n_thr"] for r in ref)))
    for case in DYN_CASES:
        for vs in DYN_SETS:
            c = dyn_case(*case, vs)
            for b, sb in enumerate(c["bounds"]):
                if c["counts"][b]:
                    n = sb["hdec"].numel()
                    rows.append((f"dyn_mask_nms {case[:5]} {vs} clip {b}", int(round(sb["share"] * 2 * n)), 2 * n))
    for case in ROW_CASES:
        for vs in DYN_SETS:
            sb = row_case(*case, vs)["bounds"]
            rows.append((f"mask_row_stats {case} {vs}", int(round(sb["share"] * 2 * sb["hdec"].numel())), 2 * sb["hdec"].numel()))
    for case in FIN_CASES:
        for kind in FIN_KINDS:
            c = fin_case(*case, kind)
            rows.append((f"clip_finalize {case[:3]} {kind}", c["undecided"], max(1, c["decisions"])))
    for case in IMG_CASES:
        for vs in IMG_SETS:
            c = img_case(*case, vs)
            und = int((~c["hdec"]).sum() + (~c["pdec"]).sum())
            rows.append((f"image_mask_stats {case} {vs}", und, 2 * c["hdec"].numel()))
            rows.append((f"image_final_masks {case} {vs}", int((~c["bdec"]).sum()), c["bdec"].numel()))
    return rows
