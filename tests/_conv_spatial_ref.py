"""float64 references, per-element error bounds, launch geometry and case lists of the convolution and spatial kernels (a helper,
not a conftest): csrc/winograd.hip (mdqe_winograd_weight_f32, mdqe_conv3x3_winograd_f32), csrc/stem_conv.hip, csrc/dwconv.hip and
the small kernels of csrc/spatial.hip (stem_im2col, maxpool3x3s2, upsample_nearest_add, the generic depthwise 5x5).
tests/test_conv_spatial_ref_cpu.py shows on these cases that every bound admits the formula evaluated in float32 on the CPU and
rejects the seeded mistakes; tests/test_conv_spatial_gpu.py holds the kernels to them.  U = 2^-24 is the fp32 unit roundoff (as in
_gemm_ref).  Every bound is  constant x U x (the same formula on absolute values), times the activation's Lipschitz constant plus
its absolute error (_gemm_ref.ACT_L, ACT_A); to first order -- with at most 170 roundings behind a term the second-order part is
below 1e-5 of the bound.

WINOGRAD F(2x2, 3x3).  Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A + bias on the 4x4 input tile d at (2 ty - 1, 2 tx - 1).  The
reference is the plain float64 convolution.  The absolute-value formula is the PIPELINE on absolute values,

    Yabs = |A^T| [ sum_c (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A| + |bias|,

not conv2d(|x|, |w|): the transforms cancel (B^T d B subtracts neighbours that the direct sum never combines), so an output next to
large neighbours carries their rounding.  Being linear with non-negative coefficients, Yabs is itself a convolution -- 4x4, stride
2, one kernel per output parity -- and `wino_abs` evaluates it that way.  A term d * g passes through

    2        the two stages of the input transform (one addition or subtraction each),
    1        the rounding of U = G g G^T, computed in double and rounded once,
    1        its product,
    Cin - 1  the additions of the K = Cin accumulation, in any order (x + 0 for the plane products' zero bias is exact),
    2 + 2    the two stages of the output transform (two additions each),
    1        the bias,                                                                       constant  WINO_C(Cin) = Cin + 8,

and the weight transform by itself must satisfy |U - U64| <= U |U64| (one rounding from double).

STEM.  relu(conv7x7/s2/p3(pad(normalise(frames))) + bias), normalise = (raw - mean) / sd with the fp32-rounded mean and sd as
constants (the C ABI is handed float[3]), the canvas beyond h x w zero in normalised space.  A term passes the two roundings of
the normalisation, its product, at most 146 additions of the 147-term sum in any order, the bias and the output: (147 + 8) + 2 as
_gemm_ref counts K + 8.        constant STEM_C = 157 on conv(|xn|, |w|) + |bias|;     stem_im2col: 2 U |ref| (columns 147..159: 0).

DEPTHWISE 5x5.  Plain: bias + 25 products added one by one: a product, at most 25 additions.     constant DW_C = 27
Over the virtual ConvTranspose output (up[2i, 2j] = x tw + tb, tb elsewhere inside the image, nothing outside):
    generic kernel, tap by tap:  v = x tw + tb (2 roundings), acc += v w (2): at most 2 + 1 + 25.
    C == 256 quad kernel:        bias + tb * sum(in-bounds w) + tw * sum(w x): the tap sum's 24 additions, its product with tb, the
                                 addition to bias, the final addition: 27 on |tb| sum|w|; the product, at most 9 additions, the
                                 product with tw and the final addition: 12 on |tw| sum|w||x|.
                                                                                                 constant DW_UP2_C = 28 for both
on |bias| + |tb| sum_{in-bounds} |w| + |tw| sum |w| |x| -- which is also the tap-by-tap sum of |w| (|x tw| + |tb|).

EXACT.  Max pool.  Upsample-add: fp32(a) + fp32(b[idx]) is ONE rounding of an exact sum, so the result must equal the float32
sum bit for bit; idx = min(floor(dst * fp32(Hb / H)), Hb - 1) with the product in float32, as the kernel evaluates it.
"""
import torch
import torch.nn.functional as F

from _gemm_ref import ACT_A, ACT_L, U, act64, check_within, within  # noqa: F401  (re-exported)
from _attn_norm_ref import worst_ratio  # noqa: F401  (re-exported)

_cache = {}
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
STEM_C, DW_C, DW_UP2_C = 157, 27, 28


def WINO_C(Cin):
    return Cin + 8


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 5) * 104729 ** (i % 3) * int(v) for i, v in enumerate(key)) % (2 ** 31))


def act_any(x, act):
    """The activation in x's own precision (float32: torch's operators, an independent evaluation)."""
    if x.dtype == torch.float64 or act in (None, "none"):
        return act64(x, act)
    return {"relu": F.relu, "gelu": F.gelu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](x)


def conv_banded(x, w, stride, budget=1 << 28):
    """F.conv2d(x, w, stride=stride) without padding, in bands of output rows (the im2col of a 516 x 516 x 128 image is gigabytes)."""
    k = w.shape[2]
    OH = (x.shape[2] - k) // stride + 1
    OW = (x.shape[3] - k) // stride + 1
    rows = max(1, budget // (8 * OW * w.shape[1] * k * k))
    if rows >= OH:
        return F.conv2d(x, w, None, stride)
    return torch.cat([F.conv2d(x[:, :, r * stride:(min(r + rows, OH) - 1) * stride + k], w, None, stride) for r in range(0, OH, rows)], 2)


# ---- Winograd ---------------------------------------------------------------------------------------------------------------------
# the transforms as the kernels add them, left to right: row -> ((index, sign), ...)
BT_ROWS = (((0, 1), (2, -1)), ((1, 1), (2, 1)), ((2, 1), (1, -1)), ((1, 1), (3, -1)))
AT_ROWS = (((0, 1), (1, 1), (2, 1)), ((1, 1), (2, -1), (3, -1)))
WINO_ACTS = (None, "relu", "gelu", "sigmoid", "tanh")


def rows_matrix(rows, n=4):
    m = torch.zeros(len(rows), n, dtype=torch.float64)
    for r, row in enumerate(rows):
        for i, s in row:
            m[r, i] += s
    return m


def flip_sign(rows, r, j):
    """`rows` with the sign of term j of row r flipped (a seeded mistake)."""
    return tuple(tuple((i, -s if (rr, jj) == (r, j) else s) for jj, (i, s) in enumerate(row)) for rr, row in enumerate(rows))


def _comb(rows, v):
    out = []
    for row in rows:
        acc = None
        for i, s in row:
            acc = (v[i] if s > 0 else -v[i]) if acc is None else (acc + v[i] if s > 0 else acc - v[i])
        out.append(acc)
    return out


def wino_weight64(w, absolute=False):
    """w [Cout, 3, 3, Cin] -> G g G^T [16, Cout, Cin] in float64 (|G| |g| |G^T| when `absolute`)."""
    g = w.double().abs() if absolute else w.double()
    s = 1.0 if absolute else -1.0
    t = torch.stack([g[:, 0], 0.5 * (g[:, 0] + g[:, 1] + g[:, 2]), 0.5 * (g[:, 0] + s * g[:, 1] + g[:, 2]), g[:, 2]], 1)   # [Co, 4, 3, Ci]
    u = torch.stack([t[:, :, 0], 0.5 * (t[:, :, 0] + t[:, :, 1] + t[:, :, 2]), 0.5 * (t[:, :, 0] + s * t[:, :, 1] + t[:, :, 2]), t[:, :, 2]], 2)
    return u.permute(1, 2, 0, 3).reshape(16, w.shape[0], w.shape[3]).contiguous()


def wino_weight(w):
    """U [16, Cout, Cin] = G g G^T in double, rounded once (wino_weight_kernel)."""
    return wino_weight64(w).float()


def wino_tiles(H, W):
    return (H + 1) // 2, (W + 1) // 2


def wino_eval(x, w, b, act=None, dtype=torch.float32, bt=BT_ROWS, at=AT_ROWS, swap_ab=False, swap_tiles=False, pad="zero", bias_first=False,
              crop=True):
    """x [NI, H, W, Cin] NHWC, w [Cout, 3, 3, Cin] -> [NI, H, W, Cout] (stride 1, pad 1): the kernels' pipeline in their order of
    operations, in `dtype` (float32: the emulation of csrc/winograd.hip; float64: the same algebra, which the seeded mistakes alter).
    `crop=False` returns all [NI, 2 th, 2 tw, Cout] values the tiles produce."""
    NI, H, W, C = x.shape
    th, tw = wino_tiles(H, W)
    xp = torch.zeros(NI, 2 * th + 2, 2 * tw + 2, C, dtype=dtype)
    if pad == "replicate":
        xp[:, :H + 2, :W + 2] = F.pad(x.to(dtype).permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
    else:
        xp[:, 1:H + 1, 1:W + 1] = x.to(dtype)
    d = xp.unfold(1, 4, 2).unfold(2, 4, 2)                     # [NI, th, tw, C, 4 (row), 4 (col)]
    V = [v for r in _comb(bt, [d[..., i, :] for i in range(4)]) for v in _comb(bt, [r[..., j] for j in range(4)])]
    V = torch.stack(V, 0)                                      # [16, NI, th, tw, Cin]
    if swap_ab:
        V = V.view(4, 4, NI, th, tw, C).transpose(0, 1).reshape(16, NI, th, tw, C)
    if swap_tiles:                                             # tile r of an image read as (ty, tx) = (r % th, r / th)
        V = V.transpose(2, 3).reshape(16, NI, th, tw, C)
    Uw = wino_weight64(w)
    M = torch.bmm(V.reshape(16, -1, C), (Uw.float() if dtype == torch.float32 else Uw).transpose(1, 2))          # [16, T, Cout]
    bias = b.to(dtype) if b is not None else torch.zeros(w.shape[0], dtype=dtype)
    if bias_first:
        M = M + bias
    m = M.reshape(4, 4, NI, th, tw, -1)
    q = _comb(at, [m[i] for i in range(4)])
    y = torch.empty(NI, th, 2, tw, 2, M.shape[-1], dtype=dtype)
    for a in range(2):
        ya = _comb(at, [q[a][j] for j in range(4)])
        for bb in range(2):
            y[:, :, a, :, bb] = ya[bb] if bias_first else ya[bb] + bias
    y = act_any(y.reshape(NI, 2 * th, 2 * tw, -1), act)
    return y[:, :H, :W] if crop else y


def wino_store_unguarded(yfull, H, W, tail):
    """What the output buffer holds when the odd-edge guard of wino_output_kernel is missing and the stray store wins its race:
    yfull [NI, 2 th, 2 tw, N] stored at ((img H + oh) W + ow) for EVERY oh, ow.  Returns ([NI, H, W, N], the `tail` rows behind it)."""
    NI, H2, W2, N = yfull.shape
    flat = torch.full((NI * H * W + tail, N), float("nan"), dtype=yfull.dtype)
    img, oh, ow = torch.meshgrid(torch.arange(NI), torch.arange(H2), torch.arange(W2), indexing="ij")
    addr = (img * H + oh) * W + ow
    stray = (oh >= H) | (ow >= W)
    for sel in (~stray, stray):                                # the stray stores last
        flat[addr[sel]] = yfull[sel]
    return flat[:NI * H * W].view(NI, H, W, N), flat[NI * H * W:]


def wino_ref64(x, w, b, act):
    y = conv_banded(F.pad(x.double().permute(0, 3, 1, 2), (1, 1, 1, 1)), w.double().permute(0, 3, 1, 2), 1).permute(0, 2, 3, 1)
    return act64(y + b.double() if b is not None else y, act)


def wino_abs(x, w, b):
    """Yabs [NI, H, W, Cout] (module docstring), as one 4x4 / stride-2 convolution of |x| with 4 Cout kernels (one per output parity)."""
    NI, H, W, C = x.shape
    N = w.shape[0]
    th, tw = wino_tiles(H, W)
    Bm, Am = rows_matrix(BT_ROWS).abs(), rows_matrix(AT_ROWS).abs()
    Ua = wino_weight64(w, absolute=True).view(4, 4, N, C)
    K = torch.einsum("pa,qb,abnc,ai,bj->pqncij", Am, Am, Ua, Bm, Bm).reshape(4 * N, C, 4, 4)
    xp = torch.zeros(NI, C, 2 * th + 2, 2 * tw + 2, dtype=torch.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x.double().abs().permute(0, 3, 1, 2)
    y = conv_banded(xp, K, 2).view(NI, 2, 2, N, th, tw).permute(0, 4, 1, 5, 2, 3).reshape(NI, 2 * th, 2 * tw, N)[:, :H, :W]
    return y + b.double().abs() if b is not None else y


def wino_bound(x, w, b, act):
    return WINO_C(x.shape[3]) * U * wino_abs(x, w, b) * ACT_L[act] + ACT_A[act]


# (NI, H, W, Cin, Cout, act, bias, ldy - Cout, x image stride - H W Cin); T = NI * tiles
WINO_BIG = (1, 516, 516, 128, 4, "relu", True, 0, 0)      # one image of 562 MB of V + M: over the group budget; the input transform's grid capped
WINO_BIG_OUT = (1, 362, 362, 32, 260, "relu", True, 0, 0)  # 612 MB of V + M, mostly M: the output transform's grid capped
WINO_RAGGED = (3, 15, 17, 32, 260, "relu", True, 4, 0)    # T = 216: ragged against 32, 64 and 128 rows; N ragged against 64, 128 and 256
WINO_CASES = [
    (1, 1, 1, 32, 4, None, True, 0, 0),                   # T = 1
    (3, 2, 3, 32, 36, "relu", True, 4, 0),                # T = 6
    (1, 3, 5, 96, 64, "gelu", True, 0, 96),               # T = 6, exact N tile, padded image stride
    (3, 5, 8, 160, 100, "sigmoid", False, 64, 0),         # T = 36, no bias
    (1, 8, 5, 32, 260, "tanh", True, 4, 64),              # T = 12
    (3, 1, 8, 96, 4, None, False, 64, 32),                # T = 12: H = 1
    (1, 5, 1, 160, 36, "relu", True, 0, 0),               # T = 3: W = 1
    (3, 8, 2, 32, 100, "gelu", True, 4, 0),               # T = 12
    (3, 3, 3, 96, 260, None, True, 0, 0),                 # T = 12
    (1, 2, 2, 160, 64, "tanh", True, 64, 0),              # T = 1, even sizes
    (1, 16, 16, 32, 64, "sigmoid", True, 0, 0),           # T = 64: exact M and N tiles
    WINO_RAGGED, WINO_BIG, WINO_BIG_OUT,
]
WINO_TILES = (1, 2, 3, 4, 5, 7, 8, 9)                     # every code mdqe_launch_gemm_k16 takes for a plane batch
WINO_WEIGHTS = [(4, 32), (36, 96), (260, 4064)]           # (Cout, Cin) of the weight transform alone; the last: over 4096 blocks
GROUP_BYTES = 128 << 20


def wino_case(geom):
    """dict(x, w, b, ref, bound) of one geometry, computed once (callers must not modify it)."""
    key = ("wino",) + tuple(geom)
    if key not in _cache:
        NI, H, W, Cin, Cout, act, bias = geom[:7]
        g = _gen(NI, H, W, Cin, Cout)
        x = torch.randn(NI, H, W, Cin, generator=g)
        w = torch.randn(Cout, 3, 3, Cin, generator=g) / (9 * Cin) ** 0.5
        b = torch.randn(Cout, generator=g) if bias else None
        _cache[key] = dict(x=x, w=w, b=b, ref=wino_ref64(x, w, b, act), bound=wino_bound(x, w, b, act))
    return _cache[key]


def wino_geometry(geom):
    """The launcher's arithmetic (mdqe_conv3x3_winograd_f32): images per group, rows T of the first group's plane products, and how
    often a block of each transform's grid-stride loop runs."""
    NI, H, W, Cin, Cout = geom[:5]
    th, tw = wino_tiles(H, W)
    per_img = 16 * th * tw * (Cin + Cout) * 4
    group = min(NI, max(1, GROUP_BYTES // per_img))
    T = group * th * tw
    return dict(per_img=per_img, group=group, ngroups=-(-NI // group), T=T, loops_in=grid_loops(T * (Cin // 4), 256, 8192),
                loops_out=grid_loops(T * (Cout // 4), 256, 8192))


def grid_loops(items, per_block, cap):
    """{how many times a block's grid-stride loop runs}, over the blocks of min(ceil(items / per_block), cap) blocks."""
    nb = min(-(-items // per_block), cap)
    step = nb * per_block
    return {-(-(items - first) // step) for first in (0, step - 1) if first < items}


# ---- stem -------------------------------------------------------------------------------------------------------------------------
def stem_norm(frames, dtype=torch.float64):
    mean, std = (torch.tensor(t, dtype=torch.float32).to(dtype).view(1, 3, 1, 1) for t in (MEAN, STD))
    return (frames.to(dtype) - mean) / std


def stem_ref(frames, Hp, Wp, w, b, dtype=torch.float64, pad=3, canvas_raw_zero=False, channels=(0, 1, 2), prev_tile=False):
    """frames [NI, 3, h, w]; w [64, 7, 7, 3]; -> NHWC [NI, Hp / 2, Wp / 2, 64].  The keywords are the seeded mistakes."""
    NI, _, h, wd = frames.shape
    xn = stem_norm(frames, dtype)[:, list(channels)]
    if canvas_raw_zero:                                          # the canvas normalised as (0 - mean) / sd
        xn = stem_norm(F.pad(frames.to(dtype), (0, Wp - wd, 0, Hp - h)), dtype)
    else:
        xn = F.pad(xn, (0, Wp - wd, 0, Hp - h))
    y = F.conv2d(F.pad(xn, (pad, 6 - pad, pad, 6 - pad)), w.to(dtype).permute(0, 3, 1, 2), b.to(dtype), 2)[:, :, :Hp // 2, :Wp // 2]
    y = torch.relu(y).permute(0, 2, 3, 1)
    if prev_tile:                                                # tile i holds what tile i - 1's patch gives
        OH, OW = Hp // 2, Wp // 2
        ty, tx = -(-OH // 8), -(-OW // 16)
        t = F.pad(y, (0, 0, 0, tx * 16 - OW, 0, ty * 8 - OH)).view(NI, ty, 8, tx, 16, 64).permute(0, 1, 3, 2, 4, 5).reshape(-1, 8, 16, 64)
        y = t.roll(1, 0).view(NI, ty, tx, 8, 16, 64).permute(0, 1, 3, 2, 4, 5).reshape(NI, ty * 8, tx * 16, 64)[:, :OH, :OW]
    return y.contiguous()


def stem_bound(frames, Hp, Wp, w, b):
    xn = stem_norm(frames).abs()
    xn = F.pad(xn, (3, 3 + Wp - frames.shape[3], 3, 3 + Hp - frames.shape[2]))
    P = F.conv2d(xn, w.double().abs().permute(0, 3, 1, 2), b.double().abs(), 2)[:, :, :Hp // 2, :Wp // 2]
    return (STEM_C * U * P).permute(0, 2, 3, 1).contiguous()


def im2col_ref(frames, Hp, Wp, dtype=torch.float64):
    """[NI * Hp/2 * Wp/2, 160]: k = (kh, kw, c), columns 147..159 zero."""
    NI, _, h, w = frames.shape
    xn = F.pad(stem_norm(frames, dtype), (3, 3 + Wp - w, 3, 3 + Hp - h))
    col = F.unfold(xn, 7, stride=2)[:, :, :]                     # [NI, 3 * 49 (c, kh, kw), L]
    OH, OW = Hp // 2, Wp // 2
    L_w = (Wp + 6 - 7) // 2 + 1
    col = col.view(NI, 3, 49, -1, L_w)[:, :, :, :OH, :OW].permute(0, 3, 4, 2, 1).reshape(-1, 147)
    return F.pad(col, (0, 13))


# (NI, h, w, Hp, Wp, u8, frame stride - 3 h w)
STEM_CASES = [
    (130, 47, 66, 50, 70, True, 0),                              # 1560 tiles: blocks walk 3 and 2
    (70, 47, 66, 50, 70, False, 8),                              # 840 tiles: the float kernel's blocks walk 2 and 1
    (2, 47, 66, 50, 70, False, 0),                               # float frames with fractions; ragged tiles on both axes
    (1, 16, 32, 16, 32, True, 0),                                # one tile, exact
    (2, 1, 1, 2, 2, True, 5),                                    # h = w = 1; padded frame stride
    (3, 1, 9, 4, 10, False, 8), (2, 9, 1, 10, 2, True, 0),
    (2, 13, 31, 16, 34, False, 64),
]
IM2COL_CASES = [(3, 261, 263, 264, 266, True, 0), (2, 5, 7, 6, 8, False, 4), (1, 1, 1, 2, 2, True, 0)]     # 52 668 rows; tiny


def stem_frames(NI, h, w, u8):
    g = _gen(NI, h, w, int(u8), 23)
    f = torch.randint(0, 256, (NI, 3, h, w), generator=g, dtype=torch.uint8)
    return f if u8 else f.float() + torch.rand(NI, 3, h, w, generator=g)


def stem_weights():
    if "stemw" not in _cache:
        g = _gen(64, 7, 7, 3)
        _cache["stemw"] = (torch.randn(64, 7, 7, 3, generator=g) / 12, torch.randn(64, generator=g))
    return _cache["stemw"]


def stem_case(geom):
    key = ("stem",) + tuple(geom)
    if key not in _cache:
        NI, h, w, Hp, Wp, u8 = geom[:6]
        f = stem_frames(NI, h, w, u8)
        wt, b = stem_weights()
        _cache[key] = dict(frames=f, w=wt, b=b, ref=stem_ref(f, Hp, Wp, wt, b), bound=stem_bound(f, Hp, Wp, wt, b))
    return _cache[key]


def stem_geometry(geom):
    NI, h, w, Hp, Wp = geom[:5]
    OH, OW = Hp // 2, Wp // 2
    tx, ty = -(-OW // 16), -(-OH // 8)
    ntiles = NI * tx * ty
    return dict(ntiles=ntiles, loops=grid_loops(ntiles, 1, 768), ragged=(OH % 8 != 0, OW % 16 != 0))


def im2col_geometry(geom):
    NI, h, w, Hp, Wp = geom[:5]
    rows = NI * (Hp // 2) * (Wp // 2)
    return dict(rows=rows, loops=grid_loops(rows * 40, 256, 4096))


# ---- depthwise 5x5 ------------------------------------------------------------------------------------------------------------------
def dw_taps(x, wt, transpose=False):
    """sum over the 25 taps of x [NI, H, W, C] (zero outside) times wt [25, C] (tap kh * 5 + kw), NHWC."""
    NI, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 2, 2, 2, 2))
    acc = torch.zeros_like(x)
    for kh in range(5):
        for kw in range(5):
            acc += xp[:, kh:kh + H, kw:kw + W] * wt[(kw * 5 + kh) if transpose else (kh * 5 + kw)]
    return acc


def up2_virtual(x, tw, tb, parity=0):
    NI, Hs, Ws, C = x.shape
    up = tb.expand(NI, 2 * Hs, 2 * Ws, C).clone()
    up[:, parity::2, parity::2] = x * tw + tb
    return up


def dw_ref(x, wt, bias, up2=False, tw=None, tb=None, dtype=torch.float64, transpose=False, parity=0, tb_outside=False, interior_bottom_right=False):
    """Depthwise 5x5 of x (or of its virtual ConvTranspose output when `up2`); the last four keywords are the seeded mistakes."""
    x, wt, bias = x.to(dtype), wt.to(dtype), bias.to(dtype)
    if not up2:
        return dw_taps(x, wt, transpose) + bias
    tw, tb = tw.to(dtype), tb.to(dtype)
    y = dw_taps(up2_virtual(x, tw, tb, parity), wt, transpose) + bias
    if tb_outside or interior_bottom_right:                      # tb also at taps outside the image: the interior constant
        z = torch.zeros_like(tb)
        wrong = dw_taps(up2_virtual(x, tw, z, parity), wt, transpose) + bias + tb * wt.sum(0)
        if tb_outside:
            return wrong
        NI, H, W, C = y.shape                                    # only the quads of the last row / column of quads forget their border
        sel = torch.zeros(H, W, dtype=torch.bool)
        sel[H - 2:, :] = True
        sel[:, W - 2:] = True
        sel[:2, :] = False
        sel[:, :2] = False
        y = torch.where(sel[None, :, :, None], wrong, y)
    return y


def dw_bound(x, wt, bias, up2=False, tw=None, tb=None):
    x, wt, bias = x.double().abs(), wt.double().abs(), bias.double().abs()
    if not up2:
        return DW_C * U * (dw_taps(x, wt) + bias)
    return DW_UP2_C * U * (dw_taps(up2_virtual(x, tw.double().abs(), tb.double().abs()), wt) + bias)


# (kernel, NI, H, W, C, up2): H, W are the INPUT sizes (the output of an up2 case is 2H x 2W)
DW_SMALL = [(1, 1), (1, 7), (7, 1), (2, 3), (5, 8)]
DW_CASES = ([("c256", 2, H, W, 256, False) for H, W in DW_SMALL] + [("c256", 2, 100, 165, 256, False)]
            + [("quad", 2, H, W, 256, True) for H, W in DW_SMALL] + [("quad", 2, 91, 91, 256, True)]
            + [("generic", 2, H, W, C, up2) for (H, W), C in zip(DW_SMALL, (4, 32, 252, 32, 252)) for up2 in (False, True)]
            + [("generic", 3, 3, 4, 4, True), ("generic", 2, 92, 91, 252, True)])


def dw_case(geom):
    key = ("dw",) + tuple(geom)
    if key not in _cache:
        kernel, NI, H, W, C, up2 = geom
        g = _gen(NI, H, W, C, int(up2), len(kernel))
        x = torch.randn(NI, H, W, C, generator=g)
        wt = torch.randn(25, C, generator=g) / 5
        bias = torch.randn(C, generator=g) * 4                   # bias and tb large beside w * x: a wrong constant shows
        tw, tb = (torch.randn(C, generator=g), torch.randn(C, generator=g) * 4) if up2 else (None, None)
        _cache[key] = dict(x=x, wt=wt, bias=bias, tw=tw, tb=tb, ref=dw_ref(x, wt, bias, up2, tw, tb), bound=dw_bound(x, wt, bias, up2, tw, tb))
    return _cache[key]


def dw_geometry(geom):
    """Work items, loop counts and how many work items are border-only / interior."""
    kernel, NI, H, W, C, up2 = geom
    if kernel == "c256":
        items = NI * H * ((W + 1) // 2)
        return dict(items=items, loops=grid_loops(items, 4, 2048), odd_w=W % 2 == 1, interior=H > 4 and W > 5)
    if kernel == "quad":
        items = NI * H * W
        return dict(items=items, loops=grid_loops(items, 4, 2048), interior=H > 2 and W > 2, both_borders=H == 1 or W == 1)
    OH, OW = (2 * H, 2 * W) if up2 else (H, W)
    items = NI * OH * OW * (C // 4)
    return dict(items=items, loops=grid_loops(items, 256, 8192), interior=OH > 4 and OW > 4)


# ---- max pool, upsample-add ---------------------------------------------------------------------------------------------------------
def maxpool_ref(x, init=float("-inf"), shift=0):
    """x [NI, H, W, C] float32 -> 3x3 / stride 2 / pad 1 max, exact.  `init`, `shift`: the seeded mistakes."""
    NI, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xp = F.pad(x, (0, 0, 1 - shift, 2 + shift, 1 - shift, 2 + shift), value=float("-inf"))
    win = xp.unfold(1, 3, 2).unfold(2, 3, 2)[:, :OH, :OW]        # [NI, OH, OW, C, 3, 3]
    return win.amax((-1, -2)).clamp_min(init)


# (NI, H, W, C, negative)
POOL_CASES = [(2, 1, 1, 4, True), (1, 2, 3, 64, False), (2, 3, 4, 4, True), (1, 4, 2, 64, True), (2, 31, 48, 64, False), (1, 48, 31, 4, True),
              (1, 3, 1, 4, False), (2, 513, 513, 64, False)]   # the last: 2.1 M work items, over 4096 blocks twice


def pool_case(geom):
    key = ("pool",) + tuple(geom)
    if key not in _cache:
        NI, H, W, C, neg = geom
        x = torch.randn(NI, H, W, C, generator=_gen(NI, H, W, C, 31))
        x = -x.abs() - 0.5 if neg else x
        _cache[key] = dict(x=x, ref=maxpool_ref(x))
    return _cache[key]


def pool_geometry(geom):
    NI, H, W, C = geom[:4]
    items = NI * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1) * (C // 4)
    return dict(items=items, loops=grid_loops(items, 256, 4096))


def up_index(n, nb, rounding=torch.floor):
    """min(floor(dst * fp32(nb / n)), nb - 1) with the scale and the product in float32 (upsample_add_kernel)."""
    s = torch.tensor(float(nb), dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    return rounding(torch.arange(n, dtype=torch.float32) * s).long().clamp_max(nb - 1)


def upsample_add_ref(a, b, rounding=torch.floor):
    """a [NI, H, W, C] + b [NI, Hb, Wb, C][idx], in float32: exact up to the one rounding the kernel makes too."""
    ih, iw = up_index(a.shape[1], b.shape[1], rounding), up_index(a.shape[2], b.shape[2], rounding)
    return a + b[:, ih][:, :, iw]


# (NI, H, W, Hb, Wb, C)
UP_CASES = [(2, 6, 10, 3, 5, 32), (1, 45, 23, 23, 12, 4), (2, 15, 20, 7, 9, 32), (2, 1, 5, 1, 5, 4), (1, 23, 45, 12, 23, 32), (3, 20, 15, 9, 7, 4),
            (1, 363, 363, 182, 182, 64)]                       # the last: 2.1 M work items


def up_case(geom):
    key = ("up",) + tuple(geom)
    if key not in _cache:
        NI, H, W, Hb, Wb, C = geom
        g = _gen(NI, H, W, Hb, Wb, C)
        a, b = torch.randn(NI, H, W, C, generator=g), torch.randn(NI, Hb, Wb, C, generator=g)
        _cache[key] = dict(a=a, b=b, ref=upsample_add_ref(a, b))
    return _cache[key]


def up_geometry(geom):
    NI, H, W, Hb, Wb, C = geom
    items = NI * H * W * (C // 4)
    return dict(items=items, loops=grid_loops(items, 256, 4096))
