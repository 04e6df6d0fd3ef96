"""Host wrappers over the C ABI (include/mdqe_hip.h): torch owns memory + stream, HIP does the math.

All tensors are CUDA fp32 contiguous unless stated; images are NHWC.  Nothing here falls back to
torch arithmetic: a missing library or an unsupported shape raises.
"""
import contextlib
import os
import threading

import torch

from ._lib import check, cur_stream, lib, ptr, raw_stream

ACT = {"none": 0, None: 0, "relu": 1, "gelu": 2, "sigmoid": 3, "tanh": 4}

if os.environ.get("MDQE_MSDA_VARIANT"):                 # tools/ A/B of the fused MSDA's block-to-query map (csrc/msda_fused.hip)
    check(lib.mdqe_debug_msda_variant(int(os.environ["MDQE_MSDA_VARIANT"])), "msda_variant")

if os.environ.get("MDQE_MSDA_DEC_STAGED"):              # tools/ A/B: decoder box-level MSDA on the LDS-staged kernel (1, default) or v2 (0)
    check(lib.mdqe_debug_msda_dec_staged(int(os.environ["MDQE_MSDA_DEC_STAGED"])), "msda_dec_staged")

if os.environ.get("MDQE_GEMM_TILE_RULE"):               # tools/ A/B of the auto tile rule (csrc/gemm_api.hip dispatch_gemm)
    check(lib.mdqe_debug_gemm_tile_rule(int(os.environ["MDQE_GEMM_TILE_RULE"])), "gemm_tile_rule")
if os.environ.get("MDQE_GEMM_STAGGER"):                 # tools/ A/B: start stagger between the blocks of a CU (csrc/gemm_k16.hip), 10-ns ticks
    check(lib.mdqe_debug_gemm_stagger(int(os.environ["MDQE_GEMM_STAGGER"])), "gemm_stagger")

if os.environ.get("MDQE_MSDA_DEC_STAGE_KB"):           # tools/ A/B: LDS staging budget (KB) of the decoder's box-level deformable launch
    check(lib.mdqe_debug_msda_dec_stage_kb(int(os.environ["MDQE_MSDA_DEC_STAGE_KB"])), "msda_dec_stage_kb")
if os.environ.get("MDQE_MSDA_TP_STAGED"):              # tools/ A/B: 0 = the decoder's temporal launch on the gather form (no LDS staging)
    check(lib.mdqe_debug_msda_tp_staged(int(os.environ["MDQE_MSDA_TP_STAGED"])), "msda_tp_staged")
if os.environ.get("MDQE_GEMM_LDS_PAD"):                # tools/ A/B: extra LDS bytes per K-step-16 GEMM block (caps the GEMM blocks per CU)
    check(lib.mdqe_debug_gemm_lds_pad(int(os.environ["MDQE_GEMM_LDS_PAD"])), "gemm_lds_pad")
if os.environ.get("MDQE_WINOGRAD_TILE"):               # tools/ A/B: K-step-16 tile code of the Winograd plane products (csrc/winograd.hip)
    check(lib.mdqe_debug_winograd_tile(int(os.environ["MDQE_WINOGRAD_TILE"])), "winograd_tile")

_ws = {}


GEMM_MODES = {"f32": 0, "f16x3": 1, "f16": 2}


def set_gemm_precision(mode):
    """'f32' (exact fp32 MFMA), 'f16x3' (split-precision f16 MFMA, ~1e-6 rel. to fp32) or 'f16' (ONE f16 MFMA pass, operands rounded to
    nearest f16, fp32 accumulate / out: the reference's autocast arithmetic) for the large-tile GEMM/conv."""
    check(lib.mdqe_set_gemm_precision(GEMM_MODES[mode]), "set_gemm_precision")


def get_gemm_precision():
    """The mode this thread's launches use (its `gemm_precision` region if inside one, else the process-wide mode)."""
    return {v: k for k, v in GEMM_MODES.items()}[lib.mdqe_get_gemm_precision()]


_tl_prec = threading.local()


@contextlib.contextmanager
def gemm_precision(mode):
    """`with gemm_precision("f16x3"):` -- the GEMM mode of the CALLING thread's launches inside the block (C ABI
    mdqe_set_gemm_precision_thread); nests; other host threads and the process-wide mode are untouched."""
    prev = getattr(_tl_prec, "v", -1)
    cur = GEMM_MODES[mode]
    check(lib.mdqe_set_gemm_precision_thread(cur), "set_gemm_precision_thread")
    _tl_prec.v = cur
    try:
        yield
    finally:
        check(lib.mdqe_set_gemm_precision_thread(prev), "set_gemm_precision_thread")
        _tl_prec.v = prev


# ---- constant weights: pre-split f16 planes for the f16x3 mode (gemm_f16x3w.hip) ---------------------
_split = {}          # data_ptr -> (weakref to the weight tensor, its _version, planes tensor)


def const_weight(w):
    """Declare `w` ([N, ...] CUDA fp32, contiguous) a constant GEMM/conv weight: its f16 hi / lo planes are computed
    once and handed to the kernels as `w_split`.  Returns w.  Tensors the fast kernel cannot take are left alone."""
    import weakref
    if not (torch.is_tensor(w) and w.is_cuda and w.dtype == torch.float32 and w.dim() >= 2 and w.is_contiguous()):
        return w
    N = w.shape[0]
    K = w.numel() // max(N, 1)
    if N < 128 or K % 32 != 0 or float(w.abs().max()) >= 32752.0:
        return w
    planes = torch.empty(3 * w.numel(), dtype=torch.float16, device=w.device)     # hi | lo (f16x3) | round-to-nearest (f16)
    check(lib.mdqe_f16x3_split_f32(ptr(w), w.numel(), ptr(planes), cur_stream()), "f16x3_split")
    key = w.data_ptr()
    _split[key] = (weakref.ref(w), w._version, planes)
    weakref.finalize(w, _drop_split, key)               # the planes go when the weight tensor goes
    return w


def _drop_split(key):
    ent = _split.get(key)
    if ent is not None and ent[0]() is None:            # (a newer tensor may have been registered at the same address)
        del _split[key]


def _wsplit(w):
    ent = _split.get(w.data_ptr())
    if ent is None:
        return None
    ref, ver, planes = ent
    base = ref()
    if base is None or base._version != ver:         # freed (the address may be reused) or modified in place
        del _split[w.data_ptr()]
        return None
    if w.numel() != base.numel() or w._version != ver or not w.is_contiguous():
        return None                                  # some other tensor at the same address (a partial view): not ours
    return planes                                    # w is the registered tensor or a full reshaped view of it


# ---- constant 3x3 weights: Winograd F(2x2,3x3) transforms for the stride-1 convs (csrc/winograd.hip) ----------
WINOGRAD = os.environ.get("MDQE_WINOGRAD", "1") != "0"     # 0: every 3x3 conv on the direct implicit GEMM (A/B in one process: set ops.WINOGRAD)
_wino = {}           # data_ptr -> (weakref to the packed weight, its _version, U [16, Cout, Cin])


def winograd_weight(w):
    """Declare `w` (packed [Cout, 3, 3, Cin] CUDA fp32, contiguous) a constant weight of stride-1 3x3 convs: its Winograd
    transform U = G g G^T is computed once, and `conv2d_nhwc` then runs the exact-fp32 mode's stride-1, pad-1 launches of it as
    F(2x2,3x3).  Returns w.  Weights the Winograd path cannot take (Cin < 128, Cin % 32, Cout % 4, Cout > 1024) are left alone."""
    import weakref
    if not (torch.is_tensor(w) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and w.is_contiguous()):
        return w
    Cout, KH, KW, Cin = w.shape
    if KH != 3 or KW != 3 or Cin < 128 or Cin % 32 != 0 or Cout % 4 != 0 or Cout > 1024:
        return w
    U = torch.empty((16, Cout, Cin), dtype=torch.float32, device=w.device)
    check(lib.mdqe_winograd_weight_f32(ptr(w), Cout, Cin, ptr(U), cur_stream()), "winograd_weight_f32")
    key = w.data_ptr()
    _wino[key] = (weakref.ref(w), w._version, U)
    weakref.finalize(w, _drop_wino, key)                # U goes when the weight tensor goes
    return w


def _drop_wino(key):
    ent = _wino.get(key)
    if ent is not None and ent[0]() is None:
        del _wino[key]


def _wino_u(w):
    """U of a registered weight (None: not registered, freed, modified in place, or another tensor at the same address)."""
    ent = _wino.get(w.data_ptr())
    if ent is None:
        return None
    ref, ver, U = ent
    base = ref()
    if base is None or base._version != ver:
        del _wino[w.data_ptr()]
        return None
    if w.shape != base.shape or w._version != ver or not w.is_contiguous():
        return None
    return U


def _workspace(nbytes, device):
    """Scratch buffer (split-K partials, GroupNorm statistics), one per (device, stream): the per-frame stages and the
    per-clip stages run on different streams and must not share it."""
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, raw_stream(dev))
    t = _ws.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = t
    return t


def _chk(t, name, dtype=torch.float32):
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected contiguous CUDA {dtype} tensor, got {t.dtype} {t.device} "
                           f"contiguous={t.is_contiguous()}")


def linear(x, weight, bias=None, act=None, residual=None, res_mod=0, rowmask=None, mask_cols=0, act_cols=0,
           out=None, ldc=None, tile=0, res_first=False, ksplit=0):
    """out[..., n] = epilogue(x[..., :] @ weight[n, :]).  x may be a 2-D row-strided view (last dim contiguous)."""
    K = x.shape[-1]
    N = weight.shape[0]
    if x.dim() != 2:
        x2 = x.reshape(-1, K)
    else:
        x2 = x
    if x2.stride(-1) != 1:
        raise RuntimeError("linear: last dim of x must be contiguous")
    M = x2.shape[0]
    lda = x2.stride(0) if M > 1 else K
    _chk(weight, "weight"); _chk(bias, "bias")
    if rowmask is not None and rowmask.dtype == torch.bool:
        rowmask = rowmask.view(torch.uint8)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
        ldc_ = N
    else:
        ldc_ = ldc if ldc is not None else out.stride(0) if out.dim() == 2 else N
    ldr = 0
    if residual is not None:
        ldr = residual.stride(0) if residual.dim() == 2 else residual.shape[-1]
    ws = None
    # (no automatic split-K here: a split changes the order of a row's K sum, and which arithmetic a row gets must not depend on
    # how many rows share its launch -- the schedule tests demand identical bits across pass sizes; callers pass ksplit explicitly)
    if ksplit > 1:
        ws = _workspace(ksplit * M * N * 4 + 64, x.device)
    check(lib.mdqe_gemm_nt_f32(ptr(x2), lda, ptr(weight), ptr(bias), ptr(out), ldc_, M, N, K, ACT[act], act_cols,
                               ptr(residual), ldr, res_mod, int(res_first), ptr(rowmask), mask_cols, tile, ksplit, ptr(ws),
                               ptr(_wsplit(weight)), cur_stream()), "gemm_nt_f32")
    if x.dim() != 2 and ldc is None and out.dim() == 2 and out.shape == (M, N):
        return out.view(*x.shape[:-1], N)
    return out


def conv2d_nhwc(x, w_packed, bias=None, stride=1, pad=0, act=None, residual=None, out=None, tile=0, res_first=False, ksplit=0):
    """x [NI,H,W,Cin] (dense, or a view whose images are x.stride(0) apart with dense pixels);
    w_packed [Cout,KH,KW,Cin]; returns [NI,OH,OW,Cout]."""
    _chk(w_packed, "w"); _chk(bias, "bias"); _chk(residual, "residual")
    NI, H, W, Cin = x.shape
    if not (x.is_cuda and x.dtype == torch.float32 and x.stride(3) == 1 and x.stride(2) == Cin and x.stride(1) == W * Cin):
        raise RuntimeError("conv2d_nhwc: x must be CUDA fp32 NHWC with dense pixels")
    xis = x.stride(0) if NI > 1 else 0
    Cout, KH, KW, _ = w_packed.shape
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    if out is None:
        out = torch.empty((NI, OH, OW, Cout), dtype=torch.float32, device=x.device)
    ldy = out.stride(-2)
    ldr = residual.stride(-2) if residual is not None else 0
    M, K = NI * OH * OW, KH * KW * Cin
    if (WINOGRAD and KH == 3 and KW == 3 and stride == 1 and pad == 1 and residual is None and tile == 0 and ksplit == 0
            and Cin >= 128 and Cin % 32 == 0 and lib.mdqe_get_gemm_precision() == 0):
        U = _wino_u(w_packed)
        # (the Winograd entry point takes 16-byte aligned operands and row pitches only; anything else keeps the direct kernel, which
        # handles unaligned ones)
        aligned = ((x.data_ptr() | out.data_ptr() | (bias.data_ptr() if bias is not None else 0)) & 15) == 0 and ldy % 4 == 0 and xis % 4 == 0
        if U is not None and aligned:                    # F(2x2,3x3): 2.25x fewer matrix multiplies (csrc/winograd.hip)
            nb = lib.mdqe_winograd_workspace_bytes(NI, H, W, Cin, Cout)
            ws = _workspace(nb, x.device)
            check(lib.mdqe_conv3x3_winograd_f32(ptr(x), xis, ptr(U), ptr(bias), ptr(out), ldy, NI, H, W, Cin, Cout, ACT[act],
                                                ptr(ws), ws.numel(), cur_stream()), "conv3x3_winograd_f32")
            return out
    ws = None
    if ksplit == 0 and K >= 4096 and ((OH * OW + 63) // 64) * ((Cout + 63) // 64) <= 16:
        # few output pixels PER IMAGE, very deep K (input_proj's 3x3/s2 on res5: 60 pixels, K = 18432): spread K over the CUs.  Decided
        # from one image's tiles, never from the batch: a split changes the order of the K sum, and a frame's bits must not depend on
        # how many frames share its pass
        ksplit = min(16, K // 1024)
    if ksplit > 1:
        ws = _workspace(ksplit * M * Cout * 4 + 64, x.device)
    check(lib.mdqe_conv2d_nhwc_f32(ptr(x), xis, ptr(w_packed), ptr(bias), ptr(out), ldy, NI, H, W, Cin, Cout, KH, KW, stride,
                                   pad, ACT[act], ptr(residual), ldr, int(res_first), tile, ptr(_wsplit(w_packed)), ksplit, ptr(ws),
                                   cur_stream()),
          "conv2d_nhwc_f32")
    return out


LINEAR_LN_FUSED = os.environ.get("MDQE_LINEAR_LN_FUSED", "1") != "0"     # 0: GEMM then LayerNorm kernel (debug / A-B)
LINEAR_LN_MIN_ROWS = 16384        # below this the 64x256 tile leaves CUs idle: 64x64 GEMM + LayerNorm kernel is faster


def linear_ln(x, weight, bias, residual, gamma, beta, eps=1e-5, out=None, scratch=None, second=None):
    """out = LayerNorm(x @ weight^T + bias + residual) * gamma + beta over N == 256 columns; `out` may be `residual`.
    One kernel (64x256 tile, statistics in the epilogue) in exact-fp32 mode with enough rows to fill the chip; otherwise
    the GEMM (own tile / f16x3 arithmetic) into `scratch` followed by the LayerNorm kernel.
    second=(gamma2, beta2): also returns out2 = LayerNorm(out) * gamma2 + beta2 -- in the same epilogue where the one-kernel form runs
    (mdqe_gemm_ln2_f32), by one more LayerNorm launch otherwise; the two give the same bits."""
    M, K = x.shape
    N = weight.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    # one block per 64 rows: a grid just over a multiple of the 256 CUs runs its last round nearly empty (21 168 rows = 331 blocks take two
    # rounds: 139 us against 117 for GEMM + LayerNorm, tools/ln_tile_ab.py) -- the two forms give identical bits, so the choice is free
    nb = (M + 63) // 64
    full = nb >= 1024 or nb / (256.0 * ((nb + 255) // 256)) >= 0.8
    small = M * max(out.stride(0), residual.stride(0) if residual is not None else 0) * 4 < 0xFFFF0000       # (32-bit buffer offsets in the epilogue)
    if LINEAR_LN_FUSED and N == 256 and M >= LINEAR_LN_MIN_ROWS and full and small and get_gemm_precision() == "f32" and x.stride(1) == 1:
        _chk(weight, "weight"); _chk(bias, "bias"); _chk(gamma, "gamma"); _chk(beta, "beta"); _chk(residual, "residual"); _chk(out, "out")
        if second is not None and LINEAR_LN2_FUSED:
            _chk(second[0], "gamma2"); _chk(second[1], "beta2")
            out2 = torch.empty((M, N), dtype=torch.float32, device=x.device)
            check(lib.mdqe_gemm_ln2_f32(ptr(x), x.stride(0) if M > 1 else K, ptr(weight), ptr(bias), ptr(out), out.stride(0), M, N, K,
                                        ptr(residual), residual.stride(0) if residual is not None else 0, ptr(gamma), ptr(beta),
                                        ptr(second[0]), ptr(second[1]), ptr(out2), out2.stride(0), eps, cur_stream()), "gemm_ln2_f32")
            return out, out2
        check(lib.mdqe_gemm_ln_f32(ptr(x), x.stride(0) if M > 1 else K, ptr(weight), ptr(bias), ptr(out), out.stride(0), M, N, K,
                                   ptr(residual), residual.stride(0) if residual is not None else 0, ptr(gamma), ptr(beta), eps,
                                   cur_stream()), "gemm_ln_f32")
        return out if second is None else (out, layernorm(out, second[0], second[1], eps=eps))
    y = linear(x, weight, bias, residual=residual, out=scratch)
    out = layernorm(y, gamma, beta, eps=eps, out=out)
    return out if second is None else (out, layernorm(out, second[0], second[1], eps=eps))


LINEAR_LN2_FUSED = os.environ.get("MDQE_LINEAR_LN2_FUSED", "1") != "0"   # 0: the second LayerNorm as its own launch (debug / A-B)


def linear_side(x, weight, bias, side, side_w, side_cols, out=None):
    """out = x @ weight^T + bias, and out[:, :side_cols] += side [M,4] @ side_w[:side_cols, :4]^T (mdqe_gemm_nt_side_f32): a projection
    of `x + pos` for a pos that is linear in four numbers per row, without materialising pos."""
    M, K = x.shape
    N = weight.shape[0]
    _chk(weight, "weight"); _chk(bias, "bias"); _chk(side, "side"); _chk(side_w, "side_w")
    if x.stride(1) != 1 or side.shape != (M, 4) or side_w.shape != (N, 4):
        raise RuntimeError("linear_side: x rows contiguous, side [M,4], side_w [N,4] required")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    check(lib.mdqe_gemm_nt_side_f32(ptr(x), x.stride(0) if M > 1 else K, ptr(weight), ptr(bias), ptr(out), out.stride(0), M, N, K,
                                    ptr(side), ptr(side_w), side_cols, ptr(_wsplit(weight)), cur_stream()), "gemm_nt_side_f32")
    return out


def linear_cat2(y, x_nhwc, stride, weight, bias, act=None, out=None):
    """act([y | x'] @ weight^T + bias): a bottleneck's conv3 and its projection shortcut in one product (mdqe_gemm_nt_cat2_f32).
    y [NI, OH, OW, K1] (contiguous), x_nhwc [NI, H2, W2, K2] read at (oh*stride, ow*stride), weight [N, K1 + K2] -> [NI, OH, OW, N]."""
    _chk(y, "y"); _chk(x_nhwc, "x"); _chk(weight, "weight"); _chk(bias, "bias")
    NI, OH, OW, K1 = y.shape
    _, H2, W2, K2 = x_nhwc.shape
    N = weight.shape[0]
    if not (y.is_contiguous() and x_nhwc.is_contiguous() and weight.is_contiguous() and weight.shape[1] == K1 + K2):
        raise RuntimeError("linear_cat2: contiguous operands and a [N, K1 + K2] weight required")
    if out is None:
        out = torch.empty((NI, OH, OW, N), dtype=torch.float32, device=y.device)
    check(lib.mdqe_gemm_nt_cat2_f32(ptr(y), K1, K1, ptr(x_nhwc), K2, K2, NI, OH, OW, H2, W2, stride, ptr(weight), ptr(bias), ptr(out), N, N,
                                    ACT[act], cur_stream()), "gemm_nt_cat2")
    return out


def linear_pix(x_nhwc, stride, weight, bias, act=None, out=None):
    """act(x[:, ::stride, ::stride] @ weight^T + bias): a 1x1 convolution with stride and no padding, the strided pixels read in place
    (mdqe_gemm_nt_pix_f32; exact fp32 whatever the GEMM precision mode).  x_nhwc [NI, H, W, K] contiguous, weight [N, K] ->
    [NI, (H - 1) // stride + 1, (W - 1) // stride + 1, N]."""
    _chk(x_nhwc, "x"); _chk(weight, "weight"); _chk(bias, "bias")
    NI, H, W, K = x_nhwc.shape
    N = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != K:
        raise RuntimeError("linear_pix: a [N, K] weight required")
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if out is None:
        out = torch.empty((NI, OH, OW, N), dtype=torch.float32, device=x_nhwc.device)
    check(lib.mdqe_gemm_nt_pix_f32(ptr(x_nhwc), K, K, NI, H, W, OH, OW, stride, ptr(weight), ptr(bias), ptr(out), N, N, ACT[act],
                                   cur_stream()), "gemm_nt_pix")
    return out


def layernorm(x, gamma, beta, res=None, eps=1e-5, out=None):
    _chk(x, "x"); _chk(res, "res"); _chk(gamma, "gamma"); _chk(beta, "beta")
    C = x.shape[-1]
    rows = x.numel() // C
    if out is None:
        out = torch.empty_like(x)
    check(lib.mdqe_layernorm_f32(ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(out), rows, C, eps, cur_stream()), "layernorm")
    return out


def groupnorm_nhwc(x, groups, gamma, beta, act=None, eps=1e-5, out=None):
    """x [NI, HW, C] (pixel stride x.stride(1), image stride x.stride(0)); `out` may be a strided view
    (e.g. a level slice of the encoder token buffer) or x itself (in place)."""
    if x.dim() == 4:
        x = x.view(x.shape[0], -1, x.shape[-1])
    NI, HW, C = x.shape
    if out is None:
        out = torch.empty((NI, HW, C), dtype=torch.float32, device=x.device)
    elif out.dim() == 4:
        out = out.view(NI, HW, C)
    ws = _workspace(lib.mdqe_groupnorm_workspace_bytes(NI, groups), x.device)
    check(lib.mdqe_groupnorm_nhwc_f32(ptr(x), x.stride(1), x.stride(0) if NI > 1 else 0, ptr(out), out.stride(1),
                                      out.stride(0) if NI > 1 else 0, NI, HW, C, groups, ptr(gamma),
                                      ptr(beta), eps, ACT[act], ptr(ws), cur_stream()), "groupnorm_nhwc")
    return out


def stem_im2col(frames, Hp, Wp, mean, std):
    """frames [NI,3,h,w] uint8 or fp32 CUDA -> [NI*Hp/2*Wp/2, 160] normalised+padded im2col."""
    import ctypes
    if not frames.is_cuda or not frames.is_contiguous() or frames.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("stem_im2col: frames must be contiguous CUDA uint8/float32 [NI,3,h,w]")
    NI, _, h, w = frames.shape
    out = torch.empty((NI * (Hp // 2) * (Wp // 2), 160), dtype=torch.float32, device=frames.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    check(lib.mdqe_stem_im2col_f32(ptr(frames), int(frames.dtype == torch.uint8), 3 * h * w, NI, h, w, Hp, Wp, m, s, ptr(out),
                                   cur_stream()), "stem_im2col")
    return out


def stem_weight_kmajor(w_krsc):
    """[64,7,7,3] (BN-folded, k = (kh,kw,c)) -> the [154,64] k-major layout of mdqe_stem_conv_f32 (row kh*22+21 zero)."""
    wk = torch.zeros(7, 22, 64, dtype=torch.float32)
    wk[:, :21] = w_krsc.reshape(64, 7, 21).permute(1, 2, 0)
    return wk.reshape(154, 64).contiguous()


def stem_conv(frames, Hp, Wp, mean, std, wk, bias):
    """frames [NI,3,h,w] uint8 or fp32 CUDA -> relu(conv7x7/s2(pad(normalise(frames))) + bias) as NHWC [NI,Hp/2,Wp/2,64]."""
    import ctypes
    if not frames.is_cuda or not frames.is_contiguous() or frames.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError("stem_conv: frames must be contiguous CUDA uint8/float32 [NI,3,h,w]")
    _chk(wk, "wk"); _chk(bias, "bias")
    if tuple(wk.shape) != (154, 64) or bias.numel() != 64:
        raise RuntimeError("stem_conv: wk must be [154,64] (stem_weight_kmajor) and bias [64]")
    NI, _, h, w = frames.shape
    out = torch.empty((NI, Hp // 2, Wp // 2, 64), dtype=torch.float32, device=frames.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    check(lib.mdqe_stem_conv_f32(ptr(frames), int(frames.dtype == torch.uint8), 3 * h * w, NI, h, w, Hp, Wp, m, s, ptr(wk),
                                 ptr(bias), ptr(out), cur_stream()), "stem_conv")
    return out


def maxpool3x3s2(x):
    _chk(x, "x")
    NI, H, W, C = x.shape
    out = torch.empty((NI, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), dtype=torch.float32, device=x.device)
    check(lib.mdqe_maxpool3x3s2_nhwc_f32(ptr(x), ptr(out), NI, H, W, C, cur_stream()), "maxpool")
    return out


def upsample_nearest_add(a, b, out=None):
    _chk(a, "a"); _chk(b, "b")
    NI, H, W, C = a.shape
    if out is None:
        out = torch.empty_like(a)
    check(lib.mdqe_upsample_nearest_add_nhwc_f32(ptr(a), ptr(b), ptr(out), NI, H, W, b.shape[1], b.shape[2], C, cur_stream()),
          "upsample_nearest_add")
    return out


def dwconv5x5(x, wt, bias, up2=False, tw=None, tb=None):
    """x [NI,H,W,C]; wt [25,C]; if up2: output is [NI,2H,2W,C] over the virtual transposed-conv output."""
    _chk(x, "x"); _chk(wt, "wt"); _chk(bias, "bias")
    NI, H, W, C = x.shape
    OH, OW = (2 * H, 2 * W) if up2 else (H, W)
    out = torch.empty((NI, OH, OW, C), dtype=torch.float32, device=x.device)
    if C == 256 and DW_FAST:                              # wave = the 64 channel groups of a pixel, taps in registers
        if up2:
            _chk(tw, "tw"); _chk(tb, "tb")
            check(lib.mdqe_dwconv5x5_up2_c256_f32(ptr(x), ptr(wt), ptr(bias), ptr(tw), ptr(tb), ptr(out), NI, H, W, cur_stream()),
                  "dwconv5x5_up2_c256")
        else:
            check(lib.mdqe_dwconv5x5_c256_f32(ptr(x), ptr(wt), ptr(bias), ptr(out), NI, H, W, cur_stream()), "dwconv5x5_c256")
        return out
    check(lib.mdqe_dwconv5x5_nhwc_f32(ptr(x), ptr(wt), ptr(bias), ptr(out), NI, OH, OW, C, int(up2), ptr(tw), ptr(tb),
                                      cur_stream()), "dwconv5x5")
    return out


DW_FAST = os.environ.get("MDQE_DW_FAST", "1") != "0"        # 0: generic depthwise kernel (debug / A-B)
MASK_HEAD_FUSED = os.environ.get("MDQE_MASK_HEAD_FUSED", "1") != "0"   # 0: up-sampling depthwise conv and its 1x1 as two launches


def dwconv5x5_up2_pw(x, wt, bias, tw, tb, pw, pb, out=None):
    """linear(dwconv5x5(x, wt, bias, up2=True, tw, tb), pw, pb): x [NI,Hs,Ws,C] -> [NI,2Hs,2Ws,N]; `out`: a [NI*2Hs*2Ws, N] view whose rows
    may be strided (rows of a larger buffer).  C == 256, N == 32, exact-fp32 GEMM mode and 16-byte aligned operands take ONE kernel that
    never stores the [.., C] tensor between the two (mdqe_dwconv5x5_up2_pw_c256_f32: the same bits); everything else, and
    MDQE_MASK_HEAD_FUSED=0, takes the two launches."""
    _chk(x, "x"); _chk(wt, "wt"); _chk(bias, "bias"); _chk(tw, "tw"); _chk(tb, "tb"); _chk(pw, "pw"); _chk(pb, "pb")
    NI, Hs, Ws, C = x.shape
    N = pw.shape[0]
    rows = NI * 4 * Hs * Ws
    if out is not None and (out.dim() != 2 or tuple(out.shape) != (rows, N) or out.stride(1) != 1 or not out.is_cuda or out.dtype != torch.float32):
        raise RuntimeError("dwconv5x5_up2_pw: out must be a CUDA fp32 [NI*2Hs*2Ws, N] view with contiguous rows")
    ldo = N if out is None or rows <= 1 else out.stride(0)
    ptrs = [t.data_ptr() for t in (x, wt, bias, tw, tb, pw, pb)] + ([out.data_ptr()] if out is not None else [])
    fused = (MASK_HEAD_FUSED and DW_FAST and C == 256 and N == 32 and pw.shape[1] == C and lib.mdqe_get_gemm_precision() == 0
             and all(a % 16 == 0 for a in ptrs) and ldo % 4 == 0 and ldo >= N)
    if not fused:
        z = dwconv5x5(x, wt, bias, up2=True, tw=tw, tb=tb)
        return linear(z.view(-1, C), pw, pb, out=out)
    if out is None:
        out = torch.empty((rows, N), dtype=torch.float32, device=x.device)
    check(lib.mdqe_dwconv5x5_up2_pw_c256_f32(ptr(x), ptr(wt), ptr(bias), ptr(tw), ptr(tb), ptr(pw), ptr(pb), ptr(out), ldo, NI, Hs, Ws,
                                             cur_stream()), "dwconv5x5_up2_pw_c256")
    return out


def msda(value, shapes_dev, starts_dev, loc, attn, groups=1, scale=1.0, out=None):
    """value [B,S,M,D]; shapes_dev [G*L,2] int64; loc [B,Q,M,L,P,2]; attn [B,Q,M,L,P] -> [B,Q,M*D]."""
    B, S, M, D = value.shape
    Q, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
    if out is None:
        out = torch.empty((B, Q, M * D), dtype=torch.float32, device=value.device)
    check(lib.mdqe_msda_forward_grouped_f32(ptr(value), ptr(shapes_dev), ptr(starts_dev), ptr(loc), ptr(attn), B, S, M, D,
                                            groups, L, Q, P, scale, ptr(out), cur_stream()), "msda")
    return out


def msda_fused(value, offs, logits, ref, levels, B, Q, M, D, L, P, mode=0, grid=None, groups=1, scale=1.0,
               v_brows=None, out=None, vidx=None):
    """Fused MSDeformAttn core.  value/offs/logits: 2-D row-strided fp32 views (last dim contiguous):
    value [B*v_brows, M*D], offs [B*Q, M*L*P*2], logits [B*Q, M*L*P].  ref: [Q,2|4] (broadcast) or [B,Q,2|4].
    levels: (H list, W list, start-row list) of length groups*L; the levels may lie anywhere in the element's block (the
    LDS-staged kernels are taken only where the staged levels lie back to back in ascending order)."""
    import ctypes
    Hs, Ws, Ss = levels
    n = groups * L
    assert len(Hs) == n and len(Ws) == n and len(Ss) == n
    if ref.dim() == 2:
        ref_b, ref_dim = 0, ref.shape[-1]
    else:
        ref_b, ref_dim = ref.stride(0), ref.shape[-1]
    _chk(ref, "ref")
    if out is None:
        out = torch.empty((B * Q, M * D), dtype=torch.float32, device=value.device)
    arr = lambda v: (ctypes.c_int * n)(*[int(x) for x in v])
    if v_brows is None:
        v_brows = value.shape[0] // max(B, 1)
    if vidx is not None and (vidx.dtype != torch.int32 or not vidx.is_cuda or vidx.numel() != B):
        raise RuntimeError("msda_fused: vidx must be a CUDA int32 tensor with B entries")
    check(lib.mdqe_msda_fused_f32(ptr(value), value.stride(0), v_brows, ptr(vidx), ptr(offs), offs.stride(0), ptr(logits),
                                  logits.stride(0), ptr(ref), ref_b, ref_dim, mode, ptr(grid), arr(Hs), arr(Ws), arr(Ss),
                                  B, M, D, groups, L, Q, P, scale, ptr(out), out.stride(0), value.shape[0], cur_stream()), "msda_fused")
    return out


def mask_row_stats(logits):
    """logits [n,T,H,W] -> (stats [n,5], soft_h [n,Ph], hard_h [n,Ph]); see mdqe_mask_row_stats_f32."""
    _chk(logits, "logits")
    n, T, H, W = logits.shape
    t_step = 2 if T >= 5 else 1
    Th = (T + t_step - 1) // t_step
    Ph = Th * (H // 2) * (W // 2)
    stats = torch.empty(n, 5, device=logits.device)
    soft_h = torch.empty(n, Ph, device=logits.device)
    hard_h = torch.empty(n, Ph, device=logits.device)
    check(lib.mdqe_mask_row_stats_f32(ptr(logits), n, T, H, W, t_step, ptr(stats), ptr(soft_h), ptr(hard_h), cur_stream()),
          "mask_row_stats")
    return stats, soft_h, hard_h


def mha_small(qk, v, B, Q, C, nh, out=None):
    """qk [B*Q, 2C] (q | k), v [B*Q, C] -> [B*Q, C]."""
    if out is None:
        out = torch.empty((B * Q, C), dtype=torch.float32, device=v.device)
    check(lib.mdqe_mha_small_f32(ptr(qk), qk.stride(0), ptr(v), v.stride(0), ptr(out), out.stride(0), B, Q, C, nh, cur_stream()),
          "mha_small")
    return out


def query_select(conf, nb, out=None):
    """conf [NI,H,W,K] -> coords [NI, nb*nb, 2] (out: a contiguous tensor of that shape to store into)."""
    _chk(conf, "conf")
    NI, H, W, K = conf.shape
    ws = torch.empty(NI * H * W, dtype=torch.float32, device=conf.device)
    if out is not None:
        _chk(out, "out")
        if tuple(out.shape) != (NI, nb * nb, 2):
            raise RuntimeError("query_select: out must be [NI, nb*nb, 2]")
    coords = out if out is not None else torch.empty(NI, nb * nb, 2, dtype=torch.float32, device=conf.device)
    check(lib.mdqe_query_select_f32(ptr(conf), NI, H, W, K, nb, ptr(ws), ptr(coords), cur_stream()), "query_select")
    return coords


def sample_levels_mean(tokens, coords, shapes, starts, out=None):
    """tokens [NI,N,C], coords [NI,Q,2] -> [NI,Q,C] (out: a contiguous tensor of that shape to store into)."""
    import ctypes
    _chk(tokens, "tokens"); _chk(coords, "coords")
    NI, N, C = tokens.shape
    Qn = coords.shape[1]
    n = len(shapes)
    arr = lambda v: (ctypes.c_int * n)(*[int(x) for x in v])
    if out is None:
        out = torch.empty(NI, Qn, C, dtype=torch.float32, device=tokens.device)
    else:
        _chk(out, "out")
        if tuple(out.shape) != (NI, Qn, C):
            raise RuntimeError("sample_levels_mean: out must be [NI, Q, C]")
    check(lib.mdqe_sample_levels_mean_f32(ptr(tokens), NI, N, C, ptr(coords), Qn, arr([s[0] for s in shapes]), arr([s[1] for s in shapes]),
                                          arr(starts), n, ptr(out), cur_stream()), "sample_levels_mean")
    return out


def _final_mask_args(logits, inst_idx, check_idx, cap=None):
    """The preamble of the four final-mask wrappers -> (n_sel, Fw, Hm, Wm) and, with `cap`, the RLE buffers pos, n_pos.  The two geometry
    forms validate inst_idx, the two older ones pass it through."""
    _chk(logits, "logits")
    n, Fw, Hm, Wm = logits.shape
    if check_idx:
        _chk(inst_idx, "inst_idx", torch.int32)
    k = int(inst_idx.numel())
    if cap is None:
        return k, Fw, Hm, Wm
    return (k, Fw, Hm, Wm, torch.empty(k * Fw, cap, dtype=torch.int32, device=logits.device),
            torch.empty(k * Fw, dtype=torch.int32, device=logits.device))


def final_masks(logits, inst_idx, factor, h, w, Ho, Wo, out, f_off):
    """logits [n,Fw,Hm,Wm]; inst_idx int32 CUDA [n_sel]; out uint8 [n_sel_total, L, Ho, Wo] (rows 0..n_sel-1 written)."""
    k, Fw, Hm, Wm = _final_mask_args(logits, inst_idx, False)
    check(lib.mdqe_final_masks_u8(ptr(logits), k, ptr(inst_idx), Fw, Hm, Wm, factor, h, w, Ho, Wo, ptr(out),
                                  out.stride(0), f_off, cur_stream()), "final_masks")
    return out


def final_masks_geom(logits, inst_idx, factor, h, w, Ho, Wo, out, f_off, geom=None):
    """ops.final_masks plus, from the same sweep, geom int32 [n_sel*Fw, 5]: row k*Fw+f = (area, xmin, ymin, xmax, ymax) of the set
    pixels of (row k, window frame f), inclusive; an empty mask is (0, Wo, Ho, -1, -1).  `geom`: a buffer to write into (fully overwritten, whatever it held).  -> (out, geom)."""
    k, Fw, Hm, Wm = _final_mask_args(logits, inst_idx, True)
    if (not out.is_cuda or out.dtype != torch.uint8 or out.dim() != 4 or out.shape[0] < k or (out.shape[0] and not out[0].is_contiguous())
            or tuple(out.shape[2:]) != (Ho, Wo) or f_off < 0 or f_off + Fw > out.shape[1]):
        raise RuntimeError("final_masks_geom: out must be CUDA uint8 [>= n_sel, >= f_off + Fw, Ho, Wo]")
    geom = _geom_rows(geom, k * Fw, logits.device)
    check(lib.mdqe_final_masks_u8_geom(ptr(logits), k, ptr(inst_idx), Fw, Hm, Wm, factor, h, w, Ho, Wo, ptr(out), out.stride(0), f_off,
                                       ptr(geom), cur_stream()), "final_masks_geom")
    return out, geom


def final_label_map(logits, inst_idx, factor, h, w, Ho, Wo, out, f_off, geom=None):
    """One plane per frame instead of one per track: out[f_off + f] (uint8 [>= f_off + Fw, Ho, Wo], CUDA, contiguous) = which of the rows
    `inst_idx` (int32 CUDA [n_sel]) of logits [n, Fw, Hm, Wm] owns each pixel -- inst_idx[k] + 1 for the row with the largest up-sampled
    logit among those whose final-mask bit is set there (the first of them on an exact tie), 0 where none is set; n <= 255.  `geom`:
    None, True (allocate) or an int32 [n_sel*Fw, 5] buffer -- the rows of ops.final_masks_geom for each label's visible region (fully
    overwritten).  n_sel == 0 writes zeros to the Fw frames.  -> (out, geom or None)."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if logits.dim() != 4 or int(logits.shape[0]) > 255:
        raise RuntimeError("final_label_map: logits must be [n <= 255, Fw, Hm, Wm] (uint8 labels), got %s" % (tuple(logits.shape),))
    if inst_idx.dtype != torch.int32 or inst_idx.dim() != 1:
        raise RuntimeError("final_label_map: inst_idx must be int32 [n_sel], got %s %s" % (inst_idx.dtype, tuple(inst_idx.shape)))
    Fw = int(logits.shape[1])
    if (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 3 or tuple(out.shape[1:]) != (Ho, Wo) or f_off < 0
            or f_off + Fw > out.shape[0] or not out.is_contiguous() or not out.is_cuda):
        raise RuntimeError("final_label_map: out must be contiguous CUDA uint8 [>= f_off + Fw = %d, Ho, Wo]" % (f_off + Fw))
    k, Fw, Hm, Wm = _final_mask_args(logits, inst_idx, True)
    if geom is not None:
        geom = _geom_rows(geom, k * Fw, logits.device)
    check(lib.mdqe_final_label_map_u8(ptr(logits), k, ptr(inst_idx), Fw, Hm, Wm, factor, h, w, Ho, Wo, ptr(out), f_off,
                                      ptr(geom) if geom is not None and k else None, cur_stream()), "final_label_map")
    return out, geom


def final_matte(logits, inst_idx, factor, h, w, Ho, Wo, out, f_off, take=None, gain=1.0):
    """The soft form of `final_label_map`: out[f_off + f] (uint8 [>= f_off + Fw, Ho, Wo], CUDA, contiguous) = the matte of the rows
    `inst_idx` (int32 CUDA [n_sel]) of logits [n <= 255, Fw, Hm, Wm] that take part -- all of them, or with `take` (uint8 CUDA [256],
    indexed by the row's label inst_idx[k] + 1) those whose entry is not 0: rint(255 * sigmoid(gain * the largest up-sampled logit
    among them)), held at >= 128 where one of their final-mask bits is set and at <= 127 where none is, 0 without a participating
    row.  So out >= 128 exactly on the union of those rows' dense masks.  gain in (0, 64] sharpens (> 1) or softens (< 1) the edge:
    the rule of include/mdqe_hip.h, mdqe_final_matte_u8.  n_sel == 0 writes zeros to the Fw frames.  -> out."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if not torch.is_tensor(logits) or logits.dim() != 4 or int(logits.shape[0]) > 255:
        raise RuntimeError("final_matte: logits must be [n <= 255, Fw, Hm, Wm], got %s" % (tuple(getattr(logits, "shape", ())),))
    if not torch.is_tensor(inst_idx) or inst_idx.dtype != torch.int32 or inst_idx.dim() != 1:
        raise RuntimeError("final_matte: inst_idx must be int32 [n_sel]")
    if isinstance(gain, bool) or not isinstance(gain, (int, float)) or not 0.0 < float(gain) <= 64.0:
        raise RuntimeError("final_matte: gain must be a finite number in (0, 64], got %r" % (gain,))
    if take is not None and (not torch.is_tensor(take) or take.dtype != torch.uint8 or tuple(take.shape) != (256,) or not take.is_contiguous()):
        raise RuntimeError("final_matte: take must be contiguous uint8 [256] (render.Style.takes) or None")
    Fw = int(logits.shape[1])
    if (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 3 or tuple(out.shape[1:]) != (Ho, Wo)
            or not isinstance(f_off, int) or f_off < 0 or f_off + Fw > out.shape[0] or not out.is_contiguous()):
        raise RuntimeError("final_matte: out must be contiguous CUDA uint8 [>= f_off + Fw = %d, Ho, Wo]" % (f_off + Fw))
    for name, t in (("out", out), ("take", take)):
        if t is not None and (not t.is_cuda or t.device != logits.device):
            raise RuntimeError("final_matte: %s must be a CUDA tensor on the logits' device, got %s" % (name, t.device))
    k, Fw, Hm, Wm = _final_mask_args(logits, inst_idx, True)
    check(lib.mdqe_final_matte_u8(ptr(logits), k, ptr(inst_idx), Fw, Hm, Wm, factor, h, w, Ho, Wo, ptr(take), float(gain), ptr(out), f_off,
                                  cur_stream()), "final_matte")
    return out


def final_masks_overlap(logits, inst_idx, factor, h, w, Ho, Wo, gt_bits, G, f_off, inter, area=None):
    """A window's final masks scored against ground truth on the device (vis_score.py): for the rows `inst_idx` (int32 CUDA [n_sel]) of
    logits [n, Fw, Hm, Wm], with b_k the final-mask bit of row k (ops.final_masks' own bit), inter[k, g] (int64 CUDA [>= n_sel, >= G],
    rows inter.stride(0) apart) is INCREASED by the number of window pixels where b_k and bit g of gt_bits[f_off + f] (uint32 CUDA
    [>= f_off + Fw, Ho, Wo], contiguous; G <= 32 ground-truth tracks, one bit each) are both set -- zero it once per video, the windows
    add up -- and area (int32 CUDA [n_sel * Fw], allocated when None) is OVERWRITTEN with the set pixels of (row k, frame f), column 0
    of ops.final_masks_geom's table.  Integers only: exact, identical from run to run.  -> (inter, area)."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise RuntimeError("final_masks_overlap: logits must be [n, Fw, Hm, Wm], got %s" % (tuple(getattr(logits, "shape", ())),))
    if not torch.is_tensor(inst_idx) or inst_idx.dtype != torch.int32 or inst_idx.dim() != 1:
        raise RuntimeError("final_masks_overlap: inst_idx must be int32 [n_sel]")
    k, Fw = int(inst_idx.numel()), int(logits.shape[1])
    if (not torch.is_tensor(gt_bits) or gt_bits.dtype != torch.uint32 or gt_bits.dim() != 3 or tuple(gt_bits.shape[1:]) != (Ho, Wo)
            or not gt_bits.is_contiguous()):
        raise RuntimeError("final_masks_overlap: gt_bits must be contiguous uint32 [frames, Ho = %d, Wo = %d]" % (Ho, Wo))
    if f_off < 0 or f_off + Fw > gt_bits.shape[0]:
        raise RuntimeError("final_masks_overlap: gt_bits holds %d frames, the window needs f_off + Fw = %d" % (gt_bits.shape[0], f_off + Fw))
    if (not torch.is_tensor(inter) or inter.dtype != torch.int64 or inter.dim() != 2 or inter.shape[0] < k or inter.shape[1] < G
            or inter.stride(1) != 1 or (inter.shape[0] > 1 and inter.stride(0) < G)):
        raise RuntimeError("final_masks_overlap: inter must be int64 [>= n_sel = %d, >= G = %d] with unit column stride" % (k, G))
    if area is not None and (not torch.is_tensor(area) or area.dtype != torch.int32 or area.numel() != k * Fw or not area.is_contiguous()):
        raise RuntimeError("final_masks_overlap: area must be contiguous int32 [n_sel * Fw = %d]" % (k * Fw))
    for name, t in (("gt_bits", gt_bits), ("inter", inter), ("area", area)):
        if t is not None and not t.is_cuda:
            raise RuntimeError("final_masks_overlap: %s must be a CUDA tensor" % name)
    k, Fw, Hm, Wm = _final_mask_args(logits, inst_idx, True)
    if area is None:
        area = torch.empty(k * Fw, dtype=torch.int32, device=logits.device)
    check(lib.mdqe_final_masks_overlap(ptr(logits), k, ptr(inst_idx), Fw, Hm, Wm, factor, h, w, Ho, Wo, ptr(gt_bits), G, f_off,
                                       ptr(inter), inter.stride(0) if inter.shape[0] > 1 else max(int(inter.shape[1]), G), ptr(area),
                                       cur_stream()), "final_masks_overlap")
    return inter, area


def final_occlusion(logits, inst_idx, factor, h, w, Ho, Wo, out=None):
    """A window's final masks counted against each other on the device: for the rows `inst_idx` (int32 CUDA [n_sel], n_sel <= 255) of
    logits [n, Fw, Hm, Wm], with b_k the final-mask bit of row k (ops.final_masks' own bit) and o the pixel's owner (ops.final_label_map's
    own choice among those rows), occ[k, f, j] = the number of pixels of window frame f with b_k set and o == j.  So occ[k, f, k] is the
    area of k's visible region, occ[k, f].sum() the area of its dense mask and, for j != k, occ[k, f, j] the part of k that j hides
    (the rule of include/mdqe_hip.h, mdqe_final_masks_occlusion; helpers on the table: occlusion.py).  `out`: a contiguous int32 CUDA
    [n_sel, Fw, n_sel] buffer to write into (fully overwritten, whatever it held).  Integers only: exact, identical from run to run.
    -> occ int32 CUDA [n_sel, Fw, n_sel]."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if not torch.is_tensor(logits) or logits.dim() != 4:
        raise RuntimeError("final_occlusion: logits must be [n, Fw, Hm, Wm], got %s" % (tuple(getattr(logits, "shape", ())),))
    if not torch.is_tensor(inst_idx) or inst_idx.dtype != torch.int32 or inst_idx.dim() != 1 or int(inst_idx.numel()) > 255:
        raise RuntimeError("final_occlusion: inst_idx must be int32 [n_sel <= 255]")
    k, Fw = int(inst_idx.numel()), int(logits.shape[1])
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.int32 or tuple(out.shape) != (k, Fw, k) or not out.is_contiguous()):
        raise RuntimeError("final_occlusion: out must be contiguous int32 [n_sel = %d, Fw = %d, n_sel]" % (k, Fw))
    if out is not None and (not out.is_cuda or out.device != logits.device):
        raise RuntimeError("final_occlusion: out must be a CUDA tensor on the logits' device, got %s" % (out.device,))
    k, Fw, Hm, Wm = _final_mask_args(logits, inst_idx, True)
    if out is None:
        out = torch.empty((k, Fw, k), dtype=torch.int32, device=logits.device)
    check(lib.mdqe_final_masks_occlusion(ptr(logits), k, ptr(inst_idx), Fw, Hm, Wm, factor, h, w, Ho, Wo, ptr(out), cur_stream()),
          "final_occlusion")
    return out


def _action_arg(name, action):
    """The per-label action table of the painters that take one."""
    if not torch.is_tensor(action) or action.dtype != torch.uint8 or tuple(action.shape) != (256,) or not action.is_contiguous():
        raise RuntimeError("%s: action must be contiguous uint8 [256] (render.Style.actions)" % name)


def _mosaic_args(name, action, cell):
    _action_arg(name, action)
    if isinstance(cell, bool) or not isinstance(cell, int) or not 2 <= cell <= 64 or cell % 2:
        raise RuntimeError("%s: cell must be an even int in 2..64, got %r" % (name, cell))


def _blur_args(name, action, taps, taps_c=None, surface=False):
    """The action table and the tap tables of the blur painters (render.blur_taps): luma / RGB radius 0..32, chroma 0..16."""
    _action_arg(name, action)
    for t, what, top in ((taps, "taps", 32),) + (((taps_c, "taps_c", 16),) if surface else ()):
        if (not torch.is_tensor(t) or t.dtype not in (torch.uint16, torch.int16) or t.dim() != 1 or not 1 <= t.numel() <= top + 1
                or not t.is_contiguous()):
            raise RuntimeError("%s: %s must be contiguous uint16 [radius + 1], radius in 0..%d (render.blur_taps)" % (name, what, top))


def _replace_args(name, action, matte, backdrop, F, H, W):
    """The action table, the matte and an RGB backdrop of the compositing painter."""
    _action_arg(name, action)
    if not torch.is_tensor(matte) or matte.dtype != torch.uint8 or tuple(matte.shape) != (F, H, W) or not matte.is_contiguous():
        raise RuntimeError("%s: matte must be contiguous uint8 [F = %d, %d, %d], the labels' shape (ops.final_matte)" % (name, F, H, W))
    if (not torch.is_tensor(backdrop) or backdrop.dtype != torch.uint8 or tuple(backdrop.shape) not in ((3,), (H, W, 3))
            or not backdrop.is_contiguous()):
        raise RuntimeError("%s: backdrop must be contiguous uint8 [3] (a colour) or [%d, %d, 3] (a picture of the output's size), got %s"
                           % (name, H, W, tuple(getattr(backdrop, "shape", ()))))


def _rgb_paint_args(name, labels, frames, palette, out, f_off, a256, contour, mosaic=None, blur=None, replace=None):
    """The checks of render_overlay, of render_mosaic (mosaic = (action, cell)), of render_blur (blur = (action, taps)) and of
    render_replace (replace = (action, matte, backdrop)).  -> (F, Ho, Wo, h0, w0, frame stride)."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise RuntimeError("%s: labels must be contiguous uint8 [F, Ho, Wo]" % name)
    F, Ho, Wo = (int(v) for v in labels.shape)
    if not isinstance(a256, int) or not isinstance(contour, int) or not 0 <= a256 <= 256 or not 0 <= contour <= 3:
        raise RuntimeError("%s: a256 must be an int in 0..256 and contour an int in 0..3, got %r, %r" % (name, a256, contour))
    if mosaic is not None:
        _mosaic_args(name, *mosaic)
    if blur is not None:
        _blur_args(name, *blur)
    if replace is not None:
        _replace_args(name, *replace, F, Ho, Wo)
    if Ho < 1 or Wo < 1 or Ho * Wo * 3 >= 2 ** 31 or F * Ho * Wo >= 2 ** 31:
        raise RuntimeError("%s: Ho, Wo must be positive with Ho*Wo*3 < 2^31 and F*Ho*Wo < 2^31, got %s" % (name, tuple(labels.shape)))
    if not torch.is_tensor(palette) or palette.dtype != torch.uint8 or tuple(palette.shape) != (256, 3) or not palette.is_contiguous():
        raise RuntimeError("%s: palette must be contiguous uint8 [256, 3]" % name)
    if (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 4 or tuple(out.shape[1:]) != (Ho, Wo, 3) or f_off < 0
            or f_off + F > out.shape[0] or not out.is_contiguous()):
        raise RuntimeError("%s: out must be contiguous CUDA uint8 [>= f_off + F = %d, Ho, Wo, 3]" % (name, f_off + F))
    h0 = w0 = stride = 0
    if frames is not None:
        if (not torch.is_tensor(frames) or frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4
                or int(frames.shape[0]) != F or int(frames.shape[1]) != 3 or frames.shape[2] < 1 or frames.shape[3] < 1):
            raise RuntimeError("%s: frames must be uint8 or float32 [F = %d, 3, h0, w0] or None" % (name, F))
        h0, w0 = int(frames.shape[2]), int(frames.shape[3])
        stride = int(frames.stride(0)) if F > 1 else 3 * h0 * w0
        if tuple(frames.stride()[1:]) != (h0 * w0, w0, 1) or stride < 3 * h0 * w0 or h0 * Ho >= 2 ** 31 or w0 * Wo >= 2 ** 31:
            raise RuntimeError("%s: every frame must be contiguous and the frames a stride >= 3*h0*w0 apart, got strides %s"
                               % (name, tuple(frames.stride())))
    tensors = [(labels, "labels"), (palette, "palette")] + ([(mosaic[0], "action")] if mosaic is not None else [])
    tensors += [(blur[0], "action"), (blur[1], "taps")] if blur is not None else []
    tensors += [(replace[0], "action"), (replace[1], "matte"), (replace[2], "backdrop")] if replace is not None else []
    tensors += [(out, "out"), (frames, "frames")]
    for t, what in tensors:
        if t is not None and (not t.is_cuda or t.device != out.device):
            raise RuntimeError("%s: %s must be a CUDA tensor on out's device, got %s" % (name, what, t.device))
    return F, Ho, Wo, h0, w0, stride


def render_overlay(labels, frames, palette, out, f_off=0, a256=128, contour=1):
    """The picture of a label map: out[f_off + f] (uint8 [>= f_off + F, Ho, Wo, 3], CUDA, contiguous, pixel-interleaved) painted from
    labels (uint8 [F, Ho, Wo], ops.final_label_map's output), frames ([F, 3, h0, w0] uint8 or float32, each frame contiguous, the frames
    any stride >= 3*h0*w0 apart -- a view into a larger store -- or None: onto black) and palette (uint8 [256, 3] in the frames' channel
    order).  Background keeps the frame (nearest-sampled at another size), a labelled pixel becomes (s*(256 - a256) + colour*a256 + 128)
    >> 8, and one with a neighbour of another label within `contour` pixels along an axis, inside the image, the plain colour: the
    integer rule of include/mdqe_hip.h, mdqe_render_overlay_u8.  a256 in 0..256, contour in 0..3.  -> out."""
    F, Ho, Wo, h0, w0, stride = _rgb_paint_args("render_overlay", labels, frames, palette, out, f_off, a256, contour)
    check(lib.mdqe_render_overlay_u8(ptr(frames) if frames is not None else None, int(frames is not None and frames.dtype == torch.uint8),
                                     stride, h0, w0, ptr(labels), F, Ho, Wo, ptr(palette), a256, contour, ptr(out), f_off, cur_stream()),
          "render_overlay")
    return out


def render_mosaic(labels, frames, palette, action, out, f_off=0, a256=128, contour=1, cell=16):
    """`render_overlay` with a per-label action (uint8 [256], action[l]: 0 keep the source, 1 tint as render_overlay does, 2 mosaic;
    action[0] is the background's): a mosaic pixel becomes the rounded mean of its cell x cell square of the output grid (anchored at
    (0, 0), over all in-picture source values of the square whatever their labels; cell even, 2..64).  Every other argument is
    render_overlay's; with action = [0, 1, 1, ...] the picture is render_overlay's bit for bit: the integer rule of
    include/mdqe_hip.h, mdqe_render_mosaic_u8.  -> out."""
    F, Ho, Wo, h0, w0, stride = _rgb_paint_args("render_mosaic", labels, frames, palette, out, f_off, a256, contour, (action, cell))
    check(lib.mdqe_render_mosaic_u8(ptr(frames) if frames is not None else None, int(frames is not None and frames.dtype == torch.uint8),
                                    stride, h0, w0, ptr(labels), F, Ho, Wo, ptr(palette), ptr(action), a256, contour, cell, ptr(out),
                                    f_off, cur_stream()), "render_mosaic")
    return out


REPLACE_MODES = ("background", "tracks")     # mode 0: the matte is the foreground that is kept; 1: the matte covers what is replaced


def render_replace(labels, frames, palette, action, matte, backdrop, out, f_off=0, a256=128, contour=1, mode="background"):
    """`render_overlay` composited over a backdrop by a soft matte: with `base` the pixel of render_overlay under the per-label action
    (uint8 [256], action[l]: 1 tint as render_overlay does, anything else -- 0 keep, 4 replace -- the source), Wt = matte (uint8
    [F, Ho, Wo], ops.final_matte's output) in mode "background" and 255 - matte in mode "tracks",
    out_c = (base_c * Wt + B_c * (255 - Wt) + 127) // 255, where B is `backdrop`: uint8 [3], one colour in the frames' channel order, or
    uint8 [Ho, Wo, 3], one picture for every frame.  Every other argument is render_overlay's: the integer rule of include/mdqe_hip.h,
    mdqe_render_replace_u8.  -> out."""
    if mode not in REPLACE_MODES:
        raise RuntimeError("render_replace: mode must be 'background' or 'tracks', got %r" % (mode,))
    F, Ho, Wo, h0, w0, stride = _rgb_paint_args("render_replace", labels, frames, palette, out, f_off, a256, contour,
                                                replace=(action, matte, backdrop))
    check(lib.mdqe_render_replace_u8(ptr(frames) if frames is not None else None, int(frames is not None and frames.dtype == torch.uint8),
                                     stride, h0, w0, ptr(labels), F, Ho, Wo, ptr(palette), ptr(action), a256, contour, ptr(matte),
                                     ptr(backdrop), int(backdrop.dim() == 3), REPLACE_MODES.index(mode), ptr(out), f_off, cur_stream()),
          "render_replace")
    return out


def render_replace_yuv(labels, yuv, palette_yuv, action, matte, backdrop, out=None, f_off=0, a256=128, contour=1, mode="background"):
    """`render_replace` on decoder surfaces: `render_overlay_yuv` under the per-label action (1 tints, anything else keeps the sample)
    mixed with a backdrop by the matte (uint8 [F, H, W]).  backdrop: uint16 [3], (Y, U, V) in sample units (render.backdrop_yuv), or a
    preprocess.YuvFrames of ONE surface of yuv's size and fmt.  Luma: mix(baseY, BY, Wt); a chroma pair: the rounded mean over its 2 x 2
    block's in-picture pixels of mix(px_i(C), BC, Wt_i); a kept sample at full weight keeps the decoder's bits (P010: all 16 of a word;
    a chroma pair when its whole block is such): the integer rule of include/mdqe_hip.h, mdqe_render_replace_yuv420sp.  `out` may be
    `yuv` itself (in place), nothing else that overlaps it.  On a HIP device one launch on the current stream; on host planes the same
    rule in torch integers.  -> out."""
    from .preprocess import YuvFrames
    name = "render_replace_yuv"
    if mode not in REPLACE_MODES:
        raise RuntimeError("%s: mode must be 'background' or 'tracks', got %r" % (name, mode))
    if not isinstance(yuv, YuvFrames):
        raise RuntimeError("%s: yuv must be a preprocess.YuvFrames, got %s" % (name, type(yuv).__name__))
    F, H, W = len(yuv), yuv.height, yuv.width
    _action_arg(name, action)
    if not torch.is_tensor(matte) or matte.dtype != torch.uint8 or tuple(matte.shape) != (F, H, W) or not matte.is_contiguous():
        raise RuntimeError("%s: matte must be contiguous uint8 [F = %d, %d, %d], the surfaces' own size (ops.final_matte)" % (name, F, H, W))
    surf = isinstance(backdrop, YuvFrames)
    if surf:
        if len(backdrop) != 1 or (backdrop.height, backdrop.width, backdrop.fmt) != (H, W, yuv.fmt):
            raise RuntimeError("%s: a backdrop surface must be a YuvFrames of ONE surface of %d x %d %s" % (name, H, W, yuv.fmt))
    elif (not torch.is_tensor(backdrop) or backdrop.dtype not in (torch.uint16, torch.int16) or tuple(backdrop.shape) != (3,)
          or not backdrop.is_contiguous()):
        raise RuntimeError("%s: backdrop must be contiguous uint16 [3] (render.backdrop_yuv) or a YuvFrames of one surface" % name)
    F, H, W, out = _yuv_paint_args(name, labels, yuv, palette_yuv, out, f_off, a256, contour)
    for t, what in ((action, "action"), (matte, "matte"), (backdrop, "backdrop")):
        if t.device != yuv.device:
            raise RuntimeError("%s: %s must be on the surfaces' device %s, got %s" % (name, what, yuv.device, t.device))
    if yuv.is_cuda:
        from .preprocess import _pitch_stride
        src, dst = _surface_call_args(labels, yuv, palette_yuv, out, F, H, W)
        back = (None, ptr(backdrop.y), _pitch_stride(backdrop.y)[0], ptr(backdrop.uv), _pitch_stride(backdrop.uv)[0]) if surf \
            else (ptr(backdrop), None, 0, None, 0)
        with torch.cuda.device(yuv.device):
            check(lib.mdqe_render_replace_yuv420sp(*src, ptr(action), a256, contour, ptr(matte), *back, REPLACE_MODES.index(mode), *dst, f_off,
                                                   cur_stream(yuv.device)), name)
        return out
    if F == 0:
        return out
    return _replace_yuv_host(labels, yuv, palette_yuv, action, matte, backdrop, out, f_off, a256, contour, REPLACE_MODES.index(mode))


def _replace_yuv_host(labels, yuv, palette_yuv, action, matte, backdrop, out, f_off, a256, contour, mode):
    """mdqe_render_replace_yuv420sp's rule on host planes, in torch integers."""
    F, H, W = len(yuv), yuv.height, yuv.width
    p010 = yuv.fmt == "p010"
    ch, cw = (H + 1) // 2, (W + 1) // 2
    mask = 0x3FF if p010 else 0xFF

    def raw(t):
        v = t.to(torch.int64)
        return v & 0xFFFF if p010 else v

    def store(dst, word):
        dst.copy_(((word + 0x8000) & 0xFFFF) - 0x8000 if p010 else word)

    def up(t):                                      # a chroma-plane quantity at every pixel of its block
        return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]

    def mix(s, b, w):
        return (s * w + b * (255 - w) + 127) // 255
    lab = labels.to(torch.int64)
    tinted = action.to(torch.int64)[lab] == 1
    edge = torch.zeros(lab.shape, dtype=torch.bool)
    for d in range(1, contour + 1):
        if d < H:
            edge[:, d:] |= lab[:, d:] != lab[:, :-d]
            edge[:, :-d] |= lab[:, :-d] != lab[:, d:]
        if d < W:
            edge[:, :, d:] |= lab[:, :, d:] != lab[:, :, :-d]
            edge[:, :, :-d] |= lab[:, :, :-d] != lab[:, :, d:]
    col = (palette_yuv.view(torch.int16).to(torch.int64) & mask)[lab]
    wt = matte.to(torch.int64)
    wt = 255 - wt if mode else wt
    if torch.is_tensor(backdrop):
        B = backdrop.view(torch.int16).to(torch.int64) & mask
        BY, BC = B[0], [B[1], B[2]]
    else:
        by, bc = raw(backdrop.y[:, :H, :W]), raw(backdrop.uv[:, :ch, :2 * cw]).reshape(1, ch, cw, 2)
        BY, BC = (by >> 6 if p010 else by), [up((bc[..., k] >> 6 if p010 else bc[..., k]).expand(F, ch, cw)) for k in (0, 1)]

    def base(s, p):
        return torch.where(tinted, torch.where(edge, p, (s * (256 - a256) + p * a256 + 128) >> 8), s)
    kept = ~tinted & (wt == 255)
    ry = raw(yuv.y[:, :H, :W])
    Y = ry >> 6 if p010 else ry
    yo = mix(base(Y, col[..., 0]), BY, wt)
    rc = raw(yuv.uv[:, :ch, :2 * cw]).reshape(F, ch, cw, 2)
    C = rc >> 6 if p010 else rc

    def blocks(t):                                  # [F, H, W] -> the sum over each 2 x 2 block's in-picture pixels, [F, ch, cw]
        full = torch.zeros((F, 2 * ch, 2 * cw), dtype=torch.int64)
        full[:, :H, :W] = t
        return full.reshape(F, ch, 2, cw, 2).sum((2, 4))
    n = blocks(torch.ones((F, H, W), dtype=torch.int64))
    sh = n >> 1                                     # n = 1, 2, 4: n / 2 = log2(n) = 0, 1, 2
    same = blocks((~kept).to(torch.int64)) == 0
    oc = torch.stack([(blocks(mix(base(up(C[..., k]), col[..., k + 1]), BC[k], wt)) + sh) >> sh for k in (0, 1)], -1)
    # (everything is computed before anything is stored: `out` may be `yuv`)
    store(out.y[f_off:f_off + F, :H, :W], torch.where(kept, ry, yo << 6 if p010 else yo))
    store(out.uv[f_off:f_off + F, :ch, :2 * cw], torch.where(same[..., None], rc, oc << 6 if p010 else oc).reshape(F, ch, 2 * cw))
    return out


def _yuv_paint_args(name, labels, yuv, palette_yuv, out, f_off, a256, contour, mosaic=None, blur=None):
    """The checks of render_overlay_yuv, of render_mosaic_yuv (mosaic = (action, cell)) and of render_blur_yuv (blur = (action, taps,
    taps_c)); allocates `out` when None.  -> (F, H, W, out)."""
    from .preprocess import YuvFrames
    if not isinstance(yuv, YuvFrames):
        raise RuntimeError("%s: yuv must be a preprocess.YuvFrames, got %s" % (name, type(yuv).__name__))
    F, H, W = len(yuv), yuv.height, yuv.width
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or tuple(labels.shape) != (F, H, W) or not labels.is_contiguous():
        raise RuntimeError("%s: labels must be contiguous uint8 [F = %d, H = %d, W = %d] (the surfaces' own size)" % (name, F, H, W))
    if not isinstance(a256, int) or not isinstance(contour, int) or not 0 <= a256 <= 256 or not 0 <= contour <= 3:
        raise RuntimeError("%s: a256 must be an int in 0..256 and contour an int in 0..3, got %r, %r" % (name, a256, contour))
    if mosaic is not None:
        _mosaic_args(name, *mosaic)
    if blur is not None:
        _blur_args(name, *blur, surface=True)
    if F * H * W >= 2 ** 31 - 1:
        raise RuntimeError("%s: F*H*W must stay below 2^31 - 1, got %s" % (name, (F, H, W)))
    if (not torch.is_tensor(palette_yuv) or palette_yuv.dtype not in (torch.uint16, torch.int16) or tuple(palette_yuv.shape) != (256, 3)
            or not palette_yuv.is_contiguous()):
        raise RuntimeError("%s: palette_yuv must be contiguous uint16 [256, 3] (render.palette_yuv)" % name)
    if out is None:
        out = YuvFrames.empty(f_off + F, H, W, fmt=yuv.fmt, device=yuv.device, matrix=yuv.matrix, full_range=yuv.full_range, order=yuv.order)
    if (not isinstance(out, YuvFrames) or (out.height, out.width, out.fmt) != (H, W, yuv.fmt) or not isinstance(f_off, int) or f_off < 0
            or f_off + F > len(out)):
        raise RuntimeError("%s: out must be a YuvFrames of >= f_off + F = %d surfaces of %d x %d %s" % (name, f_off + F, H, W, yuv.fmt))
    tensors = [(labels, "labels"), (palette_yuv, "palette_yuv")] + ([(mosaic[0], "action")] if mosaic is not None else [])
    tensors += ([(blur[0], "action"), (blur[1], "taps"), (blur[2], "taps_c")] if blur is not None else []) + [(out, "out")]
    for t, what in tensors:
        if t.device != yuv.device:
            raise RuntimeError("%s: %s must be on the surfaces' device %s, got %s" % (name, what, yuv.device, t.device))
    return F, H, W, out


def _surface_call_args(labels, yuv, palette_yuv, out, F, H, W):
    """The arguments the two surface entries share: (input planes .. palette), (output planes)."""
    from .preprocess import YUV_FORMATS, _pitch_stride
    (yp, ys), (cp, cs) = _pitch_stride(yuv.y), _pitch_stride(yuv.uv)
    (oyp, oys), (ocp, ocs) = _pitch_stride(out.y), _pitch_stride(out.uv)
    return ((ptr(yuv.y), yp, ys, ptr(yuv.uv), cp, cs, F, H, W, YUV_FORMATS.index(yuv.fmt), ptr(labels), ptr(palette_yuv)),
            (ptr(out.y), oyp, oys, ptr(out.uv), ocp, ocs))


def render_overlay_yuv(labels, yuv, palette_yuv, out=None, f_off=0, a256=128, contour=1):
    """A label map painted straight onto decoder surfaces: out[f_off + f] (a preprocess.YuvFrames of yuv's size and fmt with >= f_off
    + F surfaces, its own pitches; None: F fresh surfaces at a tight pitch) from labels (uint8 [F, H, W], contiguous, at the surfaces'
    own size), yuv (a YuvFrames of F surfaces) and palette_yuv (uint16 [256, 3], rows (Y, U, V) in sample units: render.palette_yuv).
    Luma follows ops.render_overlay's rule per sample; a chroma pair is the rounded mean of its block's painted pixels; a background
    pixel keeps the decoder's bits (P010: all 16 of a word): the integer rule of include/mdqe_hip.h, mdqe_render_overlay_yuv420sp.
    `out` may be `yuv` itself (in place), nothing else that overlaps it.  On a HIP device one launch on the current stream; on host
    planes the same rule in torch integers.  -> out."""
    F, H, W, out = _yuv_paint_args("render_overlay_yuv", labels, yuv, palette_yuv, out, f_off, a256, contour)
    if yuv.is_cuda:
        src, dst = _surface_call_args(labels, yuv, palette_yuv, out, F, H, W)
        with torch.cuda.device(yuv.device):
            check(lib.mdqe_render_overlay_yuv420sp(*src, a256, contour, *dst, f_off, cur_stream(yuv.device)), "render_overlay_yuv")
        return out
    if F == 0:
        return out
    return _paint_yuv_host(labels, yuv, palette_yuv, out, f_off, a256, contour)


def _cell_means(v, cell):
    """v int64 [F, h, w] -> each position's cell mean, (sum + n / 2) / n over the in-picture positions of its cell x cell square."""
    F, h, w = v.shape
    ny, nx = -(-h // cell), -(-w // cell)

    def sums(t):
        full = torch.zeros((F, ny * cell, nx * cell), dtype=torch.int64)
        full[:, :h, :w] = t
        return full.reshape(F, ny, cell, nx, cell).sum((2, 4))
    n = sums(torch.ones_like(v))
    m = (sums(v) + n // 2) // n
    return m.repeat_interleave(cell, dim=1).repeat_interleave(cell, dim=2)[:, :h, :w]


def render_mosaic_yuv(labels, yuv, palette_yuv, action, out=None, f_off=0, a256=128, contour=1, cell=16):
    """`render_overlay_yuv` with a per-label action (as `render_mosaic`): a mosaic pixel's luma is the rounded mean of its cell x cell
    luma square, and it enters its chroma pair's block mean with the mean U / V of the (cell/2) x (cell/2) pairs under that square; a
    pixel of action 0 keeps the decoder's bits (P010: all 16 of a word; a chroma pair when its whole block is kept): the integer rule
    of include/mdqe_hip.h, mdqe_render_mosaic_yuv420sp.  Not in place: `out` must not share memory with `yuv` (a cell's mean reads
    samples other threads write).  On a HIP device one launch on the current stream; on host planes the same rule in torch
    integers.  -> out."""
    F, H, W, out = _yuv_paint_args("render_mosaic_yuv", labels, yuv, palette_yuv, out, f_off, a256, contour, (action, cell))
    if yuv.is_cuda:
        src, dst = _surface_call_args(labels, yuv, palette_yuv, out, F, H, W)
        with torch.cuda.device(yuv.device):
            check(lib.mdqe_render_mosaic_yuv420sp(*src, ptr(action), a256, contour, cell, *dst, f_off, cur_stream(yuv.device)),
                  "render_mosaic_yuv")
        return out
    if F == 0:
        return out
    _host_planes_apart("render_mosaic_yuv", "mosaic", yuv, out, f_off, F)
    return _paint_yuv_host(labels, yuv, palette_yuv, out, f_off, a256, contour, action, cell)


def _host_planes_apart(name, what, yuv, out, f_off, F):
    """The host paths' refusal of an `out` that shares memory with `yuv` (a mosaic and a blur are not painted in place)."""
    def span(t):                                    # the bytes a plane's view reaches
        return t.data_ptr(), t.data_ptr() + (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size()
    for src in (yuv.y, yuv.uv):
        for dst in (out.y[f_off:f_off + F], out.uv[f_off:f_off + F]):
            (a0, a1), (b0, b1) = span(src), span(dst)
            if a0 < b1 and b0 < a1:
                raise RuntimeError("%s: out must not share memory with yuv (the %s is not painted in place)" % (name, what))


def _blur_edge(name, edge):
    """The `edge` of render_blur / render_blur_yuv: "bleed", the plain Gaussian, or "stop", the blur that stays inside the blurred region."""
    if edge not in ("bleed", "stop"):
        raise RuntimeError("%s: edge must be 'bleed' or 'stop', got %r" % (name, edge))
    return edge == "stop"


def render_blur(labels, frames, palette, action, taps, out, f_off=0, a256=128, contour=1, edge="bleed"):
    """`render_overlay` with a per-label action (uint8 [256], action[l]: 0 keep the source, 1 tint as render_overlay does, 3 blur, any
    other value as 0; action[0] is the background's): a blur pixel becomes the separable Gaussian of the OUTPUT grid's source values
    with the integer taps `taps` (uint16 [radius + 1], radius 0..32, taps[0] + 2 * sum(taps[1:]) == 4096: render.blur_taps), the
    picture's border replicated, over all pixels under the kernel whatever their labels.  Every other argument is render_overlay's;
    with action = [0, 1, 1, ...] the picture is render_overlay's bit for bit: the integer rule of include/mdqe_hip.h,
    mdqe_render_blur_u8.  edge="stop": the blur stays inside the blurred region -- the taps weigh only pixels of action 3 and the
    sums are normalised by the weight they met (one exact division per sample), so nothing that is kept or tinted bleeds into a
    blurred pixel: mdqe_render_blur_within_u8 (csrc/render_blur_within.hip), same arguments, same checks.  -> out."""
    stop = _blur_edge("render_blur", edge)
    F, Ho, Wo, h0, w0, stride = _rgb_paint_args("render_blur", labels, frames, palette, out, f_off, a256, contour, blur=(action, taps))
    entry = lib.mdqe_render_blur_within_u8 if stop else lib.mdqe_render_blur_u8
    check(entry(ptr(frames) if frames is not None else None, int(frames is not None and frames.dtype == torch.uint8),
                stride, h0, w0, ptr(labels), F, Ho, Wo, ptr(palette), ptr(action), a256, contour, ptr(taps),
                int(taps.numel()) - 1, ptr(out), f_off, cur_stream()), "render_blur")
    return out


def render_blur_yuv(labels, yuv, palette_yuv, action, taps, taps_c, out=None, f_off=0, a256=128, contour=1, edge="bleed"):
    """`render_overlay_yuv` with a per-label action (as `render_blur`): a blur pixel's luma is the Gaussian of the luma plane with
    `taps`, and it enters its chroma pair's block mean with the pair's U / V blurred on the chroma plane's own ceil(H/2) x ceil(W/2)
    grid with `taps_c` (uint16 [radius_c + 1], radius_c 0..16); a pixel that is kept keeps the decoder's bits (P010: all 16 of a word;
    a chroma pair when its whole block is kept): the integer rule of include/mdqe_hip.h, mdqe_render_blur_yuv420sp.  Not in place:
    `out` must not share memory with `yuv` (the taps read samples other threads write).  On a HIP device one launch on the current
    stream; on host planes the same rule in torch integers.  edge="stop": the blur stays inside the blurred region, as
    render_blur's -- luma among the pixels of action 3, U and V among the pairs whose block holds such a pixel:
    mdqe_render_blur_within_yuv420sp, on the device and on host planes alike.  -> out."""
    stop = _blur_edge("render_blur_yuv", edge)
    F, H, W, out = _yuv_paint_args("render_blur_yuv", labels, yuv, palette_yuv, out, f_off, a256, contour, blur=(action, taps, taps_c))
    if yuv.is_cuda:
        src, dst = _surface_call_args(labels, yuv, palette_yuv, out, F, H, W)
        with torch.cuda.device(yuv.device):
            entry = lib.mdqe_render_blur_within_yuv420sp if stop else lib.mdqe_render_blur_yuv420sp
            check(entry(*src, ptr(action), a256, contour, ptr(taps), int(taps.numel()) - 1, ptr(taps_c),
                        int(taps_c.numel()) - 1, *dst, f_off, cur_stream(yuv.device)), "render_blur_yuv")
        return out
    if F == 0:
        return out
    _host_planes_apart("render_blur_yuv", "blur", yuv, out, f_off, F)
    return _paint_yuv_host(labels, yuv, palette_yuv, out, f_off, a256, contour, action, taps=(taps, taps_c), within=stop)


def _tap_sums(t, dim, taps):
    """sum_d taps[|d|] * t[.. + d ..] along `dim` of an int64 tensor, the border replicated: one pass of the blurs, not rounded."""
    w = (taps.view(torch.int16).to(torch.int64) & 0xFFFF).tolist()
    R = len(w) - 1
    n = t.shape[dim]
    idx = torch.arange(n)
    acc = torch.zeros_like(t)
    for d in range(-R, R + 1):
        acc += w[abs(d)] * t.index_select(dim, (idx + d).clamp(0, n - 1))
    return acc


def _blur_plane(v, taps):
    """v int64 [F, h, w] -> the blur of include/mdqe_hip.h: rows first, (sum + 128) >> 8, then columns, (sum + 32768) >> 16, the
    border replicated."""
    return (_tap_sums((_tap_sums(v, 2, taps) + 128) >> 8, 1, taps) + 32768) >> 16


def _blur_plane_within(v, member, taps):
    """v int64 [F, h, w], member bool [F, h, w] -> the edge-stopping blur of include/mdqe_hip.h (mdqe_render_blur_within_u8): the taps
    weigh member * v and member, rows then columns with no rounding between, the border replicated with its membership, then
    (N + D // 2) // D where `member`, 0 elsewhere (there the value is not defined and D may be 0).  N stays below 2^34."""
    m = member.to(torch.int64)
    N, D = _tap_sums(_tap_sums(m * v, 2, taps), 1, taps), _tap_sums(_tap_sums(m, 2, taps), 1, taps)
    return torch.where(member, (N + D // 2) // D.clamp(min=1), torch.zeros_like(N))


def _annotate_args(name, geom, n, palette, ink, captions, font, f_off, box, scale, min_area, table_dtypes):
    """The checks annotate and annotate_yuv share.  -> (frames of the call, cap_len)."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 255:
        raise RuntimeError("%s: n must be an int in 0..255, got %r" % (name, n))
    for what, v, lo, hi in (("box", box, 0, 4), ("scale", scale, 1, 4), ("min_area", min_area, 0, 2 ** 31 - 1), ("f_off", f_off, 0, 2 ** 31 - 1)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise RuntimeError("%s: %s must be an int in %d..%d, got %r" % (name, what, lo, hi, v))
    if (not torch.is_tensor(geom) or geom.dtype != torch.int32 or not geom.is_contiguous() or geom.dim() not in (2, 3) or geom.shape[-1] != 5
            or (geom.dim() == 3 and int(geom.shape[0]) != n) or (n and (geom.numel() // 5) % n)):
        raise RuntimeError("%s: geom must be contiguous int32 [n * F, 5] or [n = %d, F, 5] (ops.final_label_map's table)" % (name, n))
    F = geom.numel() // 5 // n if n else 0
    for what, t in (("palette", palette), ("ink", ink)):
        if not torch.is_tensor(t) or t.dtype not in table_dtypes or tuple(t.shape) != (256, 3) or not t.is_contiguous():
            raise RuntimeError("%s: %s must be contiguous %s [256, 3]" % (name, what, str(table_dtypes[0]).replace("torch.", "")))
    if captions is not None and (not torch.is_tensor(captions) or captions.dtype != torch.uint8 or captions.dim() != 2
                                 or int(captions.shape[0]) != 256 or not 1 <= captions.shape[1] <= 64 or not captions.is_contiguous()):
        raise RuntimeError("%s: captions must be None or contiguous uint8 [256, 1..64] (render.captions)" % name)
    if not torch.is_tensor(font) or font.dtype != torch.uint8 or tuple(font.shape) != (64, 7) or not font.is_contiguous():
        raise RuntimeError("%s: font must be contiguous uint8 [64, 7] (render.default_font)" % name)
    return F, int(captions.shape[1]) if captions is not None else 0


def annotate(pic, geom, n, palette, ink, captions, font, f_off=0, box=0, scale=1, min_area=0):
    """Track boxes and captions drawn onto a painted picture, in place: pic (uint8 [>= f_off + F, Ho, Wo, 3], CUDA, contiguous -- what
    ops.render_overlay / ops.render_mosaic painted) gets, in its frames f_off .. f_off + F - 1 and for each label l = 1..n whose row of
    geom (int32 [n * F, 5] or [n, F, 5], row (l - 1) * F + f = (area, xmin, ymin, xmax, ymax): ops.final_label_map's table) is live
    (area >= max(1, min_area), the box inside the picture), a frame of `box` pixels along its box in palette[l] (box 0: none) and, with
    captions (uint8 [256, cap_len <= 64], render.captions; None: none), a plate in palette[l] at the box's top left corner that holds
    row l of captions in ink[l], drawn from font (uint8 [64, 7], render.default_font) at `scale` pixels per font pixel.  Plates lie
    over frames, lower labels over higher ones; a pixel that nothing hits is not written: the integer rule of include/mdqe_hip.h,
    mdqe_annotate_u8.  One launch on the current stream, none when F == 0, n == 0 or there is nothing to draw.  -> pic."""
    F, cap_len = _annotate_args("annotate", geom, n, palette, ink, captions, font, f_off, box, scale, min_area, (torch.uint8,))
    if not torch.is_tensor(pic) or pic.dtype != torch.uint8 or pic.dim() != 4 or int(pic.shape[3]) != 3 or not pic.is_contiguous():
        raise RuntimeError("annotate: pic must be contiguous uint8 [frames, Ho, Wo, 3]")
    Ho, Wo = int(pic.shape[1]), int(pic.shape[2])
    if Ho < 1 or Wo < 1 or f_off + F > pic.shape[0] or F * Ho * Wo >= 2 ** 31 - 1:
        raise RuntimeError("annotate: pic %s must hold frames f_off .. f_off + F = %d of positive size, F*Ho*Wo < 2^31 - 1" % (tuple(pic.shape), f_off + F))
    for t, what in ((pic, "pic"), (geom, "geom"), (palette, "palette"), (ink, "ink"), (captions, "captions"), (font, "font")):
        if t is not None and (not t.is_cuda or t.device != pic.device):
            raise RuntimeError("annotate: %s must be a CUDA tensor on pic's device, got %s" % (what, t.device))
    with torch.cuda.device(pic.device):
        check(lib.mdqe_annotate_u8(ptr(pic), F, Ho, Wo, f_off, ptr(geom), n, ptr(palette), ptr(ink), ptr(captions), cap_len, ptr(font),
                                   box, scale, min_area, cur_stream(pic.device)), "annotate")
    return pic


def annotate_yuv(yuv, geom, n, palette_yuv, ink_yuv, captions, font, f_off=0, box=0, scale=1, min_area=0):
    """`annotate` on painted decoder surfaces, in place: yuv (a preprocess.YuvFrames on a HIP device, NV12 or P010 -- what
    ops.render_overlay_yuv / ops.render_mosaic_yuv painted) gets the same boxes and plates in its surfaces f_off .. f_off + F - 1, with
    palette_yuv and ink_yuv (uint16 [256, 3], rows (Y, U, V) in sample units: render.palette_yuv of the palette and of render.ink).
    Luma follows the rule per sample; a chroma pair with a hit in its 2 x 2 block becomes the rounded mean of the hits' components and
    the stored value for the block's other pixels, a pair without a hit keeps its bits: the integer rule of include/mdqe_hip.h,
    mdqe_annotate_yuv420sp.  -> yuv."""
    from .preprocess import YUV_FORMATS, YuvFrames, _pitch_stride
    F, cap_len = _annotate_args("annotate_yuv", geom, n, palette_yuv, ink_yuv, captions, font, f_off, box, scale, min_area, (torch.uint16, torch.int16))
    if not isinstance(yuv, YuvFrames):
        raise RuntimeError("annotate_yuv: yuv must be a preprocess.YuvFrames, got %s" % type(yuv).__name__)
    H, W = yuv.height, yuv.width
    if f_off + F > len(yuv) or F * H * W >= 2 ** 31 - 1:
        raise RuntimeError("annotate_yuv: yuv holds %d surfaces, the call needs f_off + F = %d, F*H*W < 2^31 - 1" % (len(yuv), f_off + F))
    if not yuv.is_cuda:
        raise RuntimeError("annotate_yuv: the surfaces must be on a HIP device, got %s (the annotation pass has no host path)" % (yuv.device,))
    for t, what in ((geom, "geom"), (palette_yuv, "palette_yuv"), (ink_yuv, "ink_yuv"), (captions, "captions"), (font, "font")):
        if t is not None and t.device != yuv.device:
            raise RuntimeError("annotate_yuv: %s must be on the surfaces' device %s, got %s" % (what, yuv.device, t.device))
    (yp, ys), (cp, cs) = _pitch_stride(yuv.y), _pitch_stride(yuv.uv)
    with torch.cuda.device(yuv.device):
        check(lib.mdqe_annotate_yuv420sp(ptr(yuv.y), yp, ys, ptr(yuv.uv), cp, cs, F, H, W, YUV_FORMATS.index(yuv.fmt), f_off, ptr(geom), n,
                                         ptr(palette_yuv), ptr(ink_yuv), ptr(captions), cap_len, ptr(font), box, scale, min_area,
                                         cur_stream(yuv.device)), "annotate_yuv")
    return yuv


def _crop_args(name, labels, n_frames, device, geom, n, size, out, c_off, rects, first, step, pad256, min_area, cutout, fill):
    """The checks track_crops and track_crops_yuv share; allocates `out` / `rects` when None.
    -> (F, Ho, Wo, Sh, Sw, frames taken, packed fill, out, rects)."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise RuntimeError("%s: labels must be contiguous uint8 [F, Ho, Wo]" % name)
    F, Ho, Wo = (int(v) for v in labels.shape)
    if n_frames != F:
        raise RuntimeError("%s: labels hold F = %d frames, the frames handed in %d" % (name, F, n_frames))
    if Ho < 1 or Wo < 1 or Ho * Wo >= 2 ** 24:
        raise RuntimeError("%s: Ho, Wo must be positive with Ho*Wo < 2^24, got %s" % (name, tuple(labels.shape)))
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 255:
        raise RuntimeError("%s: n must be an int in 0..255, got %r" % (name, n))
    if (not isinstance(size, (tuple, list)) or len(size) != 2
            or any(isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= 512 for v in size)):
        raise RuntimeError("%s: size must be (Sh, Sw), ints in 1..512, got %r" % (name, size))
    Sh, Sw = size
    for what, v, lo, hi in (("pad256", pad256, 0, 256), ("min_area", min_area, 0, 2 ** 31 - 1), ("c_off", c_off, 0, 2 ** 31 - 1),
                            ("first", first, 0, 2 ** 31 - 1), ("step", step, 1, 2 ** 31 - 1)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise RuntimeError("%s: %s must be an int in %d..%d, got %r" % (name, what, lo, hi, v))
    if cutout not in (False, True, 0, 1):
        raise RuntimeError("%s: cutout must be a bool, got %r" % (name, cutout))
    if (not isinstance(fill, (tuple, list)) or len(fill) != 3
            or any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255 for v in fill)):
        raise RuntimeError("%s: fill must be three ints in 0..255 (the frames' channel order), got %r" % (name, fill))
    if (not torch.is_tensor(geom) or geom.dtype != torch.int32 or not geom.is_contiguous() or geom.dim() not in (2, 3) or geom.shape[-1] != 5
            or (geom.dim() == 3 and int(geom.shape[0]) != n) or geom.numel() != n * F * 5):
        raise RuntimeError("%s: geom must be contiguous int32 [n * F = %d, 5] or [n = %d, F = %d, 5] (ops.final_label_map's table)"
                           % (name, n * F, n, F))
    Fc = len(range(first, F, step))
    chips = c_off + Fc
    if chips * Sh * Sw * 3 >= 2 ** 31 - 1:
        raise RuntimeError("%s: (c_off + frames taken) * Sh * Sw * 3 must stay below 2^31 - 1, got %d chips of %d x %d" % (name, chips, Sh, Sw))
    if out is None:
        out = torch.empty((n, chips, Sh, Sw, 3), dtype=torch.uint8, device=device)
    if (not torch.is_tensor(out) or out.dtype != torch.uint8 or out.dim() != 5 or tuple(out.shape[2:]) != (Sh, Sw, 3) or out.shape[0] < n
            or out.shape[1] < chips or tuple(out.stride()[1:]) != (Sh * Sw * 3, Sw * 3, 3, 1)
            or (out.shape[0] > 1 and out.stride(0) < out.shape[1] * Sh * Sw * 3)):
        raise RuntimeError("%s: out must be uint8 [>= n = %d, >= c_off + frames taken = %d, Sh = %d, Sw = %d, 3], each row contiguous and the "
                           "rows apart" % (name, n, chips, Sh, Sw))
    if rects is None:
        rects = torch.empty((n, chips, 4), dtype=torch.int32, device=device)
    if (not torch.is_tensor(rects) or rects.dtype != torch.int32 or rects.dim() != 3 or int(rects.shape[2]) != 4 or rects.shape[0] < n
            or rects.shape[1] < chips or tuple(rects.stride()[1:]) != (4, 1) or (rects.shape[0] > 1 and rects.stride(0) < rects.shape[1] * 4)):
        raise RuntimeError("%s: rects must be int32 [>= n = %d, >= c_off + frames taken = %d, 4], each row contiguous and the rows apart"
                           % (name, n, chips))
    for t, what in ((labels, "labels"), (geom, "geom"), (out, "out"), (rects, "rects")):
        if not t.is_cuda or t.device != torch.device(device):
            raise RuntimeError("%s: %s must be a CUDA tensor on the frames' device, got %s" % (name, what, t.device))
    return F, Ho, Wo, Sh, Sw, Fc, fill[0] | fill[1] << 8 | fill[2] << 16, out, rects


def _row_stride(t, row_elems):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]) * row_elems


def track_crops(labels, frames, geom, n, size, out=None, c_off=0, rects=None, first=0, step=1, pad256=0, min_area=0, cutout=False,
                fill=(0, 0, 0)):
    """One fixed-size picture per track and frame, cut and resized on the device: for rows k = 0..n-1 (label k + 1) and the window
    frames f = first, first + step, ... < F, the t-th of them into out[k, c_off + t] (uint8 [>= n, >= c_off + frames taken, Sh, Sw, 3],
    CUDA, pixel-interleaved, rows any stride apart; None: allocated, [n, c_off + taken, Sh, Sw, 3]) and its source rect (X0, Y0, X1, Y1),
    inclusive, in output pixels into rects[k, c_off + t] (int32 [>= n, >= c_off + taken, 4]; None: allocated).  labels: uint8 [F, Ho, Wo]
    (ops.final_label_map's output), frames: [F, 3, h0, w0] uint8 or float32 (ops.render_overlay's: a view into a larger store works),
    geom: int32 [n * F, 5] or [n, F, 5], the table ops.final_label_map writes.  A row's box grows by pad256/256 of its size per side,
    clamped to the picture; chip pixel (i, j) is the rounded mean of the source pixels of its footprint in that rect (a smaller rect is
    replicated) -- with `cutout` of those the track owns, `fill` where it owns none.  A row that is not live (area < max(1, min_area),
    or no box) gives a chip of `fill` and the rect (0, 0, -1, -1): the integer rule of include/mdqe_hip.h, mdqe_track_crops_u8.  One
    launch on the current stream, none when n == 0 or no frame is taken.  -> (out, rects)."""
    if (not torch.is_tensor(frames) or frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4 or int(frames.shape[1]) != 3
            or frames.shape[2] < 1 or frames.shape[3] < 1):
        raise RuntimeError("track_crops: frames must be uint8 or float32 [F, 3, h0, w0]")
    h0, w0 = int(frames.shape[2]), int(frames.shape[3])
    stride = int(frames.stride(0)) if frames.shape[0] > 1 else 3 * h0 * w0
    if tuple(frames.stride()[1:]) != (h0 * w0, w0, 1) or stride < 3 * h0 * w0:
        raise RuntimeError("track_crops: every frame must be contiguous and the frames a stride >= 3*h0*w0 apart, got strides %s"
                           % (tuple(frames.stride()),))
    F, Ho, Wo, Sh, Sw, Fc, packed, out, rects = _crop_args("track_crops", labels, int(frames.shape[0]), frames.device, geom, n, size, out,
                                                           c_off, rects, first, step, pad256, min_area, cutout, fill)
    if h0 * Ho >= 2 ** 31 - 1 or w0 * Wo >= 2 ** 31 - 1:
        raise RuntimeError("track_crops: h0*Ho and w0*Wo must stay below 2^31 - 1")
    with torch.cuda.device(frames.device):
        check(lib.mdqe_track_crops_u8(ptr(frames), int(frames.dtype == torch.uint8), stride, h0, w0, ptr(labels), F, Ho, Wo, ptr(geom), n,
                                      first, step, Sh, Sw, pad256, min_area, int(cutout), packed, ptr(out), _row_stride(out, Sh * Sw * 3),
                                      c_off, ptr(rects), _row_stride(rects, 4), cur_stream(frames.device)), "track_crops")
    return out, rects


def track_crops_yuv(labels, yuv, geom, n, size, out=None, c_off=0, rects=None, first=0, step=1, pad256=0, min_area=0, cutout=False,
                    fill=(0, 0, 0)):
    """`track_crops` from decoder surfaces: yuv is a preprocess.YuvFrames of F surfaces on a HIP device (NV12 or P010); a source pixel is
    the RGB -- in the surfaces' `order` -- that preprocess.yuv_to_rgb gives for that sample, so the chips equal
    track_crops(labels, yuv_to_rgb(yuv), ...) bit for bit without the converted frames ever being stored: the integer rule of
    include/mdqe_hip.h, mdqe_track_crops_yuv420sp.  -> (out, rects)."""
    from .preprocess import YUV_FORMATS, YUV_MATRICES, YuvFrames, _pitch_stride
    if not isinstance(yuv, YuvFrames):
        raise RuntimeError("track_crops_yuv: yuv must be a preprocess.YuvFrames, got %s" % type(yuv).__name__)
    if not yuv.is_cuda:
        raise RuntimeError("track_crops_yuv: the surfaces must be on a HIP device, got %s (the crops have no host path)" % (yuv.device,))
    F, Ho, Wo, Sh, Sw, Fc, packed, out, rects = _crop_args("track_crops_yuv", labels, len(yuv), yuv.device, geom, n, size, out, c_off, rects,
                                                           first, step, pad256, min_area, cutout, fill)
    H, W = yuv.height, yuv.width
    if H * Ho >= 2 ** 31 - 1 or W * Wo >= 2 ** 31 - 1:
        raise RuntimeError("track_crops_yuv: H*Ho and W*Wo must stay below 2^31 - 1")
    (yp, ys), (cp, cs) = _pitch_stride(yuv.y), _pitch_stride(yuv.uv)
    with torch.cuda.device(yuv.device):
        check(lib.mdqe_track_crops_yuv420sp(ptr(yuv.y), yp, ys, ptr(yuv.uv), cp, cs, H, W, YUV_FORMATS.index(yuv.fmt),
                                            YUV_MATRICES.index(yuv.matrix), int(yuv.full_range), int(yuv.order == "bgr"), ptr(labels), F, Ho,
                                            Wo, ptr(geom), n, first, step, Sh, Sw, pad256, min_area, int(cutout), packed, ptr(out),
                                            _row_stride(out, Sh * Sw * 3), c_off, ptr(rects), _row_stride(rects, 4),
                                            cur_stream(yuv.device)), "track_crops_yuv")
    return out, rects


def _point_table(name, pts, n, cols):
    """The checks of a point table (ops.label_centroids writes it, ops.render_trails reads it): int32 [>= n, >= cols, 2], each row
    contiguous and the rows apart.  -> its row stride in elements."""
    if (not torch.is_tensor(pts) or pts.dtype != torch.int32 or pts.dim() != 3 or int(pts.shape[2]) != 2 or pts.shape[0] < n
            or pts.shape[1] < cols or tuple(pts.stride()[1:]) != (2, 1) or (pts.shape[0] > 1 and pts.stride(0) < pts.shape[1] * 2)):
        raise RuntimeError("%s: pts must be int32 [>= n = %d, >= p_off + F = %d, 2], each row contiguous and the rows apart" % (name, n, cols))
    return _row_stride(pts, 2)


def label_centroids(labels, n, min_area=0, mom=None, pts=None, p_off=0):
    """Where each track is: for rows k = 0..n-1 (label k + 1) and the frames f of labels (uint8 [F, Ho, Wo], CUDA, contiguous:
    ops.final_label_map's output), mom[k, f] = (m, SX, SY) (int64 [n, F, 3] or [n * F, 3], contiguous; None: allocated): the pixels
    that hold the label, the sum of their X and of their Y; and the centroid of the visible region, ((SX + m/2) / m, (SY + m/2) / m) in
    integer division where m >= max(1, min_area) and (-1, -1) elsewhere, into pts[k, p_off + f] (int32 [>= n, >= p_off + F, 2], rows any
    stride apart -- a table whose columns are frames, kept over several windows; None: allocated, [n, p_off + F, 2], the columns below
    p_off -1; False: the moments alone).  Both are fully overwritten; integers only, identical from run to run: the rule of
    include/mdqe_hip.h, mdqe_label_centroids_u8.  At most three launches on the current stream, none when n == 0 or F == 0.
    -> (mom, pts or None)."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise RuntimeError("label_centroids: labels must be contiguous uint8 [F, Ho, Wo]")
    F, Ho, Wo = (int(v) for v in labels.shape)
    if Ho < 1 or Wo < 1 or Ho > 16384 or Wo > 16384 or F * Ho * Wo >= 2 ** 31 - 1:
        raise RuntimeError("label_centroids: Ho, Wo must be in 1..16384 with F*Ho*Wo < 2^31 - 1, got %s" % (tuple(labels.shape),))
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 255:
        raise RuntimeError("label_centroids: n must be an int in 0..255, got %r" % (n,))
    for what, v in (("min_area", min_area), ("p_off", p_off)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 2 ** 31 - 1:
            raise RuntimeError("label_centroids: %s must be an int in 0..%d, got %r" % (what, 2 ** 31 - 1, v))
    if mom is None:
        mom = torch.empty((n, F, 3), dtype=torch.int64, device=labels.device)
    if (not torch.is_tensor(mom) or mom.dtype != torch.int64 or not mom.is_contiguous() or mom.dim() not in (2, 3) or mom.shape[-1] != 3
            or mom.numel() != n * F * 3 or (mom.dim() == 3 and int(mom.shape[0]) != n)):
        raise RuntimeError("label_centroids: mom must be contiguous int64 [n * F = %d, 3] or [n = %d, F = %d, 3]" % (n * F, n, F))
    stride = 2 * (p_off + F)
    if pts is None:
        pts = torch.full((n, p_off + F, 2), -1, dtype=torch.int32, device=labels.device)
    if pts is not False:
        stride = _point_table("label_centroids", pts, n, p_off + F)
    for t, what in ((labels, "labels"), (mom, "mom"), (pts, "pts")):
        if t is not False and (not t.is_cuda or t.device != labels.device):
            raise RuntimeError("label_centroids: %s must be a CUDA tensor on the labels' device, got %s" % (what, t.device))
    with torch.cuda.device(labels.device):
        check(lib.mdqe_label_centroids_u8(ptr(labels), F, Ho, Wo, n, min_area, ptr(mom), ptr(pts) if pts is not False and n else None,
                                          stride, p_off, cur_stream(labels.device)), "label_centroids")
    return mom, (None if pts is False else pts)


def label_polygons(labels, n, min_area=0, cap_vertices=None, cap_rings=None):
    """The outlines of each track's visible region: for rows k = 0..n-1 (label k + 1) and the frames f of labels (uint8 [F, Ho, Wo],
    CUDA, contiguous: ops.final_label_map's output) the closed rings of lattice corners around the pixels that hold the label -- the
    rule of include/mdqe_hip.h, mdqe_label_polygons_u8: the region on the right of every edge, corners only, a ring from its smallest
    corner (f, Y, X, heading), the rings by ascending start, holes flagged.  -> (xy int32 [cap_vertices, 2]: (X, Y), ring after ring;
    rings int32 [cap_rings, 5]: (row k, frame f, first vertex, vertex count, hole); totals int32 [2]: the TRUE vertex and ring counts),
    all on the device.  Where a count exceeds its cap, xy and rings hold nothing of use: call again with the counts as caps
    (merge.polygon_rings does).  Regions of fewer than max(1, min_area) pixels have no rings.  Default caps: F * 16 * (Ho + Wo) + 1024
    vertices and a quarter of that for rings, generous for anything mask-like.  Integers only, identical from run to run; the
    workspace is ops._workspace's; n == 0 or F == 0 write the totals and launch nothing else."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise RuntimeError("label_polygons: labels must be contiguous uint8 [F, Ho, Wo]")
    F, Ho, Wo = (int(v) for v in labels.shape)
    if Ho < 1 or Wo < 1 or Ho > 16384 or Wo > 16384 or F * Ho * Wo >= 2 ** 31 - 1:
        raise RuntimeError("label_polygons: Ho, Wo must be in 1..16384 with F*Ho*Wo < 2^31 - 1, got %s" % (tuple(labels.shape),))
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 255:
        raise RuntimeError("label_polygons: n must be an int in 0..255, got %r" % (n,))
    if isinstance(min_area, bool) or not isinstance(min_area, int) or not 0 <= min_area <= 2 ** 31 - 1:
        raise RuntimeError("label_polygons: min_area must be an int in 0..%d, got %r" % (2 ** 31 - 1, min_area))
    if cap_vertices is None:
        cap_vertices = min(F * 16 * (Ho + Wo) + 1024, 2 ** 26)
    if cap_rings is None:
        cap_rings = min(max(cap_vertices // 4, 1), 2 ** 24)
    for what, v, hi in (("cap_vertices", cap_vertices, 2 ** 26), ("cap_rings", cap_rings, 2 ** 24)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
            raise RuntimeError("label_polygons: %s must be an int in 1..%d, got %r" % (what, hi, v))
    if not labels.is_cuda:
        raise RuntimeError("label_polygons: labels must be a CUDA tensor, got %s" % (labels.device,))
    xy = torch.empty((cap_vertices, 2), dtype=torch.int32, device=labels.device)
    rings = torch.empty((cap_rings, 5), dtype=torch.int32, device=labels.device)
    totals = torch.empty(2, dtype=torch.int32, device=labels.device)
    with torch.cuda.device(labels.device):
        need = int(lib.mdqe_label_polygons_workspace(F, Ho, Wo, cap_vertices))
        if need < 0:
            raise RuntimeError("label_polygons: no workspace for labels %s with cap_vertices = %d" % (tuple(labels.shape), cap_vertices))
        ws = _workspace(need, labels.device)
        check(lib.mdqe_label_polygons_u8(ptr(labels), F, Ho, Wo, n, min_area, cap_vertices, cap_rings, ptr(xy), ptr(rings), ptr(totals),
                                         ptr(ws), ws.numel(), cur_stream(labels.device)), "label_polygons")
    return xy, rings, totals


def grow_labels(labels, grow, radius, out=None):
    """The redaction margin: a copy of labels (uint8 [F, Ho, Wo], CUDA, contiguous: ops.final_label_map's output) in which the labels
    that `grow` (uint8 [256] on the same device; entry 0 is ignored) marks have grown by up to `radius` pixels (an int in 0..32) over
    the background and over the tracks that do not grow -- the rule of include/mdqe_hip.h, mdqe_grow_labels_u8: a pixel whose label
    grows keeps it, any other takes the label of the nearest growing pixel of its frame within the Euclidean radius, of equally near
    ones the smallest label.  `out`: a buffer of labels' shape that shares no byte with labels or grow (None: allocated), fully
    overwritten.  The painters (ops.render_overlay and the others) take the result in place of the label map.  Integers only, identical
    from run to run; one launch on the current stream, none for an empty map.  -> out."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if not torch.is_tensor(labels) or labels.dtype != torch.uint8 or labels.dim() != 3 or not labels.is_contiguous():
        raise RuntimeError("grow_labels: labels must be contiguous uint8 [F, Ho, Wo]")
    F, Ho, Wo = (int(v) for v in labels.shape)
    if F * Ho * Wo >= 2 ** 31 - 1:
        raise RuntimeError("grow_labels: F*Ho*Wo must be < 2^31 - 1, got %s" % (tuple(labels.shape),))
    if not torch.is_tensor(grow) or grow.dtype != torch.uint8 or tuple(grow.shape) != (256,) or not grow.is_contiguous():
        raise RuntimeError("grow_labels: grow must be contiguous uint8 [256] (entry l: whether label l grows)")
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= 32:
        raise RuntimeError("grow_labels: radius must be an int in 0..32, got %r" % (radius,))
    if out is None:
        out = torch.empty_like(labels)
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (F, Ho, Wo) or not out.is_contiguous():
        raise RuntimeError("grow_labels: out must be contiguous uint8 %s, the labels' shape" % ((F, Ho, Wo),))
    for t, what in ((labels, "labels"), (grow, "grow"), (out, "out")):
        if not t.is_cuda or t.device != labels.device:
            raise RuntimeError("grow_labels: %s must be a CUDA tensor on the labels' device, got %s" % (what, t.device))
    n = F * Ho * Wo
    if n and (max(out.data_ptr(), labels.data_ptr()) < min(out.data_ptr(), labels.data_ptr()) + n
              or (out.data_ptr() < grow.data_ptr() + 256 and grow.data_ptr() < out.data_ptr() + n)):
        raise RuntimeError("grow_labels: out must not share memory with labels or grow (a pixel reads its neighbours' labels)")
    with torch.cuda.device(labels.device):
        check(lib.mdqe_grow_labels_u8(ptr(labels), F, Ho, Wo, ptr(grow), radius, ptr(out), cur_stream(labels.device)), "grow_labels")
    return out


def _plate_state(name, what, t, shape):
    if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
        raise RuntimeError("%s: %s must be contiguous int32 %s (merge.Plate holds it)" % (name, what, list(shape)))


def _plate_rgb(name, plate):
    if not torch.is_tensor(plate) or plate.dtype != torch.int32 or plate.dim() != 3 or plate.shape[2] != 4 or not plate.is_contiguous():
        raise RuntimeError("%s: plate must be contiguous int32 [Ho, Wo, 4] (merge.Plate holds it)" % name)
    return int(plate.shape[0]), int(plate.shape[1])


def _plate_int(name, what, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise RuntimeError("%s: %s must be an int in %d..%d, got %r" % (name, what, lo, hi, v))


def _plate_block(name, block, F, H, W):
    if not torch.is_tensor(block) or block.dtype != torch.uint8 or tuple(block.shape) != (F, H, W) or not block.is_contiguous():
        raise RuntimeError("%s: block must be contiguous uint8 [F = %d, %d, %d] (the label map, or ops.grow_labels of it)" % (name, F, H, W))


def _plate_on(name, first, tensors):
    dev = first.device
    for t, what in tensors:
        if not t.is_cuda or t.device != dev:
            raise RuntimeError("%s: %s must be a CUDA tensor on one device (%s), got %s: the plate has no host path" % (name, what, dev, t.device))
    return dev


def plate_update(plate, frames, block, n_max=64):
    """The background plate learns from frames: plate (int32 [Ho, Wo, 4], CUDA, cells (P_0, P_1, P_2, n), P in 24.8 fixed point; zeros
    when fresh) takes, frame by frame, ops.render_overlay's source value of frames ([F, 3, h0, w0] uint8 or float32, each frame
    contiguous, any stride >= 3*h0*w0 apart) at every pixel where block (uint8 [F, Ho, Wo]) is 0: n' = min(n + 1, n_max), P += floordiv(256 *
    s - P + (n' >> 1), n') -- the integer rule of include/mdqe_hip.h, mdqe_plate_update_u8.  n_max: an int in 1..256.  One launch on the
    current stream, in place.  -> plate."""
    name = "plate_update"
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    Ho, Wo = _plate_rgb(name, plate)
    if (not torch.is_tensor(frames) or frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4 or int(frames.shape[1]) != 3
            or frames.shape[2] < 1 or frames.shape[3] < 1):
        raise RuntimeError("%s: frames must be uint8 or float32 [F, 3, h0, w0]" % name)
    F, h0, w0 = int(frames.shape[0]), int(frames.shape[2]), int(frames.shape[3])
    stride = int(frames.stride(0)) if F > 1 else 3 * h0 * w0
    if tuple(frames.stride()[1:]) != (h0 * w0, w0, 1) or stride < 3 * h0 * w0 or h0 * Ho >= 2 ** 31 or w0 * Wo >= 2 ** 31:
        raise RuntimeError("%s: every frame must be contiguous and the frames a stride >= 3*h0*w0 apart, got strides %s"
                           % (name, tuple(frames.stride())))
    _plate_block(name, block, F, Ho, Wo)
    _plate_int(name, "n_max", n_max, 1, 256)
    if Ho * Wo * 4 >= 2 ** 31 - 1 or F * Ho * Wo >= 2 ** 31 - 1:
        raise RuntimeError("%s: Ho*Wo*4 and F*Ho*Wo must stay below 2^31 - 1, got %s" % (name, (F, Ho, Wo)))
    dev = _plate_on(name, plate, ((plate, "plate"), (frames, "frames"), (block, "block")))
    with torch.cuda.device(dev):
        check(lib.mdqe_plate_update_u8(ptr(frames), int(frames.dtype == torch.uint8), stride, h0, w0, ptr(block), F, Ho, Wo, n_max, ptr(plate),
                                       cur_stream(dev)), name)
    return plate


def plate_update_yuv(plate_y, plate_c, yuv, block, n_max=64):
    """`plate_update` on decoder surfaces: plate_y (int32 [H, W, 2], cells (P, n)) learns the luma samples where block (uint8 [F, H, W])
    is 0, plate_c (int32 [ceil(H/2), ceil(W/2), 4], cells (P_U, P_V, n, 0)) the chroma pairs whose whole 2 x 2 block (its in-picture
    pixels) is 0; a P010 sample's value is word >> 6: include/mdqe_hip.h, mdqe_plate_update_yuv420sp.  yuv: a preprocess.YuvFrames of F
    surfaces on the device.  One launch, in place.  -> (plate_y, plate_c)."""
    from .preprocess import YUV_FORMATS, YuvFrames, _pitch_stride
    name = "plate_update_yuv"
    if not isinstance(yuv, YuvFrames):
        raise RuntimeError("%s: yuv must be a preprocess.YuvFrames, got %s" % (name, type(yuv).__name__))
    F, H, W = len(yuv), yuv.height, yuv.width
    _plate_state(name, "plate_y", plate_y, (H, W, 2))
    _plate_state(name, "plate_c", plate_c, ((H + 1) // 2, (W + 1) // 2, 4))
    _plate_block(name, block, F, H, W)
    _plate_int(name, "n_max", n_max, 1, 256)
    if H * W * 4 >= 2 ** 31 - 1 or F * H * W >= 2 ** 31 - 1:
        raise RuntimeError("%s: H*W*4 and F*H*W must stay below 2^31 - 1, got %s" % (name, (F, H, W)))
    dev = _plate_on(name, plate_y, ((plate_y, "plate_y"), (plate_c, "plate_c"), (yuv.y, "yuv"), (yuv.uv, "yuv"), (block, "block")))
    (yp, ys), (cp, cs) = _pitch_stride(yuv.y), _pitch_stride(yuv.uv)
    with torch.cuda.device(dev):
        check(lib.mdqe_plate_update_yuv420sp(ptr(yuv.y), yp, ys, ptr(yuv.uv), cp, cs, F, H, W, YUV_FORMATS.index(yuv.fmt), ptr(block), n_max,
                                             ptr(plate_y), ptr(plate_c), cur_stream(dev)), name)
    return plate_y, plate_c


def plate_picture(plate, fill, reach=16, out=None):
    """The background plate's picture, the backdrop ops.render_replace takes: out (uint8 [Ho, Wo, 3], CUDA, contiguous; None:
    allocated) from plate (int32 [Ho, Wo, 4], `plate_update`'s state).  A seen pixel (n > 0) shows (P + 128) >> 8, a never-seen one the
    seen pixel with the smallest (d2, Y', X') within `reach` pixels (Euclidean; an int in 0..32), else `fill` (uint8 [3] on the device):
    the integer rule of include/mdqe_hip.h, mdqe_plate_picture_u8.  One launch on the current stream.  -> out."""
    name = "plate_picture"
    Ho, Wo = _plate_rgb(name, plate)
    if not torch.is_tensor(fill) or fill.dtype != torch.uint8 or tuple(fill.shape) != (3,) or not fill.is_contiguous():
        raise RuntimeError("%s: fill must be contiguous uint8 [3] in the frames' channel order (render.Style.plate_fill_on)" % name)
    _plate_int(name, "reach", reach, 0, 32)
    if Ho * Wo * 4 >= 2 ** 31 - 1:
        raise RuntimeError("%s: Ho*Wo*4 must stay below 2^31 - 1, got %s" % (name, (Ho, Wo)))
    if out is None:
        out = torch.empty((Ho, Wo, 3), dtype=torch.uint8, device=plate.device)
    if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (Ho, Wo, 3) or not out.is_contiguous():
        raise RuntimeError("%s: out must be contiguous uint8 %s" % (name, [Ho, Wo, 3]))
    dev = _plate_on(name, plate, ((plate, "plate"), (fill, "fill"), (out, "out")))
    with torch.cuda.device(dev):
        check(lib.mdqe_plate_picture_u8(ptr(plate), Ho, Wo, reach, ptr(fill), ptr(out), cur_stream(dev)), name)
    return out


def plate_picture_yuv(plate_y, plate_c, fill_yuv, out, reach=16):
    """`plate_picture` as one decoder surface, the backdrop ops.render_replace_yuv takes: out (a preprocess.YuvFrames of ONE surface on
    the device; its height, width and fmt say the planes' sizes and samples) from plate_y and plate_c (`plate_update_yuv`'s state).  The
    chroma plane is filled on its own grid with reach (reach + 1) // 2; fill_yuv: uint16 [3], (Y, U, V) in sample units
    (render.backdrop_yuv); P010 words are value << 6: include/mdqe_hip.h, mdqe_plate_picture_yuv420sp.  One launch.  -> out."""
    from .preprocess import YUV_FORMATS, YuvFrames, _pitch_stride
    name = "plate_picture_yuv"
    if not isinstance(out, YuvFrames) or len(out) != 1:
        raise RuntimeError("%s: out must be a preprocess.YuvFrames of ONE surface" % name)
    H, W = out.height, out.width
    _plate_state(name, "plate_y", plate_y, (H, W, 2))
    _plate_state(name, "plate_c", plate_c, ((H + 1) // 2, (W + 1) // 2, 4))
    if (not torch.is_tensor(fill_yuv) or fill_yuv.dtype not in (torch.uint16, torch.int16) or tuple(fill_yuv.shape) != (3,)
            or not fill_yuv.is_contiguous()):
        raise RuntimeError("%s: fill_yuv must be contiguous uint16 [3], (Y, U, V) in sample units (render.backdrop_yuv)" % name)
    _plate_int(name, "reach", reach, 0, 32)
    if H * W * 4 >= 2 ** 31 - 1:
        raise RuntimeError("%s: H*W*4 must stay below 2^31 - 1, got %s" % (name, (H, W)))
    dev = _plate_on(name, plate_y, ((plate_y, "plate_y"), (plate_c, "plate_c"), (fill_yuv, "fill_yuv"), (out.y, "out"), (out.uv, "out")))
    with torch.cuda.device(dev):
        check(lib.mdqe_plate_picture_yuv420sp(ptr(plate_y), ptr(plate_c), H, W, YUV_FORMATS.index(out.fmt), reach, ptr(fill_yuv),
                                              ptr(out.y), _pitch_stride(out.y)[0], ptr(out.uv), _pitch_stride(out.uv)[0], cur_stream(dev)), name)
    return out


def _trail_args(name, pts, n, palette, F, f_off, p_off, trail, width, table_dtypes):
    """The checks render_trails and render_trails_yuv share.  -> the point table's row stride."""
    # (shapes and dtypes first, devices after: what a host without a GPU can check is checked the same way there)
    if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= 255:
        raise RuntimeError("%s: n must be an int in 0..255, got %r" % (name, n))
    for what, v, lo, hi in (("trail", trail, 1, 64), ("width", width, 1, 5), ("F", F, 0, 2 ** 31 - 1), ("f_off", f_off, 0, 2 ** 31 - 1),
                            ("p_off", p_off, 0, 2 ** 31 - 1)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise RuntimeError("%s: %s must be an int in %d..%d, got %r" % (name, what, lo, hi, v))
    stride = _point_table(name, pts, n, p_off + F)
    if not torch.is_tensor(palette) or palette.dtype not in table_dtypes or tuple(palette.shape) != (256, 3) or not palette.is_contiguous():
        raise RuntimeError("%s: palette must be contiguous %s [256, 3]" % (name, str(table_dtypes[0]).replace("torch.", "")))
    return stride


def render_trails(pic, pts, n, palette, F, f_off=0, p_off=0, trail=16, width=2):
    """Motion trails drawn onto a painted picture, in place: pic (uint8 [>= f_off + F, Ho, Wo, 3], CUDA, contiguous) gets, in its frames
    f_off .. f_off + F - 1 and for each label l = 1..n, the line through the points of row l - 1 of pts (int32 [>= n, >= p_off + F, 2]:
    ops.label_centroids' table) in columns p_off + f - trail .. p_off + f, `width` pixels wide with round caps, in palette[l] (uint8
    [256, 3]).  A column below 0 and a point outside the picture are absent; the present points are joined in column order, gaps
    bridged; a lone point is a disc.  Lower labels lie over higher ones; a pixel that nothing hits is not written: the integer rule of
    include/mdqe_hip.h, mdqe_render_trails_u8.  trail in 1..64, width in 1..5.  One launch on the current stream, none when F == 0 or
    n == 0.  -> pic."""
    stride = _trail_args("render_trails", pts, n, palette, F, f_off, p_off, trail, width, (torch.uint8,))
    if not torch.is_tensor(pic) or pic.dtype != torch.uint8 or pic.dim() != 4 or int(pic.shape[3]) != 3 or not pic.is_contiguous():
        raise RuntimeError("render_trails: pic must be contiguous uint8 [frames, Ho, Wo, 3]")
    Ho, Wo = int(pic.shape[1]), int(pic.shape[2])
    if Ho < 1 or Wo < 1 or Ho > 16384 or Wo > 16384 or f_off + F > pic.shape[0] or F * Ho * Wo >= 2 ** 31 - 1:
        raise RuntimeError("render_trails: pic %s must hold frames f_off .. f_off + F = %d of a size in 1..16384, F*Ho*Wo < 2^31 - 1"
                           % (tuple(pic.shape), f_off + F))
    for t, what in ((pic, "pic"), (pts, "pts"), (palette, "palette")):
        if not t.is_cuda or t.device != pic.device:
            raise RuntimeError("render_trails: %s must be a CUDA tensor on pic's device, got %s" % (what, t.device))
    with torch.cuda.device(pic.device):
        check(lib.mdqe_render_trails_u8(ptr(pic), F, Ho, Wo, f_off, ptr(pts), stride, p_off, n, trail, width, ptr(palette),
                                        cur_stream(pic.device)), "render_trails")
    return pic


def render_trails_yuv(yuv, pts, n, palette_yuv, F, f_off=0, p_off=0, trail=16, width=2):
    """`render_trails` on painted decoder surfaces, in place: yuv (a preprocess.YuvFrames on a HIP device, NV12 or P010) gets the same
    lines in its surfaces f_off .. f_off + F - 1, with palette_yuv (uint16 [256, 3], rows (Y, U, V) in sample units:
    render.palette_yuv).  Luma follows the rule per sample; chroma is ops.annotate_yuv's rule: the integer rule of include/mdqe_hip.h,
    mdqe_render_trails_yuv420sp.  -> yuv."""
    from .preprocess import YUV_FORMATS, YuvFrames, _pitch_stride
    stride = _trail_args("render_trails_yuv", pts, n, palette_yuv, F, f_off, p_off, trail, width, (torch.uint16, torch.int16))
    if not isinstance(yuv, YuvFrames):
        raise RuntimeError("render_trails_yuv: yuv must be a preprocess.YuvFrames, got %s" % type(yuv).__name__)
    H, W = yuv.height, yuv.width
    if H > 16384 or W > 16384 or f_off + F > len(yuv) or F * H * W >= 2 ** 31 - 1:
        raise RuntimeError("render_trails_yuv: yuv holds %d surfaces of %d x %d, the call needs f_off + F = %d of a size up to 16384, "
                           "F*H*W < 2^31 - 1" % (len(yuv), H, W, f_off + F))
    if not yuv.is_cuda:
        raise RuntimeError("render_trails_yuv: the surfaces must be on a HIP device, got %s (the trail pass has no host path)" % (yuv.device,))
    for t, what in ((pts, "pts"), (palette_yuv, "palette_yuv")):
        if t.device != yuv.device:
            raise RuntimeError("render_trails_yuv: %s must be on the surfaces' device %s, got %s" % (what, yuv.device, t.device))
    (yp, ys), (cp, cs) = _pitch_stride(yuv.y), _pitch_stride(yuv.uv)
    with torch.cuda.device(yuv.device):
        check(lib.mdqe_render_trails_yuv420sp(ptr(yuv.y), yp, ys, ptr(yuv.uv), cp, cs, F, H, W, YUV_FORMATS.index(yuv.fmt), f_off, ptr(pts),
                                              stride, p_off, n, trail, width, ptr(palette_yuv), cur_stream(yuv.device)), "render_trails_yuv")
    return yuv


def _paint_yuv_host(labels, yuv, palette_yuv, out, f_off, a256, contour, action=None, cell=None, taps=None, within=False):
    """The surface painters' rule of include/mdqe_hip.h on host planes, in torch integers.  action None: the plain painter, which is the
    table [0, 1, 1, ...] (no label has action 2, so no cell mean is taken) and may paint in place.  taps = (taps, taps_c): the blur
    painter, whose special action is 3 and whose special value is the blurred plane's; every action but 1 and 3 then keeps.  within:
    the blur painter's edge-stopping rule (mdqe_render_blur_within_yuv420sp): luma is blurred among the pixels of action 3, U and V
    among the pairs whose block holds one.  -> out."""
    F, H, W = len(yuv), yuv.height, yuv.width
    p010 = yuv.fmt == "p010"
    ch, cw = (H + 1) // 2, (W + 1) // 2

    def raw(t):
        v = t.to(torch.int64)
        return v & 0xFFFF if p010 else v

    def store(dst, word):
        dst.copy_(((word + 0x8000) & 0xFFFF) - 0x8000 if p010 else word)

    def up(t):                                      # a chroma-plane quantity at every pixel of its block
        return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)[:, :H, :W]

    def means(v, sub):                              # cell means of a plane sub-sampled by `sub`; never looked at without an action 2
        if taps is not None:                        # (the blur: the plane's own taps; what px calls action 2 is action 3 here)
            if within:
                return _blur_plane_within(v, act == 2 if sub == 1 else blocks((act == 2).to(torch.int64)) > 0, taps[sub - 1])
            return _blur_plane(v, taps[sub - 1])
        return v if action is None else _cell_means(v, cell // sub)

    lab = labels.to(torch.int64)
    act = (lab != 0).to(torch.int64) if action is None else action.to(torch.int64)[lab]
    if taps is not None:
        act = torch.where(act == 3, 2, torch.where(act == 1, 1, 0))
    edge = torch.zeros(lab.shape, dtype=torch.bool)
    for d in range(1, contour + 1):
        if d < H:
            edge[:, d:] |= lab[:, d:] != lab[:, :-d]
            edge[:, :-d] |= lab[:, :-d] != lab[:, d:]
        if d < W:
            edge[:, :, d:] |= lab[:, :, d:] != lab[:, :, :-d]
            edge[:, :, :-d] |= lab[:, :, :-d] != lab[:, :, d:]
    col = (palette_yuv.view(torch.int16).to(torch.int64) & (0x3FF if p010 else 0xFF))[lab]          # [F, H, W, 3]
    keep_px = act == 0

    def px(s, p, mean):
        return torch.where(keep_px, s, torch.where(act == 2, mean, torch.where(edge, p, (s * (256 - a256) + p * a256 + 128) >> 8)))
    ry = raw(yuv.y[:, :H, :W])
    Y = ry >> 6 if p010 else ry
    yo = px(Y, col[..., 0], means(Y, 1))
    store(out.y[f_off:f_off + F, :H, :W], torch.where(keep_px, ry, yo << 6 if p010 else yo))
    rc = raw(yuv.uv[:, :ch, :2 * cw]).reshape(F, ch, cw, 2)
    C = rc >> 6 if p010 else rc

    def blocks(t):                                  # [F, H, W] -> the sum over each 2 x 2 block's in-picture pixels, [F, ch, cw]
        full = torch.zeros((F, 2 * ch, 2 * cw), dtype=torch.int64)
        full[:, :H, :W] = t
        return full.reshape(F, ch, 2, cw, 2).sum((2, 4))
    n = blocks(torch.ones((F, H, W), dtype=torch.int64))
    sh = n >> 1                                     # n = 1, 2, 4: n / 2 = log2(n) = 0, 1, 2
    keep = blocks((~keep_px).to(torch.int64)) == 0
    oc = torch.stack([(blocks(px(up(C[..., k]), col[..., k + 1], up(means(C[..., k], 2)))) + sh) >> sh for k in (0, 1)], -1)
    word = torch.where(keep[..., None], rc, oc << 6 if p010 else oc)
    store(out.uv[f_off:f_off + F, :ch, :2 * cw], word.reshape(F, ch, 2 * cw))
    return out


def layernorm_post(x, gamma, beta, post, eps=1e-5, out=None):
    """out = LN(x)*gamma + beta + post."""
    _chk(x, "x"); _chk(post, "post")
    C = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    check(lib.mdqe_layernorm_post_f32(ptr(x), ptr(gamma), ptr(beta), ptr(post), ptr(out), x.numel() // C, C, eps, cur_stream()),
          "layernorm_post")
    return out


def patch4_im2col(frames, Hp, Wp, mean, std):
    import ctypes
    NI, _, h, w = frames.shape
    out = torch.empty((NI * (Hp // 4) * (Wp // 4), 48), dtype=torch.float32, device=frames.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    check(lib.mdqe_patch4_im2col_f32(ptr(frames), int(frames.dtype == torch.uint8), 3 * h * w, NI, h, w, Hp, Wp, m, s, ptr(out),
                                     cur_stream()), "patch4_im2col")
    return out


def swin_window_gather(x, ws, shift):
    """x [B,H,W,C] -> window rows [B*nW*ws*ws, C] (zero pad + cyclic shift + partition)."""
    _chk(x, "x")
    B, H, W, C = x.shape
    Hp, Wp = (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws
    out = torch.empty((B * Hp * Wp, C), dtype=torch.float32, device=x.device)
    check(lib.mdqe_swin_window_f32(ptr(x), None, ptr(out), B, H, W, C, ws, shift, 0, cur_stream()), "swin_window_gather")
    return out


def swin_window_scatter_add(rows, shortcut, ws, shift, out=None):
    """out[b,y,x] = shortcut[b,y,x] + rows[window order] (reverse + un-shift + crop)."""
    _chk(rows, "rows"); _chk(shortcut, "shortcut")
    B, H, W, C = shortcut.shape
    if out is None:
        out = torch.empty_like(shortcut)
    check(lib.mdqe_swin_window_f32(ptr(rows), ptr(shortcut), ptr(out), B, H, W, C, ws, shift, 1, cur_stream()), "swin_window_scatter")
    return out


def linear_swin(x, weight, bias, ws, shift, out=None):
    """x [B,H,W,C] (contiguous NHWC) -> window_partition(roll(pad(x))) @ weight^T + bias as rows [B*Hp*Wp, N] in window order, without
    the partitioned copy (mdqe_gemm_nt_swin_f32; exact-fp32 GEMM mode only -- callers check get_gemm_precision())."""
    _chk(x, "x"); _chk(weight, "weight"); _chk(bias, "bias")
    B, H, W, C = x.shape
    N = weight.shape[0]
    Hp, Wp = (H + ws - 1) // ws * ws, (W + ws - 1) // ws * ws
    if out is None:
        out = torch.empty((B * Hp * Wp, N), dtype=torch.float32, device=x.device)
    check(lib.mdqe_gemm_nt_swin_f32(ptr(x), C, ptr(weight), ptr(bias), ptr(out), out.stride(0), B, H, W, ws, shift, N, C, cur_stream()),
          "gemm_nt_swin")
    return out


def layernorm_swin_scatter(rows, gamma, beta, shortcut, ws, shift, eps=1e-5, out=None):
    """out[b,y,x] = shortcut[b,y,x] + LN(rows[window-order row of (b,y,x)]) * gamma + beta; rows [B*Hp*Wp, C], shortcut [B,H,W,C].
    out=None writes over `shortcut` (every pixel is written by exactly one row)."""
    _chk(rows, "rows"); _chk(shortcut, "shortcut"); _chk(gamma, "gamma"); _chk(beta, "beta")
    B, H, W, C = shortcut.shape
    if out is None:
        out = shortcut
    check(lib.mdqe_layernorm_swin_scatter_f32(ptr(rows), ptr(gamma), ptr(beta), ptr(shortcut), ptr(out), B, H, W, C, ws, shift, eps,
                                              cur_stream()), "layernorm_swin_scatter")
    return out


def window_attn(qkv, n_windows, N, C, nh, scale, bias, mask=None, nW=1):
    _chk(qkv, "qkv"); _chk(scale, "scale"); _chk(bias, "bias"); _chk(mask, "mask")
    out = torch.empty((n_windows * N, C), dtype=torch.float32, device=qkv.device)
    check(lib.mdqe_window_attn_f32(ptr(qkv), qkv.stride(0), ptr(out), C, n_windows, N, C, nh, ptr(scale), ptr(bias), ptr(mask), nW,
                                   cur_stream()), "window_attn")
    return out


def patch_merge_gather(x):
    _chk(x, "x")
    B, H, W, C = x.shape
    out = torch.empty((B * ((H + 1) // 2) * ((W + 1) // 2), 4 * C), dtype=torch.float32, device=x.device)
    check(lib.mdqe_patch_merge_gather_f32(ptr(x), ptr(out), B, H, W, C, cur_stream()), "patch_merge_gather")
    return out


def image_mask_stats(logits, factor, h, w):
    """logits [n,Hm,Wm] -> [n,6] = (sum soft*hard, count hard, xmin, ymin, xmax, ymax of logit>0) over the x`factor` crop [:h,:w]."""
    _chk(logits, "logits")
    n, Hm, Wm = logits.shape
    out = torch.empty(n, 6, device=logits.device)
    check(lib.mdqe_image_mask_stats_f32(ptr(logits), n, Hm, Wm, factor, h, w, ptr(out), cur_stream()), "image_mask_stats")
    return out


def image_final_masks(logits, idx, factor, h, w, Ho, Wo):
    """logits [n,Hm,Wm], idx int32 CUDA [k] -> uint8 [k,Ho,Wo]: bilinear resize of the cropped up-sampled logits, > 0."""
    _chk(logits, "logits")
    n, Hm, Wm = logits.shape
    out = torch.empty(int(idx.numel()), Ho, Wo, dtype=torch.uint8, device=logits.device)
    check(lib.mdqe_image_final_masks_u8(ptr(logits), int(idx.numel()), ptr(idx), Hm, Wm, factor, h, w, Ho, Wo, ptr(out), cur_stream()),
          "image_final_masks")
    return out


def _geom_rows(geom, rows, device):
    if geom is None or geom is True:                      # (allocate)
        return torch.empty(rows, 5, dtype=torch.int32, device=device)
    _chk(geom, "geom", torch.int32)
    if tuple(geom.shape) != (rows, 5):
        raise RuntimeError("final_masks_geom: geom must be int32 [n_sel * Fw, 5]")
    return geom


def final_masks_rle(logits, inst_idx, factor, h, w, Ho, Wo, cap):
    """logits [n,Fw,Hm,Wm]; inst_idx int32 CUDA [n_sel] -> (pos int32 [n_sel*Fw, cap], n_pos int32 [n_sel*Fw]): column-major
    positions at which each final mask changes value (ops.final_masks never materialised)."""
    k, Fw, Hm, Wm, pos, n_pos = _final_mask_args(logits, inst_idx, False, cap)
    check(lib.mdqe_final_masks_rle(ptr(logits), k, ptr(inst_idx), Fw, Hm, Wm, factor, h, w, Ho, Wo, cap, ptr(pos), ptr(n_pos),
                                   cur_stream()), "final_masks_rle")
    return pos, n_pos


def final_masks_rle_geom(logits, inst_idx, factor, h, w, Ho, Wo, cap, geom=None):
    """ops.final_masks_rle plus the geom rows of ops.final_masks_geom from the same sweep -> (pos, n_pos, geom)."""
    k, Fw, Hm, Wm, pos, n_pos = _final_mask_args(logits, inst_idx, True, cap)
    geom = _geom_rows(geom, k * Fw, logits.device)
    check(lib.mdqe_final_masks_rle_geom(ptr(logits), k, ptr(inst_idx), Fw, Hm, Wm, factor, h, w, Ho, Wo, cap, ptr(pos), ptr(n_pos),
                                        ptr(geom), cur_stream()), "final_masks_rle_geom")
    return pos, n_pos, geom


# ---- per-clip stages (csrc/clip_ops.hip) -----------------------------------------------------------------------------
def clip_assoc(emb, fidx, ct, wdw, nb):
    """emb [frames, Q, E]; fidx [Bc, T] int32 CUDA -> idx [Bc, T, Q] int32 (inter-frame query association)."""
    _chk(emb, "emb"); _chk(fidx, "fidx", torch.int32)
    Bc, T = fidx.shape
    Q, E = emb.shape[1], emb.shape[2]
    idx = torch.empty(Bc, T, Q, dtype=torch.int32, device=emb.device)
    check(lib.mdqe_clip_assoc_f32(ptr(emb), Q, E, ptr(fidx), Bc, T, ct, float(wdw), nb, ptr(idx), cur_stream()), "clip_assoc")
    return idx


def clip_gather_init(content, coords, fidx, idx, ct):
    """-> x [Bc*T*Q, C], ref [Bc*T*Q, 4], x_inst [Bc*Q, C]."""
    _chk(content, "content"); _chk(coords, "coords"); _chk(fidx, "fidx", torch.int32); _chk(idx, "idx", torch.int32)
    Bc, T = fidx.shape
    Q, C = content.shape[1], content.shape[2]
    x = torch.empty(Bc * T * Q, C, device=content.device)
    ref = torch.empty(Bc * T * Q, 4, device=content.device)
    xi = torch.empty(Bc * Q, C, device=content.device)
    check(lib.mdqe_clip_gather_init_f32(ptr(content), ptr(coords), ptr(fidx), ptr(idx), Bc, T, Q, C, ct, ptr(x), ptr(ref), ptr(xi),
                                        cur_stream()), "clip_gather_init")
    return x, ref, xi


def box_refine(delta, prev, Bc, T, Q, t0, t1):
    """boxes = sigmoid(delta + inverse_sigmoid(prev)) [Bc*T*Q, 4]; clip boxes [Bc*Q, 4] over frames [t0, t1)."""
    _chk(delta, "delta"); _chk(prev, "prev")
    boxes = torch.empty(Bc * T * Q, 4, device=delta.device)
    ibox = torch.empty(Bc * Q, 4, device=delta.device)
    check(lib.mdqe_box_refine_f32(ptr(delta), ptr(prev), Bc, T, Q, t0, t1, ptr(boxes), ptr(ibox), cur_stream()), "box_refine")
    return boxes, ibox


def box_head_refine(h, w, b, prev, Bc, T, Q, t0, t1):
    """box_refine(h @ w^T + b, prev) with the 4-column product inside the kernel: h [Bc*T*Q, K] (K % 256 == 0), w [4, K], b [4]."""
    _chk(h, "h"); _chk(w, "w"); _chk(b, "b"); _chk(prev, "prev")
    boxes = torch.empty(Bc * T * Q, 4, device=h.device)
    ibox = torch.empty(Bc * Q, 4, device=h.device)
    check(lib.mdqe_box_head_refine_f32(ptr(h), h.stride(0), ptr(w), ptr(b), ptr(prev), Bc, T, Q, h.shape[1], t0, t1, ptr(boxes), ptr(ibox),
                                       cur_stream()), "box_head_refine")
    return boxes, ibox


def time_fuse_dot(xw, wt, bt, src, Bc, T, Q):
    """time_fuse(xw @ wt^T + bt, src): the time weights are computed inside the kernel.  xw, src [Bc*T*Q, 256], wt [1, 256], bt [1]."""
    _chk(xw, "xw"); _chk(wt, "wt"); _chk(bt, "bt"); _chk(src, "src")
    C = src.shape[-1]
    out = torch.empty(Bc * Q, C, device=src.device)
    check(lib.mdqe_time_fuse_dot_f32(ptr(xw), ptr(wt), ptr(bt), ptr(src), Bc, T, Q, C, ptr(out), cur_stream()), "time_fuse_dot")
    return out


def add_rows(a, b, out=None):
    """out = a + b for 2-D row-strided fp32 operands of the same shape."""
    rows, C = a.shape
    if out is None:
        out = torch.empty(rows, C, device=a.device)
    check(lib.mdqe_add_rows_f32(ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(out), out.stride(0), rows, C, cur_stream()), "add_rows")
    return out


def time_fuse(w, x, Bc, T, Q, pos=None):
    """out[b,q,:] = sum_t softmax_t(w[b,t,q]) x[b,t,q,:]  (-> (out, out + pos) when pos is given)."""
    _chk(w, "w"); _chk(x, "x"); _chk(pos, "pos")
    C = x.shape[-1]
    out = torch.empty(Bc * Q, C, device=x.device)
    out2 = torch.empty(Bc * Q, C, device=x.device) if pos is not None else None
    check(lib.mdqe_time_fuse_f32(ptr(w), ptr(x), Bc, T, Q, C, ptr(out), ptr(pos), ptr(out2), cur_stream()), "time_fuse")
    return (out, out2) if pos is not None else out


def clip_select(cls, emb, thr, max_keep):
    """cls [B,Q,K], emb [B,Q,C] -> kept [B,Q] int32 (query indices of the kept ranks, score order), n_keep [B] int32."""
    _chk(cls, "cls"); _chk(emb, "emb")
    B, Q, K = cls.shape
    C = emb.shape[-1]
    dev = cls.device
    order = torch.empty(B, Q, dtype=torch.int32, device=dev)
    n_thr = torch.empty(B, dtype=torch.int32, device=dev)
    inv = torch.empty(B, Q, device=dev)
    sim = torch.empty(B, Q, Q, device=dev)
    kept = torch.empty(B, Q, dtype=torch.int32, device=dev)
    n_keep = torch.empty(B, dtype=torch.int32, device=dev)
    check(lib.mdqe_clip_select_f32(ptr(cls), ptr(emb), B, Q, K, C, float(thr), int(max_keep), ptr(order), ptr(n_thr), ptr(inv), ptr(sim),
                                   ptr(kept), ptr(n_keep), cur_stream()), "clip_select")
    return kept, n_keep


def dyn_mask_nms(coef, kept, feats, row0, n, f0, T):
    """The fused dynamic-mask kernel + NMS for a batch of clips.  coef [B,Q,M]; kept [B,Q] int32; feats [frames,H,W,M];
    row0 / n / f0: host int32 numpy arrays [B].  -> logits [n_rows,T,H,W], stats [n_rows,5], mi [n_rows]."""
    import numpy as np
    _chk(coef, "coef"); _chk(kept, "kept", torch.int32); _chk(feats, "feats")
    B, Q, M = coef.shape
    H, W = feats.shape[1], feats.shape[2]
    n_rows = int(n.sum())
    dev = coef.device
    logits = torch.empty(n_rows, T, H, W, device=dev)
    stats = torch.empty(n_rows, 5, device=dev)
    mi = torch.empty(n_rows, device=dev)
    if n_rows == 0:
        return logits, stats, mi
    t_step = 2 if T >= 5 else 1
    Ph = ((T + t_step - 1) // t_step) * (H // 2) * (W // 2)
    soft_h = torch.empty(n_rows, Ph, device=dev)
    hard_h = torch.empty(n_rows, Ph, device=dev)
    gram = torch.empty(lib.mdqe_nms_workspace_floats(int(n.max())), device=dev)
    part = torch.empty(lib.mdqe_dyn_mask_workspace_floats(n_rows, T, H, W), device=dev)
    row0 = np.ascontiguousarray(row0, dtype=np.int32); n = np.ascontiguousarray(n, dtype=np.int32); f0 = np.ascontiguousarray(f0, dtype=np.int32)
    check(lib.mdqe_dyn_mask_nms_f32(ptr(coef), ptr(kept), ptr(feats), B, Q, M, T, H, W, row0.ctypes.data, n.ctypes.data, f0.ctypes.data,
                                    ptr(logits), ptr(soft_h), ptr(hard_h), ptr(part), ptr(gram), ptr(stats), ptr(mi), cur_stream()), "dyn_mask_nms")
    return logits, stats, mi


def clip_finalize(cls, emb, kept, stats, mi, thr, row0, n):
    """-> sel [n_rows] int32, n_sel [B] int32, out [n_rows, 2+K+C] (rows row0[b] .. row0[b]+n_sel[b] of clip b are valid)."""
    import numpy as np
    B, Q, K = cls.shape
    C = emb.shape[-1]
    n_rows = int(n.sum())
    dev = cls.device
    sel = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
    n_sel = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty(max(n_rows, 1), 2 + K + C, device=dev)
    row0 = np.ascontiguousarray(row0, dtype=np.int32); n = np.ascontiguousarray(n, dtype=np.int32)
    check(lib.mdqe_clip_finalize_f32(ptr(cls), ptr(emb), ptr(kept), ptr(stats), ptr(mi), B, Q, K, C, float(thr), row0.ctypes.data,
                                     n.ctypes.data, ptr(sel), ptr(n_sel), ptr(out), cur_stream()), "clip_finalize")
    return sel, n_sel, out


def rows_gather(src, idx, out=None):
    """out[i] = src[idx[i]] over the leading dim (idx int32 CUDA)."""
    _chk(src, "src"); _chk(idx, "idx", torch.int32)
    n = int(idx.numel())
    row_len = src.numel() // max(src.shape[0], 1)
    if out is None:
        out = torch.empty((n,) + tuple(src.shape[1:]), device=src.device)
    check(lib.mdqe_rows_gather_f32(ptr(src), ptr(idx), n, row_len, ptr(out), cur_stream()), "rows_gather")
    return out
