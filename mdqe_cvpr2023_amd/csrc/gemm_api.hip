// The front door of the GEMM kernels: the C entry points (include/mdqe_hip.h) check their arguments, fill one GemmParams and hand it
// to dispatch_gemm, which picks the tile and the kernel family -- K-step 16 fp32 (gemm_k16.hip) almost everywhere, K-step 32 fp32
// (gemm.hip), f16x3 (gemm_f16x3.hip), pre-split weights (gemm_f16x3w.hip).  Also here: the passes that are no MFMA kernel (split-K
// reduce, N <= 8 row dot products, the side term as a pass of its own) and the debug / precision switches.
#include "gemm_device.h"

// Second pass of a split-K product: sums the ksplit partial tiles in a fixed order and applies the epilogue.
__global__ void __launch_bounds__(256)
gemm_splitk_reduce_kernel(const GemmParams p) {
  const long total = (long)p.M * p.N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int m = (int)(i / p.N), n = (int)(i - (long)m * p.N);
    float x = 0.f;
    for (int s = 0; s < p.ksplit; ++s) x += p.ws[(long)s * total + i];       // fixed order: deterministic
    p.C[(long)m * p.ldc + n] = gemm_epilogue1<false>(p, x, m, n, p.res_mod > 0 ? m % p.res_mod : m, p.rowmask != nullptr && p.rowmask[m]);
  }
}

static int finish_splitk(const GemmParams& p, int rc, hipStream_t st) {
  if (rc || p.ksplit <= 1) return rc;
  long nb = ((long)p.M * p.N + 255) / 256; if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3((unsigned)nb), dim3(256), 0, st, p);
  return mdqe_launch_status();
}

static unsigned long long* g_gemm_stamps = nullptr;   // tools/ only: in-kernel phase stamps of the f16x3w kernel
extern "C" int mdqe_debug_gemm_stamps(void* buf) { g_gemm_stamps = (unsigned long long*)buf; return MDQE_OK; }

static int g_gemm_tile_rule = 0;      // tools/ A/B of the auto tile rule
extern "C" int mdqe_debug_gemm_tile_rule(int v) { g_gemm_tile_rule = v; return MDQE_OK; }
static int g_gemm_rows_dot = 1;       // tools/ A/B: 0 = N <= 8 products stay on the MFMA tiles
extern "C" int mdqe_debug_gemm_rows_dot(int v) { g_gemm_rows_dot = v; return MDQE_OK; }
static int g_gemm_variant = 2;         // fp32 kernel form: 0 = K-step 32 (gemm.hip), 1 = K-step 16 (gemm_k16.hip), 2 = by shape
extern "C" int mdqe_debug_gemm_variant(int v) { g_gemm_variant = v; return MDQE_OK; }

static int g_gemm_precision_all = 0;  // 0: exact fp32 MFMA; 1: f16x3 split on the 128-row tiles (gemm_f16x3.hip); 2: ONE f16 pass where the weight has planes -- process-wide
// The calling THREAD's override (-1 = none): a region of the model (the reference's autocast regions, engine.Engine.amp) switches
// the mode for its own launches without changing what another host thread -- the sharded schedule's tracker replay -- launches
// meanwhile.  Every reader below goes through the macro.
static thread_local int tl_gemm_precision = -1;
#define g_gemm_precision (tl_gemm_precision >= 0 ? tl_gemm_precision : g_gemm_precision_all)
extern "C" int mdqe_set_gemm_precision(int mode) {
  if (mode != 0 && mode != 1 && mode != 2) return MDQE_EINVAL;
  g_gemm_precision_all = mode;
  return MDQE_OK;
}
extern "C" int mdqe_set_gemm_precision_thread(int mode) {
  if (mode != -1 && mode != 0 && mode != 1 && mode != 2) return MDQE_EINVAL;
  tl_gemm_precision = mode;
  return MDQE_OK;
}
extern "C" int mdqe_get_gemm_precision(void) { return g_gemm_precision; }

// "This product can take the pre-split-weight kernels" (gemm_f16x3w.hip's requirements; p.vec_ok already set).
static bool planes_ok(const GemmParams& p) {
  return p.Wh != nullptr && p.K % 32 == 0 && p.N >= 128 && p.N % 4 == 0 && p.vec_ok && p.ksplit <= 1;
}

static int dispatch_gemm(GemmParams& p, int tile, hipStream_t st) {
  p.stamps = g_gemm_stamps;
  p.vec_ok = ((((uintptr_t)p.C | (uintptr_t)p.bias | (uintptr_t)p.residual) & 15) == 0) && (p.ldc % 4 == 0) &&
             (p.residual == nullptr || p.ldr % 4 == 0);
  // tile: 0 = auto.  Measured on the K-step-16 kernel (tools/tile_sweep*.py): the 128x128 tile only pays when the grid is
  // many times the 1024 resident blocks AND the tile has depth or width to amortise (N >= 1024 or K >= 1024); mid-size
  // problems -- the decoder's 21168-row GEMMs, res4/res5 3x3 convs -- run 15-30 % faster on 64x64 tiles (8 waves/SIMD).
  if (tile == 0) {
    const long b128 = (long)((p.M + 127) / 128) * ((p.N + 127) / 128);
    // f16x3w / f16w have their own tiling -- but only products the pre-split-weight kernels can take: an ineligible one (ragged K,
    // 64 < N < 128, unaligned C, split-K) keeps the fp32 heuristics' tile instead of a forced 128x128
    if (g_gemm_precision != 0 && planes_ok(p) && b128 >= 192) tile = 1;
    else if (p.N <= 64) tile = (p.M >= 4096) ? 2 : 3;
    else if ((g_gemm_tile_rule & 1) && b128 >= 2000 && p.N >= 1024 && p.N < 2048 && p.K <= 256 && !p.conv) tile = 9;   // short K, wide N -> 64x128
    else if ((g_gemm_tile_rule & 2) && p.conv && p.KH == 3 && b128 < 2000 && b128 >= 400 && p.N >= 256 && p.K < 4096) tile = 9;   // mid-grid 3x3 convs
    else if (b128 >= 2000 && (p.N >= 768 || p.K >= 1024)) tile = 1;        // (round 4: 768-wide products too -- Swin-L's K = 192 FFN1: 782 vs 794 us)
    else if (b128 >= 2000 && (p.N > 256 || p.K > 256)) tile = 2;
    else if (b128 >= 2000 && p.N >= 128 && !p.conv) tile = 2;               // (round 4, with the few-instruction epilogue: [153000,256]x[256,256] 167 vs 174 us,
    else tile = 3;                                                           //  Swin-L's [907200,192]x[192,192] 590 vs 616 us; before it 64x64 won: 288 vs 329 us)
  }
  if (tile == 1 && g_gemm_precision == 2 && planes_ok(p)) {
    // mode 2 ("f16"): ONE f16 MFMA pass on the round-to-nearest plane of a constant weight (the third plane of mdqe_f16x3_split_f32);
    // every product without planes, or too small / ragged for the 128-row tile, stays exact fp32 below (more accurate, never less)
    GemmParams q = p;
    q.Wh = (const char*)p.Wh + (long)p.N * p.K * 4;                      // planes: hi | lo | rn, N*K halves each
    const int n256 = (p.N + 255) / 256 * 256, n128 = (p.N + 127) / 128 * 128;
    const int bn = (n256 > n128 || (long)((p.M + 127) / 128) * (n256 / 256) < 400) ? 128 : 256;
    return mdqe_launch_gemm_f16w(q, bn, st);
  }
  if (tile == 1 && g_gemm_precision == 1 && planes_ok(p)) {
    // constant weights with pre-split planes: 128 x BN tile, BN by column waste, then by grid size
    const int n256 = (p.N + 255) / 256 * 256, n128 = (p.N + 127) / 128 * 128;
    int bn = 256;
    if (n256 > n128 || (long)((p.M + 127) / 128) * (n256 / 256) < 200) bn = 128;
    else {
      // the kernel is persistent, one block per CU: tiles are dealt in rounds of g_num_cus, and a 128-column tile costs ~0.55 of a
      // 256-column one (profiles/r04_f16x3w_one_site_ab.txt, columns "rule 8" / "rule 12") -- few-round grids take the narrow tile
      // when that saves a partial round (300 tiles: 2 rounds -> 3 half rounds, 93.6 -> 82.7 us)
      const long t256 = (long)((p.M + 127) / 128) * (n256 / 256), cus = 256;
      const long r256 = (t256 + cus - 1) / cus, r128 = (2 * t256 + cus - 1) / cus;
      if (r256 <= 4 && 0.55 * (double)r128 < 0.97 * (double)r256) bn = 128;
    }
    return mdqe_launch_gemm_f16x3w(p, bn, st);           // (planes_ok: never split-K)
  }
  if ((tile == 1 || tile == 2) && g_gemm_precision == 1) return finish_splitk(p, mdqe_launch_gemm_f16x3(p, tile, st), st);
  // K-step 16 (4+ blocks per CU) wins almost everywhere.  (Rounds 1-3: very deep-K convs on few rows kept the 32-wide step; with the
  // round-4 K loop and epilogue the K-step-16 kernel is ahead there too -- res5's 3x3 convs 419 against 460 us -- except on the one
  // narrow, few-row shape below: 139 against 146 us.)
  // (the window-order A map of mdqe_gemm_nt_swin_f32 exists in the K-step-16 kernel only: never the K-step-32 form, whatever the debug variant)
  if (p.swin_ws > 0 || g_gemm_variant == 1 || (g_gemm_variant == 2 && !(p.conv && p.K >= 2048 && p.K < 4096 && p.M <= 16384 && p.N <= 256)))
    return finish_splitk(p, mdqe_launch_gemm_k16(p, tile, st), st);
  return finish_splitk(p, mdqe_launch_gemm_k32(p, tile, st), st);
}

// ---- what the entry points share --------------------------------------------------------------------------------------------
// Bytes from the first to one past the last element of a [rows, cols] operand of pitch ld floats.
static long span_bytes(long rows, long ld, long cols) { return ((rows - 1) * ld + cols) * 4; }

static bool plain_dims_ok(int N, int K, long lda, long ldc) { return N > 0 && K > 0 && K % 4 == 0 && lda % 4 == 0 && lda >= K && ldc >= N; }

// The checks every product makes once its own dimensions are in order and it is not empty, then p = the plain product
// C[M, N] = A W^T + bias with no epilogue term and no split-K; the entry point adds what is particular to it.  ab = bytes of A
// that the kernel may address.  (Order matters to callers: a null operand is reported before a misaligned or oversized one.)
static int plain_params(GemmParams& p, const float* A, long lda, long ab, const float* W, const float* bias, float* C, long ldc,
                        long M, int N, long K) {
  MDQE_CHECK_PTR(A); MDQE_CHECK_PTR(W); MDQE_CHECK_PTR(C);
  MDQE_REQUIRE((((uintptr_t)A | (uintptr_t)W) & 15) == 0);
  const long wb = (long)N * K * 4;
  MDQE_REQUIRE(ab < 0xFFFFFFF0L && wb < 0xFFFFFFF0L && M < 0x7FFFFFFFL);      // (32-bit buffer ranges, int rows)
  p = {};
  p.A = A; p.W = W; p.C = C; p.M = (int)M; p.N = N; p.K = (int)K; p.lda = lda; p.ldc = ldc;
  p.bias = bias; p.act = MDQE_ACT_NONE; p.a_bytes = (unsigned)ab; p.w_bytes = (unsigned)wb;
  p.ksplit = 1; p.kchunk = (int)K;
  return MDQE_OK;
}

// Split-K over at most `ksplit` chunks of whole 32-float K-steps (conv: of whole taps x 32); partial tiles go to `ws`.
static int split_k(GemmParams& p, int ksplit, float* ws) {
  if (ksplit <= 1) return MDQE_OK;
  MDQE_CHECK_PTR(ws);
  int kc = (p.K + ksplit - 1) / ksplit; kc = (kc + 31) / 32 * 32;
  const int ks = (p.K + kc - 1) / kc;
  if (ks > 1) { p.ksplit = ks; p.kchunk = kc; p.ws = ws; }
  return MDQE_OK;
}

// Pre-split f16 planes of a constant weight (mdqe_f16x3_split_f32: hi | lo | rn, N*K halves each), or none.
static void use_planes(GemmParams& p, const void* w_split) {
  if (w_split != nullptr) { p.Wh = w_split; p.Wl = (const char*)w_split + (long)p.N * p.K * 2; }
}

// qkv = window_partition(roll(pad(x))) W^T + bias without the partitioned copy: the Swin block's first product reads its A rows straight
// from the NHWC map through the window order (SwinTransformerBlock.forward, swin_transformer_v2.py:236-262 -> WindowAttention.forward
// :153-155).  X [B, H, Wd, lda >= K]; C [B * Hp * Wp, ldc] in window order (Hp, Wp: H, Wd rounded up to multiples of ws).  Exact fp32
// MFMA only (the split-precision kernels do not know the row map: MDQE_EINVAL in that mode; the host then partitions first).
extern "C" int mdqe_gemm_nt_swin_f32(const float* X, long lda, const float* W, const float* bias, float* C, long ldc, int B, int H, int Wd,
                                     int ws, int shift, int N, int K, void* stream) {
  MDQE_REQUIRE(B >= 0 && H > 0 && Wd > 0 && ws > 0 && shift >= 0 && shift < ws && plain_dims_ok(N, K, lda, ldc));
  if (g_gemm_precision != 0) return MDQE_EINVAL;
  const int Hp = (H + ws - 1) / ws * ws, Wp = (Wd + ws - 1) / ws * ws;
  const long Ml = (long)B * Hp * Wp;
  if (Ml == 0) return MDQE_OK;
  MDQE_REQUIRE(Ml < 0x7FFFFFFFL);
  GemmParams p;
  const int rc = plain_params(p, X, lda, span_bytes((long)B * H * Wd, lda, K), W, bias, C, ldc, Ml, N, K);
  if (rc != MDQE_OK) return rc;
  p.swin_ws = ws; p.swin_shift = shift; p.swin_H = H; p.swin_W = Wd;
  mdqe_clear_error();
  return dispatch_gemm(p, 0, (hipStream_t)stream);
}

// The part mdqe_gemm_ln_f32 and mdqe_gemm_ln2_f32 share (M > 0, dimensions checked).
static int ln_params(GemmParams& p, const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N, int K,
                     const float* residual, long ldr, const float* gamma, const float* beta, float eps) {
  MDQE_CHECK_PTR(gamma); MDQE_CHECK_PTR(beta);
  const int rc = plain_params(p, A, lda, span_bytes(M, lda, K), W, bias, C, ldc, M, N, K);
  if (rc != MDQE_OK) return rc;
  MDQE_REQUIRE((((uintptr_t)C | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)gamma | (uintptr_t)beta) & 15) == 0);
  MDQE_REQUIRE(residual == nullptr || (ldr >= N && ldr % 4 == 0));
  // (the epilogue addresses C and the residual through 32-bit buffer offsets)
  MDQE_REQUIRE((long)M * ldc * 4 < 0xFFFF0000L && (residual == nullptr || (long)M * ldr * 4 < 0xFFFF0000L));
  p.residual = residual; p.ldr = ldr; p.vec_ok = 1;
  p.ln_g = gamma; p.ln_b = beta; p.ln_eps = eps;
  return MDQE_OK;
}

// C = LayerNorm(A W^T + bias + residual) * gamma + beta over N == 256 columns, ONE kernel (64x256 tile: the block owns whole
// rows, statistics in the epilogue).  Always exact fp32 MFMA.  C may alias the residual.
extern "C" int mdqe_gemm_ln_f32(const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N,
                                int K, const float* residual, long ldr, const float* gamma, const float* beta, float eps,
                                void* stream) {
  MDQE_REQUIRE(M >= 0 && N == 256 && plain_dims_ok(N, K, lda, ldc) && ldc % 4 == 0);
  if (M == 0) return MDQE_OK;
  GemmParams p;
  const int rc = ln_params(p, A, lda, W, bias, C, ldc, M, N, K, residual, ldr, gamma, beta, eps);
  if (rc != MDQE_OK) return rc;
  mdqe_clear_error();
  return mdqe_launch_gemm_k16(p, 6, (hipStream_t)stream);
}

// ... with a SECOND LayerNorm of the result in the same epilogue: C = LN(A W^T + bias + residual) * gamma + beta and
// C2 = LN(C) * gamma2 + beta2 -- the decoder's `x = norm3(x + ffn(x))` followed by the shared `decoder_norm(x)` that feeds the box head
// (transformer_dec.py:352-358,492-495).  C2 equals mdqe_layernorm_f32 applied to C bit for bit (same reduction tree).
extern "C" int mdqe_gemm_ln2_f32(const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N,
                                 int K, const float* residual, long ldr, const float* gamma, const float* beta, const float* gamma2,
                                 const float* beta2, float* C2, long ldc2, float eps, void* stream) {
  MDQE_REQUIRE(M >= 0 && N == 256 && plain_dims_ok(N, K, lda, ldc) && ldc % 4 == 0 && ldc2 >= N && ldc2 % 4 == 0);
  if (M == 0) return MDQE_OK;
  MDQE_CHECK_PTR(gamma2); MDQE_CHECK_PTR(beta2); MDQE_CHECK_PTR(C2);
  GemmParams p;
  const int rc = ln_params(p, A, lda, W, bias, C, ldc, M, N, K, residual, ldr, gamma, beta, eps);
  if (rc != MDQE_OK) return rc;
  MDQE_REQUIRE((((uintptr_t)gamma2 | (uintptr_t)beta2 | (uintptr_t)C2) & 15) == 0);
  MDQE_REQUIRE((long)M * ldc2 * 4 < 0xFFFF0000L);
  p.ln2_g = gamma2; p.ln2_b = beta2; p.C2 = C2; p.ldc2 = ldc2;
  mdqe_clear_error();
  return mdqe_launch_gemm_k16(p, 6, (hipStream_t)stream);
}

// ---- N <= 8 output columns (the decoder's box head 256 -> 4 and time weights 256 -> 1, on 31 360 rows a pass): a 128x64 MFMA tile
// computes 64 columns to keep 4, and the launch is bound by reading A anyway.  Here a wave takes 4 rows at a time, a lane 4
// consecutive k of each (one coalesced 1-KB read per row and 256 k), the N weight rows come from L1, and the partial dot products
// are summed across the wave with xor-shuffles.  fp32 FMA arithmetic; the summation order differs from the MFMA kernel's
// (the same rows always take the same path: N and K decide, not M).
template <int NN>
__global__ void __launch_bounds__(256)
rows_dot_kernel(const float* __restrict__ A, long lda, const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ C,
                long ldc, int M, int K, int act, int act_cols) {
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long)gridDim.x * 4;
  for (long r0 = wave * 4; r0 < M; r0 += nwaves * 4) {
    float acc[4][NN];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int n = 0; n < NN; ++n) acc[r][n] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 256) {
      f32x4 a[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = r0 + r < M ? r0 + r : M - 1;
        a[r] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(A + row * lda + k0 + lane * 4));
      }
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(W + (long)n * K + k0 + lane * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          acc[r][n] = fmaf(a[r][3], w[3], fmaf(a[r][2], w[2], fmaf(a[r][1], w[1], fmaf(a[r][0], w[0], acc[r][n]))));
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        float v = acc[r][n];
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) v += __shfl_xor(v, sft, 64);
        acc[r][n] = v;
      }
    if (lane < 4 && r0 + lane < M) {               // lane r writes row r0 + r
#pragma unroll
      for (int n = 0; n < NN; ++n) {
        float v = lane == 0 ? acc[0][n] : lane == 1 ? acc[1][n] : lane == 2 ? acc[2][n] : acc[3][n];
        if (bias != nullptr) v += bias[n];
        if (act != MDQE_ACT_NONE && (act_cols <= 0 || n < act_cols)) v = mdqe_act(v, act);
        C[(r0 + lane) * ldc + n] = v;
      }
    }
  }
}

extern "C" int mdqe_gemm_nt_f32(const float* A, long lda, const float* W, const float* bias, float* C, long ldc,
                                int M, int N, int K, int act, int act_cols, const float* residual, long ldr, int res_mod,
                                int res_first, const unsigned char* rowmask, int mask_cols, int tile, int ksplit,
                                float* splitk_ws, const void* w_split, void* stream) {
  MDQE_REQUIRE(M >= 0 && plain_dims_ok(N, K, lda, ldc));
  if (M == 0) return MDQE_OK;
  GemmParams p;
  int rc = plain_params(p, A, lda, span_bytes(M, lda, K), W, bias, C, ldc, M, N, K);
  if (rc != MDQE_OK) return rc;
  p.residual = residual; p.ldr = ldr; p.res_mod = res_mod; p.res_first = res_first; p.rowmask = rowmask; p.mask_cols = mask_cols;
  p.act = act; p.act_cols = act_cols;
  use_planes(p, w_split);
  if ((rc = split_k(p, ksplit, splitk_ws)) != MDQE_OK) return rc;
  mdqe_clear_error();
  if (N <= 8 && K % 256 == 0 && tile == 0 && p.ksplit <= 1 && residual == nullptr && rowmask == nullptr && g_gemm_rows_dot) {
    const long waves = ((long)M + 3) / 4;
    long nb = (waves + 3) / 4;
    if (nb > 256L * 8) nb = 256L * 8;
    hipStream_t st = (hipStream_t)stream;
#define ROWS_DOT(NN) hipLaunchKernelGGL((rows_dot_kernel<NN>), dim3((unsigned)nb), dim3(256), 0, st, A, lda, W, bias, C, ldc, M, K, act, act_cols)
    switch (N) {
      case 1: ROWS_DOT(1); break; case 2: ROWS_DOT(2); break; case 3: ROWS_DOT(3); break; case 4: ROWS_DOT(4); break;
      case 5: ROWS_DOT(5); break; case 6: ROWS_DOT(6); break; case 7: ROWS_DOT(7); break; default: ROWS_DOT(8); break;
    }
#undef ROWS_DOT
    return mdqe_launch_status();
  }
  return dispatch_gemm(p, tile, (hipStream_t)stream);
}

// C[m, n < side_cols] += side[m, 0:4] . side_w[n, 0:4] as a pass of its own: what the GEMM kernels without the in-epilogue
// side term (split-precision tiles, the K-step-32 form) are followed by.
__global__ void __launch_bounds__(256)
side_add_kernel(const float* __restrict__ side, const float* __restrict__ side_w, float* __restrict__ C, long ldc, long M, int cols) {
  const int c4n = cols / 4;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < M * c4n; i += (long)gridDim.x * blockDim.x) {
    const long m = i / c4n; const int n = (int)(i % c4n) * 4;
    const f32x4 s4 = *reinterpret_cast<const f32x4*>(side + m * 4);
    f32x4 v = *reinterpret_cast<const f32x4*>(C + m * ldc + n);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(side_w + (long)(n + e) * 4);
      v[e] += (s4[0] * w4[0] + s4[1] * w4[1]) + (s4[2] * w4[2] + s4[3] * w4[3]);
    }
    *reinterpret_cast<f32x4*>(C + m * ldc + n) = v;
  }
}

// C = A W^T + bias, and C[:, n < side_cols] += side [M, 4] x side_w[n, 0:4]^T -- a projection of `x + pos` where pos is itself a
// linear function of four numbers per row (the decoder's query position embedding, point2pos_proj(box centre),
// mdqe/models/transformer_dec.py:469,480,495,503 feeding :348-353, :397-402 and the sampling-offset / attention-weight projections
// of ms_deform_attn.py): `(x + pos) W^T = x W^T + box (W P)^T + W b_P`, with `W P` [N, 4] and the bias folded on the host once.
// One launch instead of add + GEMM, the [M, C] position tensor is never written; several projections of the same x with and
// without the position (q, k | v) become ONE product with side_cols marking the columns that take it.
extern "C" int mdqe_gemm_nt_side_f32(const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N, int K,
                                     const float* side, const float* side_w, int side_cols, const void* w_split, void* stream) {
  MDQE_REQUIRE(M >= 0 && plain_dims_ok(N, K, lda, ldc) && ldc % 4 == 0);
  MDQE_REQUIRE(side_cols >= 0 && side_cols <= N && side_cols % 4 == 0 && N % 4 == 0);
  if (M == 0) return MDQE_OK;
  if (side_cols > 0) { MDQE_CHECK_PTR(side); MDQE_CHECK_PTR(side_w); }
  GemmParams p;
  int rc = plain_params(p, A, lda, span_bytes(M, lda, K), W, bias, C, ldc, M, N, K);
  if (rc != MDQE_OK) return rc;
  MDQE_REQUIRE((((uintptr_t)C | (uintptr_t)bias | (uintptr_t)side | (uintptr_t)side_w) & 15) == 0);
  use_planes(p, w_split);
  mdqe_clear_error();
  hipStream_t st = (hipStream_t)stream;
  const bool in_epilogue = side_cols > 0 && g_gemm_precision == 0 && g_gemm_variant != 0;      // the K-step-16 fp32 kernel takes it itself
  if (in_epilogue) { p.side = side; p.side_w = side_w; p.side_cols = side_cols; }
  rc = dispatch_gemm(p, 0, st);
  if (rc != MDQE_OK || in_epilogue || side_cols == 0) return rc;
  long nb = ((long)M * (side_cols / 4) + 255) / 256; if (nb > 256L * 16) nb = 256L * 16;
  hipLaunchKernelGGL(side_add_kernel, dim3((unsigned)nb), dim3(256), 0, st, side, side_w, C, ldc, (long)M, side_cols);
  return mdqe_launch_status();
}

// Cat mode (the K-step-16 kernel with a second, pixel-addressed A operand): C = act([A1 | A2'] W^T + bias) for output rows
// m = (img, oh, ow), A1 [M, K1] rows and A2' the pixel (oh*stride, ow*stride) of the NHWC tensor A2 [NI, H2, W2, lda2 >= K2].
// K1 = 0: no first operand (A1 = A2).  The callers have checked the dimensions.
static int cat_product(const float* A1, long lda1, int K1, const float* A2, long lda2, int K2, int NI, int OH, int OW, int H2, int W2,
                       int stride, const float* W, const float* bias, float* C, long ldc, int N, int act, void* stream) {
  MDQE_REQUIRE((long)(OH - 1) * stride < H2 && (long)(OW - 1) * stride < W2);
  const long Ml = (long)NI * OH * OW;
  MDQE_REQUIRE(Ml < 0x7FFFFFFFL);
  if (Ml == 0) return MDQE_OK;
  MDQE_CHECK_PTR(A2);
  const long a2b = span_bytes((long)NI * H2 * W2, lda2, K2);
  GemmParams p;
  const int rc = plain_params(p, A1, lda1, K1 > 0 ? span_bytes(Ml, lda1, K1) : a2b, W, bias, C, ldc, Ml, N, K1 + K2);
  if (rc != MDQE_OK) return rc;
  MDQE_REQUIRE(((uintptr_t)A2 & 15) == 0 && a2b < 0xFFFFFFF0L);
  p.A2 = A2; p.lda2 = lda2; p.K1 = K1; p.a2_bytes = (unsigned)a2b; p.OH = OH; p.OW = OW; p.H = H2; p.Wd = W2; p.stride = stride;
  p.act = act; p.stamps = g_gemm_stamps;
  p.vec_ok = ((((uintptr_t)p.C | (uintptr_t)p.bias) & 15) == 0) && (p.ldc % 4 == 0);
  // The tile rule is an OLDER SNAPSHOT of dispatch_gemm's fp32 rule (N >= 1024 where that one now has N >= 768, and without its
  // `N >= 128 && !conv` -> tile 2 arm), kept as it is because the cat products were tuned on it: unifying the two is a tuning change.
  const long b128 = (long)((p.M + 127) / 128) * ((p.N + 127) / 128);
  int tile = 3;
  if (p.N <= 64) tile = (p.M >= 4096) ? 2 : 3;
  else if (b128 >= 2000 && (p.N >= 1024 || p.K >= 1024)) tile = 1;
  else if (b128 >= 2000 && (p.N > 256 || p.K > 256)) tile = 2;
  mdqe_clear_error();
  return mdqe_launch_gemm_k16(p, tile, (hipStream_t)stream);
}

// C = act([A1 | A2'] W^T + bias): the last 1x1 conv of a ResNet bottleneck and its projection shortcut as ONE product -- W = [W3 | Ws]
// along K, bias = b3 + bs -- so the shortcut's output (as wide as the block's output) is never written and read back.  A1: [M, K1]
// rows (pitch lda1); A2: the block's input, NHWC [NI, H2, W2, lda2 >= K2], read at pixel (oh*stride, ow*stride) for output row
// m = (img, oh, ow) (the shortcut's stride).  Exact fp32 MFMA only (the split-precision mode keeps the two-launch form).
extern "C" int mdqe_gemm_nt_cat2_f32(const float* A1, long lda1, int K1, const float* A2, long lda2, int K2, int NI, int OH, int OW,
                                     int H2, int W2, int stride, const float* W, const float* bias, float* C, long ldc, int N, int act,
                                     void* stream) {
  MDQE_REQUIRE(NI >= 0 && OH > 0 && OW > 0 && H2 > 0 && W2 > 0 && stride > 0 && N > 0 && K1 > 0 && K2 > 0);
  MDQE_REQUIRE(K1 % 16 == 0 && K2 % 16 == 0 && lda1 % 4 == 0 && lda2 % 4 == 0 && lda1 >= K1 && lda2 >= K2 && ldc >= N);
  return cat_product(A1, lda1, K1, A2, lda2, K2, NI, OH, OW, H2, W2, stride, W, bias, C, ldc, N, act, stream);
}

// The cat kernel with an empty first operand (K1 = 0): every K-step reads the row (img, oh*stride, ow*stride) of A.
extern "C" int mdqe_gemm_nt_pix_f32(const float* A, long lda, int K, int NI, int H, int Wd, int OH, int OW, int stride,
                                    const float* W, const float* bias, float* C, long ldc, int N, int act, void* stream) {
  MDQE_REQUIRE(NI >= 0 && H > 0 && Wd > 0 && OH > 0 && OW > 0 && stride > 0 && N > 0 && K > 0);
  MDQE_REQUIRE(K % 16 == 0 && lda % 4 == 0 && lda >= K && ldc >= N);
  return cat_product(A, lda, 0, A, lda, K, NI, OH, OW, H, Wd, stride, W, bias, C, ldc, N, act, stream);
}

extern "C" int mdqe_conv2d_nhwc_f32(const float* X, long x_img_stride, const float* Wt, const float* bias, float* Y, long ldy,
                                    int NI, int H, int Wd, int Cin, int Cout, int KH, int KW, int stride, int pad,
                                    int act, const float* residual, long ldr, int res_first, int tile, const void* w_split,
                                    int ksplit, float* splitk_ws, void* stream) {
  MDQE_REQUIRE(NI >= 0 && H > 0 && Wd > 0 && Cin > 0 && Cout > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0);
  MDQE_REQUIRE(Cin % 32 == 0);
  const int OH = (H + 2 * pad - KH) / stride + 1, OW = (Wd + 2 * pad - KW) / stride + 1;
  MDQE_REQUIRE(OH > 0 && OW > 0 && ldy >= Cout);
  if (NI == 0) return MDQE_OK;
  const long img = (long)H * Wd * Cin, pitch = x_img_stride <= 0 ? img : x_img_stride;
  GemmParams p;
  int rc = plain_params(p, X, 0, ((long)(NI - 1) * pitch + img) * 4, Wt, bias, Y, ldy, (long)NI * OH * OW, Cout, (long)KH * KW * Cin);
  if (rc != MDQE_OK) return rc;
  MDQE_REQUIRE(pitch % 4 == 0 && pitch >= img);
  p.conv = 1; p.H = H; p.Wd = Wd; p.Cin = Cin; p.OH = OH; p.OW = OW; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
  p.img_stride = pitch;
  p.residual = residual; p.ldr = ldr; p.res_first = res_first; p.act = act;
  if ((rc = split_k(p, ksplit, splitk_ws)) != MDQE_OK) return rc;     // deep-K conv on few output pixels: spread K over the CUs
  if (p.ksplit <= 1) use_planes(p, w_split);
  mdqe_clear_error();
  return dispatch_gemm(p, tile, (hipStream_t)stream);
}
