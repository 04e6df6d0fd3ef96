// Device pieces shared by the GEMM kernels (gemm.hip, gemm_k16.hip, gemm_f16x3.hip, gemm_f16x3w.hip) and the split-K reduce pass
// (gemm_api.hip): every rule below is written down here once.  All __forceinline__: after inlining a kernel sees the code it
// would have had written out by hand -- uniform conditions stay branches (gemm_k16.hip's header says why that matters).
#pragma once
#include "common.h"
#include "gemm_params.h"

// XCD-aware tile order: the hardware deals consecutive block ids round-robin over the 8 XCDs, so block `bid` takes the tile that
// makes every XCD own one contiguous range of the `ntiles` tiles -- blocks that share an A row-panel share an L2.
__device__ __forceinline__ int gemm_xcd_tile(int bid, int ntiles) {
  const int q = ntiles / 8, r = ntiles % 8, xcd = bid % 8, i = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
}

// Output row m = (img, oh, ow) on the OH x OW grid (conv and cat mode).
__device__ __forceinline__ void gemm_row_pixel(const GemmParams& p, int m, int& img, int& oh, int& ow) {
  ow = m % p.OW; const int t = m / p.OW; oh = t % p.OH; img = t / p.OH;
}
// Conv mode: row m's top-left input pixel (ih0, iw0) and its byte offset in the NHWC input.  A padded pixel's offset is
// "negative" and wraps: it is only ever used with a filter tap added that brings it back into the image (gemm_tap_addr).
__device__ __forceinline__ unsigned gemm_conv_row(const GemmParams& p, int m, int& ih0, int& iw0) {
  int img, oh, ow;
  gemm_row_pixel(p, m, img, oh, ow);
  ih0 = oh * p.stride - p.pad; iw0 = ow * p.stride - p.pad;
  return (unsigned)(((long)img * p.img_stride + ((long)ih0 * p.Wd + iw0) * p.Cin) * 4);
}

// Conv mode: the filter-tap cursor (t_kh, t_kw, channel t_c) of a K position; a K-step of bk floats lies inside one tap
// (Cin % bk == 0, host-checked).
__device__ __forceinline__ void gemm_tap_seek(const GemmParams& p, int k, int& t_kh, int& t_kw, int& t_c) {
  const int tap = k / p.Cin; t_c = k - tap * p.Cin; t_kh = tap / p.KW; t_kw = tap - t_kh * p.KW;
}
__device__ __forceinline__ void gemm_tap_advance(const GemmParams& p, int bk, int& t_kh, int& t_kw, int& t_c) {
  t_c += bk; if (t_c >= p.Cin) { t_c = 0; if (++t_kw == p.KW) { t_kw = 0; ++t_kh; } }
}
__device__ __forceinline__ int gemm_tap_bytes(const GemmParams& p, int t_kh, int t_kw, int t_c) {
  return ((t_kh * p.Wd + t_kw) * p.Cin + t_c) * 4;
}
// ... and the address of that tap for a row whose gemm_conv_row offset is `row_off`: zero padding is an out-of-range offset
// (the buffer bounds check returns 0).
__device__ __forceinline__ unsigned gemm_tap_addr(const GemmParams& p, int ih, int iw, unsigned row_off, int tap_bytes) {
  const bool ok = (ih >= 0) && (ih < p.H) && (iw >= 0) && (iw < p.Wd);
  return ok ? row_off + (unsigned)tap_bytes : OOB_OFF;
}

// Accumulator register r of a 32x32 MFMA (f32 32x32x2, f16 32x32x16) holds row gemm_acc_row(r, lane >> 5), column lane & 31
// of the sub-tile.
__device__ __forceinline__ constexpr int gemm_acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// ---- the epilogue's element formula: bias, rank-4 side term, residual before or after the activation, activation on the columns
// below act_cols, zeroing of masked rows.  `rrow` is the residual's row (m, or m % res_mod), `masked` is rowmask[m].  SIDE = false
// where the kernel never sees a side term (everything but the K-step-16 kernel): no test of p.side is compiled in.
template <bool SIDE>
__device__ __forceinline__ f32x4 gemm_epilogue4(const GemmParams& p, f32x4 v, int m, int n, long rrow, bool masked) {
  if (p.bias != nullptr) v += *reinterpret_cast<const f32x4*>(p.bias + n);
  if constexpr (SIDE) {
    if (p.side != nullptr && n < p.side_cols) {        // (side_cols % 4 == 0)
      const f32x4 s4 = *reinterpret_cast<const f32x4*>(p.side + (long)m * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(p.side_w + (long)(n + e) * 4);
        v[e] += (s4[0] * w4[0] + s4[1] * w4[1]) + (s4[2] * w4[2] + s4[3] * w4[3]);
      }
    }
  }
  f32x4 rv = {0.f, 0.f, 0.f, 0.f};
  if (p.residual != nullptr) rv = *reinterpret_cast<const f32x4*>(p.residual + rrow * p.ldr + n);
  if (p.res_first) v += rv;
  mdqe_act4(v, p.act, [&](int e) { return p.act_cols <= 0 || n + e < p.act_cols; });
  if (!p.res_first) v += rv;
  if (masked) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (n + e < p.mask_cols) v[e] = 0.f;
  }
  return v;
}

// ... one element (ragged edges, unaligned operands, the split-K reduce pass)
template <bool SIDE>
__device__ __forceinline__ float gemm_epilogue1(const GemmParams& p, float x, int m, int n, long rrow, bool masked) {
  x += p.bias != nullptr ? p.bias[n] : 0.f;
  if constexpr (SIDE) {
    if (p.side != nullptr && n < p.side_cols) {
      const float* s4 = p.side + (long)m * 4; const float* w4 = p.side_w + (long)n * 4;
      x += (s4[0] * w4[0] + s4[1] * w4[1]) + (s4[2] * w4[2] + s4[3] * w4[3]);
    }
  }
  const float rv = p.residual != nullptr ? p.residual[rrow * p.ldr + n] : 0.f;
  if (p.res_first) x += rv;
  if (p.act != MDQE_ACT_NONE && (p.act_cols <= 0 || n < p.act_cols)) x = mdqe_act(x, p.act);
  if (!p.res_first) x += rv;
  if (masked && n < p.mask_cols) x = 0.f;
  return x;
}

// A finished BM x BN fp32 tile, restaged in LDS as sC[BM][BN], to global memory by NTHR threads: every lane owns 4 consecutive
// columns of a row (bias / residual / C move as 16-B lane accesses, whole lines per row).  Split-K blocks write the raw partial
// tile to the workspace instead; the epilogue then runs in the reduce pass.  UNROLL: of the float4 loop (the body is long; see
// gemm_k16.hip's epilogue on instruction fetch).
template <int BM, int BN, int NTHR, int UNROLL>
__device__ __forceinline__ void gemm_tile_out(const GemmParams& p, const float* sC, int m0, int n0, int tid) {
  constexpr int C4 = BN / 4;                         // float4 per tile row
  constexpr int NV = BM * C4 / NTHR;                 // float4 per thread
  if (p.ksplit > 1) {
    float* w = p.ws + (long)blockIdx.y * p.M * p.N;
    for (int it = 0; it < NV; ++it) {
      const int idx = it * NTHR + tid;
      const int row = idx / C4, c4 = idx - row * C4;
      const int m = m0 + row, n = n0 + c4 * 4;
      if (m >= p.M) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (n + e < p.N) w[(long)m * p.N + n + e] = sC[row * BN + c4 * 4 + e];
    }
    return;
  }
  const bool vec = p.vec_ok;
  int rr0 = 0;
  if (p.residual != nullptr && p.res_mod > 0) rr0 = m0 % p.res_mod;
#pragma unroll UNROLL
  for (int it = 0; it < NV; ++it) {
    const int idx = it * NTHR + tid;
    const int row = idx / C4, c4 = idx - row * C4;
    const int m = m0 + row, n = n0 + c4 * 4;
    if (m >= p.M || n >= p.N) continue;
    const f32x4 v = *reinterpret_cast<const f32x4*>(sC + row * BN + c4 * 4);
    long rrow = m;
    if (p.res_mod > 0) { int t = rr0 + row; while (t >= p.res_mod) t -= p.res_mod; rrow = t; }
    const bool masked = p.rowmask != nullptr && p.rowmask[m];
    if (vec && (n + 3 < p.N)) {
      *reinterpret_cast<f32x4*>(p.C + (long)m * p.ldc + n) = gemm_epilogue4<false>(p, v, m, n, rrow, masked);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (n + e >= p.N) break;
        p.C[(long)m * p.ldc + n + e] = gemm_epilogue1<false>(p, v[e], m, n + e, rrow, masked);
      }
    }
  }
}
