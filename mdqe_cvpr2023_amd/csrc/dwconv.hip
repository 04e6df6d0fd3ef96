// Depthwise 5x5 kernels of the mask-feature head for C == 256 (one wave = the 64 float4 channel groups of a pixel, so a
// lane's 25 filter taps live in registers for the whole kernel and every bounds decision is wave-uniform):
//
//  * dw5_c256_kernel: plain depthwise 5x5 (DepthwiseSeparableConv2d.depthwise, segmentation.py:92-98,112), two
//    horizontally adjacent outputs per step (30 loads for 2 outputs instead of 50).
//  * dw5_up2_c256_kernel: ConvTranspose2d(k=1, s=2, output_padding=1, groups=C) -> depthwise 5x5 (segmentation.py:28-29,59)
//    in one pass.  The upsampled tensor is virtual: up[2i,2j] = x[i,j]*tw + tb, every other position = tb.  A 2x2 output
//    quad (2a+dy, 2b+dx) touches only x[a-1..a+1][b-1..b+1] and uses each of the 25 taps exactly once:
//    out = bias + tb * (sum of the in-bounds taps) + tw * (sum over the even-even taps of w * x)
//    -- 9 loads and 25 float4 FMAs per quad instead of 100 tap visits.
#include "common.h"

namespace {
__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
}

__global__ void __launch_bounds__(256, 2)
dw5_c256_kernel(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias, float* __restrict__ y,
                int NI, int H, int W) {
  constexpr int C = 256;
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  f32x4 w[25];
#pragma unroll
  for (int t = 0; t < 25; ++t) w[t] = ld4(wt + t * C + lane * 4);
  const f32x4 bv = ld4(bias + lane * 4);
  const int Wp = (W + 1) / 2;                         // output pairs per row
  const long total = (long)NI * H * Wp;
  for (long i = wid; i < total; i += nw) {
    const int pw_ = (int)(i % Wp); const long t = i / Wp;
    const int hh = (int)(t % H), img = (int)(t / H);
    const int w0 = pw_ * 2;
    f32x4 a0 = bv, a1 = bv;
#pragma unroll
    for (int kh = 0; kh < 5; ++kh) {
      const int ih = hh - 2 + kh;
      if (ih < 0 || ih >= H) continue;               // wave-uniform
      const float* row = x + (((long)img * H + ih) * W) * C + lane * 4;
      f32x4 X[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int iw = w0 - 2 + c;
        X[c] = (iw >= 0 && iw < W) ? ld4(row + (long)iw * C) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int kw = 0; kw < 5; ++kw) { a0 += X[kw] * w[kh * 5 + kw]; a1 += X[kw + 1] * w[kh * 5 + kw]; }
    }
    float* o = y + (((long)img * H + hh) * W + w0) * C + lane * 4;
    *reinterpret_cast<f32x4*>(o) = a0;
    if (w0 + 1 < W) *reinterpret_cast<f32x4*>(o + C) = a1;
  }
}

__global__ void __launch_bounds__(256, 2)
dw5_up2_c256_kernel(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                    const float* __restrict__ tw, const float* __restrict__ tb, float* __restrict__ y, int NI, int Hs, int Ws) {
  constexpr int C = 256;
  const int lane = threadIdx.x & 63;
  const long wid = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  const int H = 2 * Hs, W = 2 * Ws;
  f32x4 w[25];
#pragma unroll
  for (int t = 0; t < 25; ++t) w[t] = ld4(wt + t * C + lane * 4);
  const f32x4 bv = ld4(bias + lane * 4), twv = ld4(tw + lane * 4), tbv = ld4(tb + lane * 4);
  f32x4 wall = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 25; ++t) wall += w[t];
  const f32x4 cin = bv + tbv * wall;                  // constant part of an interior output

  const long total = (long)NI * Hs * Ws;
  for (long i = wid; i < total; i += nw) {
    const int b = (int)(i % Ws); const long t = i / Ws;
    const int a = (int)(t % Hs), img = (int)(t / Hs);
    f32x4 o00 = {0.f, 0.f, 0.f, 0.f}, o01 = o00, o10 = o00, o11 = o00;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int ia = a - 1 + r;
      if (ia < 0 || ia >= Hs) continue;              // wave-uniform
      const float* row = x + (((long)img * Hs + ia) * Ws) * C + lane * 4;
      f32x4 X[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int ib = b - 1 + c;
        X[c] = (ib >= 0 && ib < Ws) ? ld4(row + (long)ib * C) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
      // output (dy,dx) of the quad uses taps kh = 2r - dy, kw = 2c - dx
#pragma unroll
      for (int c = 0; c < 3; ++c) o00 += X[c] * w[(2 * r) * 5 + 2 * c];
#pragma unroll
      for (int c = 1; c < 3; ++c) o01 += X[c] * w[(2 * r) * 5 + 2 * c - 1];
      if (r >= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) o10 += X[c] * w[(2 * r - 1) * 5 + 2 * c];
#pragma unroll
        for (int c = 1; c < 3; ++c) o11 += X[c] * w[(2 * r - 1) * 5 + 2 * c - 1];
      }
    }
    f32x4 c00 = cin, c01 = cin, c10 = cin, c11 = cin;
    if (a == 0 || a == Hs - 1 || b == 0 || b == Ws - 1) {          // border quad (wave-uniform): only in-bounds taps count
      auto cst = [&](int hh, int ww) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 5; ++kh) {
          const int ih = hh - 2 + kh;
          if (ih < 0 || ih >= H) continue;
#pragma unroll
          for (int kw = 0; kw < 5; ++kw) {
            const int iw = ww - 2 + kw;
            if (iw >= 0 && iw < W) s += w[kh * 5 + kw];
          }
        }
        return bv + tbv * s;
      };
      c00 = cst(2 * a, 2 * b); c01 = cst(2 * a, 2 * b + 1); c10 = cst(2 * a + 1, 2 * b); c11 = cst(2 * a + 1, 2 * b + 1);
    }
    float* o = y + (((long)img * H + 2 * a) * W + 2 * b) * C + lane * 4;
    *reinterpret_cast<f32x4*>(o) = c00 + twv * o00;
    *reinterpret_cast<f32x4*>(o + C) = c01 + twv * o01;
    *reinterpret_cast<f32x4*>(o + (long)W * C) = c10 + twv * o10;
    *reinterpret_cast<f32x4*>(o + (long)W * C + C) = c11 + twv * o11;
  }
}

// dw5_up2_c256_kernel + the 256 -> 32 projection behind it (out_lay2.pointwise) in one kernel: the [NI, 2Hs, 2Ws, 256] tensor between
// them -- 629 MB per 40-frame 360p pass, written once and read once by nothing else -- never reaches memory.  A wave takes a strip of 8
// quads of one quad row (tile = 32 output pixels), computes each quad exactly as dw5_up2_c256_kernel does (same expressions in the same
// order, taps in registers, the border constants) from the strip's 3 x 10 input pixels, and puts the 32 rows of 256 channels into its own
// 32-KB LDS tile (16-B chunk c of row r at c ^ (r & 15): the row writes and the fragment reads below are both conflict-free).  The tile is
// then multiplied by the [32, 256] weight with v_mfma_f32_32x32x2_f32 in the K order of gemm_k16.hip's mma_stage -- per 16-wide K-step
// the k pairs (0,4) (1,5) (2,6) (3,7) (8,12) (9,13) (10,14) (11,15), lane half lh supplying the second of a pair, from a zero
// accumulator -- so a row's sum is the sum ops.linear forms for it, bit for bit; bias is added afterwards as gemm_epilogue4 does.
// Every wave multiplies its own tile, so the weight's fragments live in the wave's registers (128 VGPRs: lane (lr, lh) only ever needs
// row lr, chunks lh and 2 + lh of every K-step) instead of a 32-KB LDS image per block: 4 x 32 KB of tiles + 32 KB would be the CU's
// whole 160 KB.  One block of 4 waves per CU, one wave per SIMD; the next strip's 30 loads are issued before the 128 MFMAs of the
// current one and land behind them.  Nothing is block-wide: no barrier.
__global__ void __launch_bounds__(256, 1)
dw5_up2_pw_c256_kernel(const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ bias,
                       const float* __restrict__ tw, const float* __restrict__ tb, const float* __restrict__ pw,
                       const float* __restrict__ pb, float* __restrict__ out, long ldo, int NI, int Hs, int Ws) {
  constexpr int C = 256, QT = 8;                       // channels; quads per strip
  extern __shared__ __attribute__((aligned(16))) float dwpw_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  float* const tile = dwpw_lds + wave * (32 * C);
  const long wid = (long)blockIdx.x * 4 + wave, nw = (long)gridDim.x * 4;
  const int H = 2 * Hs, W = 2 * Ws;
  const int lr = lane & 31, lh = lane >> 5;
  f32x4 w[25];
#pragma unroll
  for (int t = 0; t < 25; ++t) w[t] = ld4(wt + t * C + lane * 4);
  const f32x4 bv = ld4(bias + lane * 4), twv = ld4(tw + lane * 4), tbv = ld4(tb + lane * 4);
  f32x4 wall = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 25; ++t) wall += w[t];
  const f32x4 cin = bv + tbv * wall;                  // constant part of an interior output
  f32x4 B0[16], B1[16];                               // weight fragments: K-step kt, halves k = 16 kt + 4 lh + s and 16 kt + 8 + 4 lh + s
#pragma unroll
  for (int kt = 0; kt < 16; ++kt) {
    B0[kt] = ld4(pw + lr * C + kt * 16 + lh * 4);
    B1[kt] = ld4(pw + lr * C + kt * 16 + 8 + lh * 4);
  }
  const f32x4 pbv = ld4(pb + (lane & 7) * 4);

  const int Wt = (Ws + QT - 1) / QT;                  // strips per quad row
  const long total = (long)NI * Hs * Wt;
  f32x4 X[3][QT + 2];
  auto load_strip = [&](long i) __attribute__((always_inline)) {
    const int b0 = (int)(i % Wt) * QT; const long t = i / Wt;
    const int a = (int)(t % Hs), img = (int)(t / Hs);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int ia = a - 1 + r;
      const bool rok = ia >= 0 && ia < Hs;             // wave-uniform
      const float* row = x + (((long)img * Hs + (rok ? ia : a)) * Ws) * C + lane * 4;
#pragma unroll
      for (int c = 0; c < QT + 2; ++c) {
        const int ib = b0 - 1 + c;
        X[r][c] = (rok && ib >= 0 && ib < Ws) ? ld4(row + (long)ib * C) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  long i = wid;
  if (i < total) load_strip(i);
  while (i < total) {
    const int b0 = (int)(i % Wt) * QT; const long ti = i / Wt;
    const int a = (int)(ti % Hs), img = (int)(ti / Hs);
    const int nq = min(QT, Ws - b0);                   // quads of the strip inside the row (wave-uniform)
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      if (q >= nq) continue;                           // (their tile rows keep stale values: a row of the product depends on its own row only)
      const int b = b0 + q;
      f32x4 o00 = {0.f, 0.f, 0.f, 0.f}, o01 = o00, o10 = o00, o11 = o00;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int ia = a - 1 + r;
        if (ia < 0 || ia >= Hs) continue;              // wave-uniform
        // output (dy,dx) of the quad uses taps kh = 2r - dy, kw = 2c - dx
#pragma unroll
        for (int c = 0; c < 3; ++c) o00 += X[r][q + c] * w[(2 * r) * 5 + 2 * c];
#pragma unroll
        for (int c = 1; c < 3; ++c) o01 += X[r][q + c] * w[(2 * r) * 5 + 2 * c - 1];
        if (r >= 1) {
#pragma unroll
          for (int c = 0; c < 3; ++c) o10 += X[r][q + c] * w[(2 * r - 1) * 5 + 2 * c];
#pragma unroll
          for (int c = 1; c < 3; ++c) o11 += X[r][q + c] * w[(2 * r - 1) * 5 + 2 * c - 1];
        }
      }
      f32x4 c00 = cin, c01 = cin, c10 = cin, c11 = cin;
      if (a == 0 || a == Hs - 1 || b == 0 || b == Ws - 1) {          // border quad (wave-uniform): only in-bounds taps count
        auto cst = [&](int hh, int ww) {
          f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kh = 0; kh < 5; ++kh) {
            const int ih = hh - 2 + kh;
            if (ih < 0 || ih >= H) continue;
#pragma unroll
            for (int kw = 0; kw < 5; ++kw) {
              const int iw = ww - 2 + kw;
              if (iw >= 0 && iw < W) s += w[kh * 5 + kw];
            }
          }
          return bv + tbv * s;
        };
        c00 = cst(2 * a, 2 * b); c01 = cst(2 * a, 2 * b + 1); c10 = cst(2 * a + 1, 2 * b); c11 = cst(2 * a + 1, 2 * b + 1);
      }
      // tile rows 4q .. 4q+3 = outputs (dy,dx) = (0,0) (0,1) (1,0) (1,1) of quad q; this lane's chunk is `lane`
      *reinterpret_cast<f32x4*>(tile + (4 * q + 0) * C + ((lane ^ ((4 * q + 0) & 15)) << 2)) = c00 + twv * o00;
      *reinterpret_cast<f32x4*>(tile + (4 * q + 1) * C + ((lane ^ ((4 * q + 1) & 15)) << 2)) = c01 + twv * o01;
      *reinterpret_cast<f32x4*>(tile + (4 * q + 2) * C + ((lane ^ ((4 * q + 2) & 15)) << 2)) = c10 + twv * o10;
      *reinterpret_cast<f32x4*>(tile + (4 * q + 3) * C + ((lane ^ ((4 * q + 3) & 15)) << 2)) = c11 + twv * o11;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const long inext = i + nw;
    if (inext < total) load_strip(inext);              // X is free again: the next strip's loads fly behind the MFMAs

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* const arow = tile + lr * C;
#pragma unroll
    for (int kt = 0; kt < 16; ++kt) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(arow + (((4 * kt + lh) ^ (lr & 15)) << 2));
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(arow + (((4 * kt + 2 + lh) ^ (lr & 15)) << 2));
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], B0[kt][s], acc, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], B1[kt][s], acc, 0, 0, 0);
    }
    // acc[r] = C(row (r & 3) + 8 (r >> 2) + 4 lh, column lr): restaged through the head of the tile so that a lane owns 4 consecutive
    // columns of a row and 8 lanes store one 128-B row of the result
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[((r & 3) + 8 * (r >> 2) + 4 * lh) * 32 + lr] = acc[r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int row = it * 8 + (lane >> 3), c4 = lane & 7;
      const int q = row >> 2, dy = (row >> 1) & 1, dx = row & 1;
      const f32x4 v = *reinterpret_cast<const f32x4*>(tile + row * 32 + c4 * 4) + pbv;
      if (q < nq) {
        const long pix = ((long)img * H + 2 * a + dy) * W + 2 * (b0 + q) + dx;
        *reinterpret_cast<f32x4*>(out + pix * ldo + c4 * 4) = v;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    i = inext;
  }
}

extern "C" int mdqe_dwconv5x5_c256_f32(const float* x, const float* wt, const float* bias, float* y, int NI, int H, int W,
                                       void* stream) {
  MDQE_REQUIRE(NI >= 0 && H > 0 && W > 0);
  if (NI == 0) return MDQE_OK;
  MDQE_CHECK_PTR(x); MDQE_CHECK_PTR(wt); MDQE_CHECK_PTR(bias); MDQE_CHECK_PTR(y);
  mdqe_clear_error();
  const long total = (long)NI * H * ((W + 1) / 2);
  long nb = (total + 3) / 4; if (nb > 256 * 8) nb = 256 * 8;
  hipLaunchKernelGGL(dw5_c256_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, wt, bias, y, NI, H, W);
  return mdqe_launch_status();
}

// x [NI,Hs,Ws,256] -> y [NI,2Hs,2Ws,256] = depthwise5x5(transposed-conv-x2(x)); wt [25,256], bias/tw/tb [256]
extern "C" int mdqe_dwconv5x5_up2_c256_f32(const float* x, const float* wt, const float* bias, const float* tw, const float* tb,
                                           float* y, int NI, int Hs, int Ws, void* stream) {
  MDQE_REQUIRE(NI >= 0 && Hs > 0 && Ws > 0);
  if (NI == 0) return MDQE_OK;
  MDQE_CHECK_PTR(x); MDQE_CHECK_PTR(wt); MDQE_CHECK_PTR(bias); MDQE_CHECK_PTR(tw); MDQE_CHECK_PTR(tb); MDQE_CHECK_PTR(y);
  mdqe_clear_error();
  const long total = (long)NI * Hs * Ws;
  long nb = (total + 3) / 4; if (nb > 256 * 8) nb = 256 * 8;
  hipLaunchKernelGGL(dw5_up2_c256_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, wt, bias, tw, tb, y, NI, Hs, Ws);
  return mdqe_launch_status();
}

// out[pixel, 0:32] = pw [32,256] . depthwise5x5(transposed-conv-x2(x))[pixel, :] + pb: the bits of mdqe_dwconv5x5_up2_c256_f32 followed
// by mdqe_gemm_nt_f32 (exact fp32), without the tensor between them.  out rows are ldo floats apart (the caller's pitch).
extern "C" int mdqe_dwconv5x5_up2_pw_c256_f32(const float* x, const float* wt, const float* bias, const float* tw, const float* tb,
                                              const float* pw, const float* pb, float* out, long ldo, int NI, int Hs, int Ws,
                                              void* stream) {
  MDQE_REQUIRE(NI >= 0 && Hs > 0 && Ws > 0 && ldo >= 32 && ldo % 4 == 0);
  if (NI == 0) return MDQE_OK;
  MDQE_CHECK_PTR(x); MDQE_CHECK_PTR(wt); MDQE_CHECK_PTR(bias); MDQE_CHECK_PTR(tw); MDQE_CHECK_PTR(tb);
  MDQE_CHECK_PTR(pw); MDQE_CHECK_PTR(pb); MDQE_CHECK_PTR(out);
  MDQE_REQUIRE((((uintptr_t)x | (uintptr_t)wt | (uintptr_t)bias | (uintptr_t)tw | (uintptr_t)tb | (uintptr_t)pw | (uintptr_t)pb |
                 (uintptr_t)out) & 15) == 0);
  mdqe_clear_error();
  static int num_cus = 0;                              // one block per CU (128 KB of LDS each)
  if (num_cus == 0) {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    num_cus = n;
  }
  const int smem = 4 * 32 * 256 * (int)sizeof(float);
  if (mdqe_allow_lds(reinterpret_cast<const void*>(dw5_up2_pw_c256_kernel), smem) != hipSuccess) return MDQE_ELAUNCH;
  const long total = (long)NI * Hs * ((Ws + 7) / 8);
  long nb = (total + 3) / 4; if (nb > num_cus) nb = num_cus;
  hipLaunchKernelGGL(dw5_up2_pw_c256_kernel, dim3((unsigned)nb), dim3(256), (size_t)smem, (hipStream_t)stream, x, wt, bias, tw, tb, pw,
                     pb, out, ldo, NI, Hs, Ws);
  return mdqe_launch_status();
}
