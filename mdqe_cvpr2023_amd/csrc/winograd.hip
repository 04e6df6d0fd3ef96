// Stride-1, pad-1 3x3 convolution as fp32 Winograd F(2x2, 3x3) (Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", 2016).
//
// The exact-fp32 pipeline is bound by the matrix cores (the f32 MFMA runs at the vector rate), and the direct implicit GEMM spends
// 9 x Cin multiply-adds per output value.  F(2x2,3x3) computes a 2x2 output tile from a 4x4 input tile with 16 products of
// transformed values instead of 36: Y = A^T [ (G g G^T) .* (B^T d B) ] A.  Across channels the 16 element-wise products are 16
// independent GEMMs ("planes"):  M[p] = V[p] U[p]^T,  V[p] [T, Cin] (input tiles), U[p] [Cout, Cin] (weights), M[p] [T, Cout].
//
//   1. weight transform, once per weight:  U[16][Cout][Cin] = G g G^T, computed in double and rounded once;
//   2. input transform:                     V[16][T][Cin]   = B^T d B (adds / subtracts only, fp32);
//   3. the 16 plane products in ONE launch of the K-step-16 GEMM kernel (gemm_k16.hip, GemmParams::planes), plain epilogue;
//   4. output transform + epilogue:         Y = A^T M A + bias, activation, NHWC rows with pitch ldy.
//
// F(2x2) only: its transform constants are 0, +-1 (and 1/2 in G, applied in double), so the transforms add at most about one rounding
// of the direct kernel's error (measured in tests/test_winograd_cpu.py); F(4x4,3x3) would cost ~40x.  Images are processed in groups
// whose V + M fit a budget that stays inside the 256-MiB Infinity Cache; the group size depends only on the per-image shape, and
// every output tile depends only on its own input tile and the plane products' rows, which the GEMM computes independently of how
// many rows share the launch -- a frame's bits never depend on the other frames of its pass.
#include "common.h"
#include "gemm_params.h"

// V + M of one image group (bytes).  The transforms' round trip then lives in the Infinity Cache instead of HBM.
static const long kWinoGroupBytes = 128L << 20;

static int g_wino_tile = 0;        // tools/ A/B: 0 = by shape, else the K-step-16 tile code of the plane products
extern "C" int mdqe_debug_winograd_tile(int v) { g_wino_tile = v; return MDQE_OK; }

// U[p][n][c] = (G g G^T)[p / 4][p % 4] of g = Wt[n, :, :, c]; G = [[1,0,0],[1/2,1/2,1/2],[1/2,-1/2,1/2],[0,0,1]]
__global__ void __launch_bounds__(256)
wino_weight_kernel(const float* __restrict__ Wt, float* __restrict__ U, int Cout, int Cin) {
  const long n_all = (long)Cout * Cin;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += (long)gridDim.x * blockDim.x) {
    const int n = (int)(i / Cin), c = (int)(i % Cin);
    double g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) g[r][s] = (double)Wt[((long)n * 9 + r * 3 + s) * Cin + c];
    double t[4][3];                                  // G g
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      t[0][s] = g[0][s];
      t[1][s] = 0.5 * (g[0][s] + g[1][s] + g[2][s]);
      t[2][s] = 0.5 * (g[0][s] - g[1][s] + g[2][s]);
      t[3][s] = g[2][s];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                    // (G g) G^T
      const double u[4] = {t[r][0], 0.5 * (t[r][0] + t[r][1] + t[r][2]), 0.5 * (t[r][0] - t[r][1] + t[r][2]), t[r][2]};
#pragma unroll
      for (int s = 0; s < 4; ++s) U[(long)(r * 4 + s) * n_all + i] = (float)u[s];
    }
  }
}

// V[p][t][c] = (B^T d B)[p / 4][p % 4] of the 4x4 input tile d whose top-left pixel is (2 ty - 1, 2 tx - 1) (zero padding);
// B^T = [[1,0,-1,0],[0,1,1,0],[0,-1,1,0],[0,1,0,-1]].  One thread per (tile, 4 channels): Cin / 4 consecutive lanes read one
// pixel's channels as one contiguous run and write one plane row the same way.  Tiles never cross an image: a tile is (img, ty, tx).
__global__ void __launch_bounds__(256)
wino_input_kernel(const float* __restrict__ X, long img_stride, float* __restrict__ V, int T, int H, int Wd, int Cin, int tw, int tpi,
                  float* __restrict__ zeros, int nzero) {
  if (blockIdx.x == 0 && (int)threadIdx.x * 4 < nzero) *reinterpret_cast<f32x4*>(zeros + threadIdx.x * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
  const int c4n = Cin >> 2;
  const long n_all = (long)T * c4n;
  const long plane = (long)T * Cin;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i / c4n), c = (int)(i % c4n) * 4;
    const int img = t / tpi, r = t % tpi, ty = r / tw, tx = r % tw;
    const float* xi = X + (long)img * img_stride + c;
    f32x4 d[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int ih = 2 * ty - 1 + a;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int iw = 2 * tx - 1 + b;
        d[a][b] = (ih >= 0 && ih < H && iw >= 0 && iw < Wd) ? *reinterpret_cast<const f32x4*>(xi + ((long)ih * Wd + iw) * Cin)
                                                            : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    f32x4 e[4][4];                                   // B^T d
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      e[0][b] = d[0][b] - d[2][b];
      e[1][b] = d[1][b] + d[2][b];
      e[2][b] = d[2][b] - d[1][b];
      e[3][b] = d[1][b] - d[3][b];
    }
    float* vo = V + (long)t * Cin + c;
#pragma unroll
    for (int a = 0; a < 4; ++a) {                    // (B^T d) B
      const f32x4 v[4] = {e[a][0] - e[a][2], e[a][1] + e[a][2], e[a][2] - e[a][1], e[a][1] - e[a][3]};
#pragma unroll
      for (int b = 0; b < 4; ++b) *reinterpret_cast<f32x4*>(vo + (a * 4 + b) * plane) = v[b];
    }
  }
}

// Y(2 ty + a, 2 tx + b) = act((A^T M A)[a][b] + bias), A^T = [[1,1,1,0],[0,1,-1,-1]]; the outputs past an odd H / W are not written.
__global__ void __launch_bounds__(256)
wino_output_kernel(const float* __restrict__ Mp, const float* __restrict__ bias, float* __restrict__ Y, long ldy, int T, int H, int Wd,
                   int Cout, int tw, int tpi, int act) {
  const int n4n = Cout >> 2;
  const long n_all = (long)T * n4n;
  const long plane = (long)T * Cout;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_all; i += (long)gridDim.x * blockDim.x) {
    const int t = (int)(i / n4n), n = (int)(i % n4n) * 4;
    const int img = t / tpi, r = t % tpi, ty = r / tw, tx = r % tw;
    const float* mi = Mp + (long)t * Cout + n;
    f32x4 m[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) m[a][b] = *reinterpret_cast<const f32x4*>(mi + (a * 4 + b) * plane);
    f32x4 q[2][4];                                   // A^T M
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      q[0][b] = (m[0][b] + m[1][b]) + m[2][b];
      q[1][b] = (m[1][b] - m[2][b]) - m[3][b];
    }
    const f32x4 bv = bias != nullptr ? *reinterpret_cast<const f32x4*>(bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int oh = 2 * ty + a;
      if (oh >= H) break;
      f32x4 y[2] = {((q[a][0] + q[a][1]) + q[a][2]) + bv, ((q[a][1] - q[a][2]) - q[a][3]) + bv};
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int ow = 2 * tx + b;
        if (ow >= Wd) break;
        mdqe_act4(y[b], act, [](int) { return true; });
        *reinterpret_cast<f32x4*>(Y + (((long)img * H + oh) * Wd + ow) * ldy + n) = y[b];
      }
    }
  }
}

// images per group: V + M of the group within kWinoGroupBytes (at least one image) -- from the per-image shape only
static long wino_group(int H, int Wd, int Cin, int Cout) {
  const long tpi = (long)((H + 1) / 2) * ((Wd + 1) / 2);
  const long per_img = 16L * tpi * (Cin + Cout) * 4;
  const long g = kWinoGroupBytes / per_img;
  return g > 0 ? g : 1;
}

extern "C" long mdqe_winograd_workspace_bytes(int NI, int H, int Wd, int Cin, int Cout) {
  if (NI <= 0 || H <= 0 || Wd <= 0 || Cin <= 0 || Cout <= 0) return 0;
  long g = wino_group(H, Wd, Cin, Cout);
  if (g > NI) g = NI;
  const long tpi = (long)((H + 1) / 2) * ((Wd + 1) / 2);
  return 16L * g * tpi * (Cin + Cout) * 4 + (long)Cout * 4 + 256;
}

extern "C" int mdqe_winograd_weight_f32(const float* Wt, int Cout, int Cin, float* U, void* stream) {
  MDQE_REQUIRE(Cout > 0 && Cin > 0);
  MDQE_CHECK_PTR(Wt); MDQE_CHECK_PTR(U);
  const long n = (long)Cout * Cin;
  long nb = (n + 255) / 256; if (nb > 4096) nb = 4096;
  mdqe_clear_error();
  hipLaunchKernelGGL(wino_weight_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, Wt, U, Cout, Cin);
  return mdqe_launch_status();
}

extern "C" int mdqe_conv3x3_winograd_f32(const float* X, long x_img_stride, const float* U, const float* bias, float* Y, long ldy,
                                         int NI, int H, int Wd, int Cin, int Cout, int act, void* workspace, long ws_bytes, void* stream) {
  MDQE_REQUIRE(NI >= 0 && H > 0 && Wd > 0 && Cin > 0 && Cout > 0);
  MDQE_REQUIRE(Cin % 32 == 0 && Cout % 4 == 0 && ldy >= Cout && ldy % 4 == 0);
  if (mdqe_get_gemm_precision() != 0) return MDQE_EINVAL;           // exact fp32 mode only: the split modes keep the direct kernel
  if (NI == 0) return MDQE_OK;
  MDQE_CHECK_PTR(X); MDQE_CHECK_PTR(U); MDQE_CHECK_PTR(Y); MDQE_CHECK_PTR(workspace);
  MDQE_REQUIRE((((uintptr_t)X | (uintptr_t)U | (uintptr_t)Y | (uintptr_t)bias | (uintptr_t)workspace) & 15) == 0);
  if (x_img_stride <= 0) x_img_stride = (long)H * Wd * Cin;
  MDQE_REQUIRE(x_img_stride % 4 == 0 && x_img_stride >= (long)H * Wd * Cin);
  MDQE_REQUIRE(ws_bytes >= mdqe_winograd_workspace_bytes(NI, H, Wd, Cin, Cout));
  const int th = (H + 1) / 2, tw = (Wd + 1) / 2, tpi = th * tw;
  long g = wino_group(H, Wd, Cin, Cout);
  if (g > NI) g = NI;
  const long tmax = g * tpi;
  // one plane of V / M (and of U) is addressed through 32-bit buffer offsets by the GEMM
  MDQE_REQUIRE(tmax * Cin * 4 < 0xFFFF0000L && tmax * Cout * 4 < 0xFFFF0000L && (long)Cout * Cin * 4 < 0xFFFF0000L && tmax < 0x7FFFFFFFL);
  float* V = (float*)workspace;
  float* Mp = V + 16 * tmax * Cin;
  // a zero bias for the plane products: the GEMM's few-instruction epilogue is specialised for products with a bias (a bias-free copy
  // costs every K-step-16 kernel registers); x + 0 == x.  Written by the input transform of every group, ahead of the GEMM on the stream.
  float* zeros = Mp + 16 * tmax * Cout;
  MDQE_REQUIRE(Cout <= 1024);
  hipStream_t st = (hipStream_t)stream;
  mdqe_clear_error();
  for (int i0 = 0; i0 < NI; i0 += (int)g) {
    const int ni = (int)(NI - i0 < g ? NI - i0 : g);
    const int T = ni * tpi;
    const float* Xg = X + (long)i0 * x_img_stride;
    float* Yg = Y + (long)i0 * H * Wd * ldy;
    long nb = ((long)T * (Cin / 4) + 255) / 256; if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)nb), dim3(256), 0, st, Xg, x_img_stride, V, T, H, Wd, Cin, tw, tpi, zeros, Cout);
    GemmParams p = {};
    p.A = V; p.W = U; p.C = Mp; p.M = T; p.N = Cout; p.K = Cin; p.lda = Cin; p.ldc = Cout; p.conv = 0;
    p.bias = zeros; p.act = MDQE_ACT_NONE; p.a_bytes = (unsigned)((long)T * Cin * 4); p.w_bytes = (unsigned)((long)Cout * Cin * 4);
    p.ksplit = 1; p.kchunk = Cin; p.vec_ok = 1;
    p.planes = 16; p.plane_a = (long)T * Cin; p.plane_w = (long)Cout * Cin; p.plane_c = (long)T * Cout;
    // tile: 64 x 64, one constant.  The group budget caps T * (Cin + Cout), so a group's 16 planes never reach the grid sizes at which
    // dispatch_gemm's rule picks a larger tile (b128 >= 2000) unless one image alone exceeds the budget; measured on the 360p pass, the
    // 128 x 64 and 128 x 128 tiles are within noise of it (profiles/r07_winograd_frame_gemm_table_360p.txt).  A constant also keeps the
    // tile independent of how many images a group holds.  (Bits do not depend on the tile either way: every K-step-16 tile accumulates an
    // element over K in the same order, the assumption dispatch_gemm's own shape-dependent rule already rests on.)
    const int tile = g_wino_tile != 0 ? g_wino_tile : 3;
    int rc = mdqe_launch_gemm_k16(p, tile, st);
    if (rc != MDQE_OK) return rc;
    nb = ((long)T * (Cout / 4) + 255) / 256; if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(wino_output_kernel, dim3((unsigned)nb), dim3(256), 0, st, Mp, bias, Yg, ldy, T, H, Wd, Cout, tw, tpi, act);
    rc = mdqe_launch_status();
    if (rc != MDQE_OK) return rc;
  }
  return MDQE_OK;
}
