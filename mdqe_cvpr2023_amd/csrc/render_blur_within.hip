// The edge-stopping blur overlay: render_blur.hip's two painters with a blur that stays INSIDE the blurred region -- a normalised,
// membership-weighted separable Gaussian.  A pixel is a member when its action is 3; the taps weigh m * s and m, nothing is rounded
// between the passes, and a blurred sample is (N + D / 2) / D, one exact division.  ONE definition, integers only (include/mdqe_hip.h has
// the rule); tests/_blur_within_ref.py restates it in numpy and every comparison is exact.
//
// The tile scheme is render_blur.hip's (render_blur_tile.h): 256 threads own 16 x 64 output pixels plus a halo, phases between barriers:
//   1 flag    as the plain kernel: a tile without a pixel of action 3 goes straight to the paint phase;
//   2 load    (16 + 2R) x (64 + 2R) halo pixels, coordinates clamped to the picture.  The halo needs the LABELS too: a pixel's membership
//             is looked up first, and only a member's source is read at all (a non-member's value cannot reach the result).  RGB: one
//             packed dword per pixel, m * c0 | m * c1 << 8 | m * c2 << 16 | m << 24; surfaces: one 16-bit word per sample, m * value |
//             m << 15 (luma; U and V of the pairs under the tile, a pair being a member when any in-picture pixel of its block is);
//   3 first   one direction's sums, exact: Hn_c in 32-bit planes (20 bits, 22 for P010) and Hw in one 16-bit plane (13 bits).  RGB takes
//             the two dwords of a distance apart into two 16-bit lanes each ((a & 0x00FF00FF) + (b & 0x00FF00FF): c0 and c2, the same of
//             a >> 8, b >> 8: c1 and m), so a distance costs two LDS loads for four quantities;
//   4 second  N_c and D, the other direction's sums over those planes: 32-bit sums for 8-bit values (N + D / 2 < 2^32), 64-bit sums for
//             P010.  A thread divides only where the centre is a member (D >= taps[0]^2 > 0 there; elsewhere D may be 0 and nothing is
//             computed): 32-bit values by the compiler's exact unsigned division, P010 by a float quotient with an integer fix-up
//             (`rdiv`).  RGB: the result plane (one packed dword per pixel) takes the place of the dead source plane -- the centres'
//             membership bits are read into a register and a barrier passes before the first result is written;
//   5 paint   the plain kernel's painters, the same functions: RGB in groups of 4 pixels laid out from the OUTPUT address (paint_rgb_tile
//             of render_tile_paint.h), surfaces one 2 x 2 block per thread (paint_blur_blocks of render_blur_tile.h).
// Which direction is first is the kernel's to choose: the plain rule rounds after its row pass, which fixes its order; this rule rounds
// nowhere between the passes, so N and D are the same double sum either way, bit for bit.  Rows first (render_blur.hip's order) sums
// at (16 + 2R) x 64 positions and keeps as many in LDS; columns first at 16 x (64 + 2R): 2048 positions against 5120 at R = 32, and
// with the second pass's 1024 half the tap work of the kernel.  Both were built for every radius and measured on the dense window of
// tools/blur_edge_ab.py (label + overlay stage, us per call, RGB, blur="tracks"; dynamic LDS in bytes):
//     R                   4              8             16              32
//     rows first     264.3  28416   328.2  38912   631.1  61440   1966.8  112640   (one block per CU at R = 32)
//     columns first  312.9  23040   353.6  28160   472.7  39936    893.8   69632
// (NV12: 282 / 335 / 596 / 1316 against 314 / 348 / 438 / 722.)  So the order goes by the padded radius, per plane: rows first up to
// R = 8 (`ROWS_FIRST_TO`), columns first from 16 -- a surface's chroma planes by their own radius.  The two orders are two KERNELS
// (the template flag CF): with both in one kernel the rows-first radii ran with the registers of the columns-first passes (163
// VGPRs against 55) and lost what they had won -- 306 / 362 us at R = 4 / 8.  The tile stays 16 x 64 at every
// radius and Hn stays 32 bits wide; the dynamic LDS is 4 (16 + 2R)(64 + 2R) bytes of source and 14 bytes per kept sum for RGB:
//     R            0       4       8      16      24      32
//     RGB       18432   28416   38912   39936   53760   69632  bytes
//     surfaces  14848   23424   28160   33792   43520   51200  bytes (with Rc = (R + 1) / 2 padded: 0, 4, 4, 8, 16, 16)
// Only RGB at R = 32 is above 64 KB: that launch asks for it with mdqe_allow_lds, and two blocks still share a CU's 160 KB.  A narrower
// tile at the large radii or Hn packed into 24 bits would save LDS that no longer limits the blocks per CU; neither was built.
// Both passes run over the whole tile of a flagged tile, whatever the labels: no data-dependent order, no atomics, no global scratch,
// identical from run to run.  The argument structs, the entries' checks and the kernels' first phase are the plain blur's too
// (render_blur_tile.h: BlurArgs, BlurYuvArgs, blur_rgb_call, blur_yuv_call, tile_begin); this file holds the passes, the LDS plans, the
// load phases and the launches.
#include "render_blur_tile.h"

namespace {

constexpr int ROWS_FIRST_TO = 8;                 // the largest padded radius whose row pass runs first (measured: the file's head)
// the positions the first pass sums at and keeps, for a tile of th x tw and the padded radius R
__host__ __device__ constexpr int kept_sums(int th, int tw, int R) { return R <= ROWS_FIRST_TO ? (th + 2 * R) * tw : th * (tw + 2 * R); }
// `with_radius` over one order's radii only: a kernel is compiled per order (CF: columns first), so that the rows-first kernel does
// not carry the registers of the columns-first passes (163 against 87 VGPRs in one kernel: a wave less per SIMD at every radius).
template <bool CF, class Fn>
__device__ __forceinline__ void with_radius_of(int R, Fn&& fn) {
  if (CF) {
    switch (R) {
      case 16: fn(std::integral_constant<int, 16>()); break;
      case 24: fn(std::integral_constant<int, 24>()); break;
      default: fn(std::integral_constant<int, 32>()); break;
    }
  } else {
    switch (R) {
      case 0: fn(std::integral_constant<int, 0>()); break;
      case 4: fn(std::integral_constant<int, 4>()); break;
      default: fn(std::integral_constant<int, 8>()); break;
    }
  }
}
constexpr size_t LDS_ASK = 60 * 1024;            // a launch with more dynamic LDS than this asks for it (the static LDS stays below 4 KB)

// (n + D / 2) / D, exact.  32 bits: n + D / 2 < 2^32 by the header's bound.
__device__ __forceinline__ uint32_t rdiv(uint32_t n, uint32_t D) { return (n + (D >> 1)) / D; }

// The same for a 64-bit n with a quotient below 2^11 (a weighted mean of 10-bit values) and D <= 2^24: D is exact as a float, n is
// rounded by at most 2^-24 of itself and so is the quotient, which is below 2^11 -- the truncated float quotient is off by at most
// one, and one step either way makes it exact.
__device__ __forceinline__ uint32_t rdiv(uint64_t n, uint32_t D) {
  const uint64_t v = n + (D >> 1);
  uint32_t q = (uint32_t)((float)v / (float)D);
  int64_t r = (int64_t)v - (int64_t)((uint64_t)q * D);
  if (r < 0) { --q; r += D; }
  if (r >= (int64_t)D) ++q;
  return q;
}

// The tap sums of phase 3, each said once for a centre and its R neighbours either way, S words apart: S is 1 along a row, the row
// length of the plane along a column -- a compile-time constant in every pass, and the loops are fully unrolled per padded radius.  The
// results go to hn[.. + i] and hw[i], indexed here as the passes index everything else.  (Phase 4's two passes carry their own tap
// loops: DESIGN.md §4, "Where the painters' rule lives", has the registers that decide it.)
// RGB: hn[k * hplane + i] = sum_d taps[|d|] * (m * c_k)(q + d * S) and hw[i] = sum_d taps[|d|] * m over packed dwords.  The two dwords
// of a distance go apart into two 16-bit lanes each: a lane of a pair's sum is at most 510, a sum at most 4096 * 255.
template <int R, int S>
__device__ __forceinline__ void first_sums_rgb(const uint32_t* q, const uint32_t* taps, uint32_t* hn, int hplane, unsigned short* hw, int i) {
  const uint32_t x = q[0], w0 = taps[0];
  uint32_t a0 = w0 * (x & 0xFFu), a1 = w0 * ((x >> 8) & 0xFFu), a2 = w0 * ((x >> 16) & 0xFFu), aw = w0 * (x >> 24);
#pragma unroll
  for (int d = 1; d <= R; ++d) {
    const uint32_t w = taps[d], xa = q[-d * S], xb = q[d * S];
    const uint32_t e = (xa & 0x00FF00FFu) + (xb & 0x00FF00FFu);                       // c0 | c2 << 16
    const uint32_t o = ((xa >> 8) & 0x00FF00FFu) + ((xb >> 8) & 0x00FF00FFu);         // c1 | m << 16
    a0 += w * (e & 0xFFFFu); a2 += w * (e >> 16);
    a1 += w * (o & 0xFFFFu); aw += w * (o >> 16);
  }
  hn[i] = a0; hn[hplane + i] = a1; hn[2 * hplane + i] = a2;
  hw[i] = (unsigned short)aw;
}

// Surfaces: the same for NP planes (`splane` words apart) of 16-bit words m * value | m << 15 (every plane carries the bit;
// plane 0's is summed).  A sum is at most 4096 * 1023.
template <int NP, int R, int S>
__device__ __forceinline__ void first_sums_yuv(const unsigned short* q, int splane, const uint32_t* taps, uint32_t* hn, int hplane, unsigned short* hw,
                                               int i) {
  uint32_t acc[NP], aw = taps[0] * ((uint32_t)q[0] >> 15);
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = taps[0] * ((uint32_t)q[p * splane] & 0x7FFFu);
#pragma unroll
  for (int d = 1; d <= R; ++d) {
    const uint32_t w = taps[d];
    aw += w * (((uint32_t)q[-d * S] >> 15) + ((uint32_t)q[d * S] >> 15));
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] += w * (((uint32_t)q[p * splane - d * S] & 0x7FFFu) + ((uint32_t)q[p * splane + d * S] & 0x7FFFu));
  }
#pragma unroll
  for (int p = 0; p < NP; ++p) hn[p * hplane + i] = acc[p];
  hw[i] = (unsigned short)aw;
}

// ROWS FIRST (R <= 8).  Phase 3, RGB: the horizontal sums at `rows` rows of TW columns, i = r * TW + c; s rows are `pitch` dwords apart.
template <int R>
__device__ __forceinline__ void row_pass_rgb(const uint32_t* s, int pitch, uint32_t* hn, int hplane, unsigned short* hw, const uint32_t* taps,
                                             int rows, int tid) {
  for (int i = tid; i < rows * TW; i += 256) first_sums_rgb<R, 1>(s + (i / TW) * pitch + i % TW + R, taps, hn, hplane, hw, i);
}

// Phase 3, surfaces, rows first: the same at `rows` rows of COLS columns of NP planes.
template <int COLS, int NP, int R>
__device__ __forceinline__ void row_pass_yuv(const unsigned short* s, int pitch, int splane, uint32_t* hn, int hplane, unsigned short* hw,
                                             const uint32_t* taps, int rows, int tid) {
  for (int i = tid; i < rows * COLS; i += 256)
    first_sums_yuv<NP, R, 1>(s + (i / COLS) * pitch + i % COLS + R, splane, taps, hn, hplane, hw, i);
}

// Phase 4, rows first: fin(i, N[NP], D) for i = r * COLS + c over `rows` rows, N_p = sum_d taps[|d|] * hn[p][r + R + d][c] in the type ACC and
// D = sum_d taps[|d|] * hw[r + R + d][c] (<= 2^24); the planes hold rows + 2R rows.  Every term is part of its sum, so with ACC 32
// bits wide nothing wraps where the sum fits (8-bit values); a pair's hn sum is below 2^23.
template <int COLS, int NP, int R, class ACC, class Fin>
__device__ __forceinline__ void column_pass_within(const uint32_t* hn, int hplane, const unsigned short* hw, const uint32_t* taps, int rows,
                                                   int tid, Fin fin) {
  for (int i = tid; i < rows * COLS; i += 256) {
    const uint32_t* q = hn + i + R * COLS;
    const unsigned short* qw = hw + i + R * COLS;
    ACC acc[NP];
    uint32_t D = taps[0] * (uint32_t)qw[0];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = (ACC)taps[0] * q[p * hplane];
#pragma unroll
    for (int d = 1; d <= R; ++d) {
      const uint32_t w = taps[d];
      D += w * ((uint32_t)qw[-d * COLS] + (uint32_t)qw[d * COLS]);
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p] += (ACC)w * (q[p * hplane - d * COLS] + q[p * hplane + d * COLS]);
    }
    fin(i, acc, D);
  }
}

// COLUMNS FIRST (R >= 16).  Phase 3, RGB: the VERTICAL sums of the TH tile rows over all SW = TW + 2R halo columns, i = r * SW + c.
template <int R>
__device__ __forceinline__ void column_pass_rgb(const uint32_t* s, uint32_t* hn, unsigned short* hw, const uint32_t* taps, int tid) {
  constexpr int SW = TW + 2 * R;
  for (int i = tid; i < TH * SW; i += 256) first_sums_rgb<R, SW>(s + i + R * SW, taps, hn, TH * SW, hw, i);
}

// Phase 3, surfaces, columns first: the same for NP planes of ROWS tile rows and SW = COLS + 2R columns.
template <int ROWS, int COLS, int NP, int R>
__device__ __forceinline__ void column_pass_yuv(const unsigned short* s, int splane, uint32_t* hn, unsigned short* hw, const uint32_t* taps,
                                                int tid) {
  constexpr int SW = COLS + 2 * R;
  for (int i = tid; i < ROWS * SW; i += 256) first_sums_yuv<NP, R, SW>(s + i + R * SW, splane, taps, hn, ROWS * SW, hw, i);
}

// Phase 4, columns first: fin(i, N[NP], D) for i = r * COLS + c over ROWS rows: the HORIZONTAL sums over the planes of phase 3 (ROWS rows of COLS +
// 2R columns), N_p = sum_d taps[|d|] * hn[p][r][c + R + d] in the type ACC and D = sum_d taps[|d|] * hw[r][c + R + d] (<= 2^24).  Every
// term is part of its sum, so with ACC 32 bits wide nothing wraps where the sum fits (8-bit values); a pair's hn sum is below 2^23.
template <int ROWS, int COLS, int NP, int R, class ACC, class Fin>
__device__ __forceinline__ void row_pass_within(const uint32_t* hn, const unsigned short* hw, const uint32_t* taps, int tid, Fin fin) {
  constexpr int SW = COLS + 2 * R, hplane = ROWS * SW;
  for (int i = tid; i < ROWS * COLS; i += 256) {
    const int at = (i / COLS) * SW + i % COLS + R;
    const uint32_t* q = hn + at;
    const unsigned short* qw = hw + at;
    ACC acc[NP];
    uint32_t D = taps[0] * (uint32_t)qw[0];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = (ACC)taps[0] * q[p * hplane];
#pragma unroll
    for (int d = 1; d <= R; ++d) {
      const uint32_t w = taps[d];
      D += w * ((uint32_t)qw[-d] + (uint32_t)qw[d]);
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p] += (ACC)w * (q[p * hplane - d] + q[p * hplane + d]);
    }
    fin(i, acc, D);
  }
}

// ---- RGB ----------------------------------------------------------------------------------------------------------------------------
template <int KIND, int CR, bool CF>              // CF: the kernel of the padded radii 16, 24, 32 (columns first); else of 0, 4, 8
__global__ __launch_bounds__(256) void render_blur_within_kernel(const BlurArgs a) {
  extern __shared__ __align__(16) unsigned char dyn[];
  __shared__ uint32_t pal[256];
  __shared__ unsigned char act[256];
  __shared__ uint32_t taps[MAX_R + 1];
  __shared__ int flag;
  const TileArgs& t = a.t;
  const int tid = (int)threadIdx.x;
  const TilePos p = tile_begin(t, pack_rgb(a.palette + 3 * tid), pal, act, taps, &flag, tid);
  uint32_t* res = (uint32_t*)dyn;                                     // [TH][TW]: the blurred pixel, c0 | c1 << 8 | c2 << 16
  if (flag != 0) {                                                    // (uniform over the block)
    const int R = t.radius, SH = TH + 2 * R, SW = TW + 2 * R;
    uint32_t* s = (uint32_t*)dyn;                                     // [SH][SW]
    uint32_t* hn = (uint32_t*)(dyn + a.src_bytes);                    // [3][hplane]
    const int hplane = kept_sums(TH, TW, R);                          // [SH][TW] rows first, [TH][SW] columns first
    unsigned short* hw = (unsigned short*)(hn + 3 * hplane);
    for (int r = tid >> 7; r < SH; r += 2) {                          // (SW <= 128)
      const int c = tid & 127;
      if (c >= SW) continue;
      const int Y = clampi(p.Y0 - R + r, t.H - 1), X = clampi(p.X0 - R + c, t.W - 1);
      const bool m = act[t.labels[((long)p.f * t.H + Y) * t.W + X]] == 3;
      s[r * SW + c] = m ? source_of<KIND>(a.src, a.ident, p.f, Y, X, t.H, t.W) | 1u << 24 : 0u;
    }
    __syncthreads();
    with_radius_of<CF>(R, [&](auto RR) {
      constexpr int K = decltype(RR)::value;
      if constexpr (K <= ROWS_FIRST_TO) row_pass_rgb<K>(s, SW, hn, hplane, hw, taps, SH, tid);
      else column_pass_rgb<K>(s, hn, hw, taps, tid);
    });
    uint32_t member = 0u;                                             // bit k: the centre of this thread's k-th pixel, tid + 256 k
#pragma unroll
    for (int k = 0; k < TH * TW / 256; ++k) {
      const int i = tid + 256 * k;
      member |= (s[(i / TW + R) * SW + i % TW + R] >> 24) << k;
    }
    __syncthreads();                                                  // (the source plane is dead from here: the results take its place)
    auto fin = [&](int i, const uint32_t* n, uint32_t D) {
      if ((member >> (i >> 8)) & 1u) res[i] = rdiv(n[0], D) | rdiv(n[1], D) << 8 | rdiv(n[2], D) << 16;
    };
    with_radius_of<CF>(R, [&](auto RR) {
      constexpr int K = decltype(RR)::value;
      if constexpr (K <= ROWS_FIRST_TO) column_pass_within<TW, 3, K, uint32_t>(hn, hplane, hw, taps, TH, tid, fin);
      else row_pass_within<TH, TW, 3, K, uint32_t>(hn, hw, taps, tid, fin);
    });
    __syncthreads();
  }
  paint_blur_rgb<KIND, CR>(a, p, pal, act, res, tid);
}

// -> MDQE_OK where the kernel was launched, MDQE_ELAUNCH where the LDS it needs was not granted (nothing is launched then)
template <int KIND>
int launch_within(int contour, dim3 grid, size_t lds, hipStream_t stream, const BlurArgs& a) {
  int st = MDQE_OK;
  with_contour(contour, [&](auto R) {
    if (a.t.radius <= ROWS_FIRST_TO) {                                 // (never above 64 KB)
      hipLaunchKernelGGL((render_blur_within_kernel<KIND, decltype(R)::value, false>), grid, dim3(256), lds, stream, a);
      return;
    }
    auto kern = render_blur_within_kernel<KIND, decltype(R)::value, true>;
    if (lds > LDS_ASK && mdqe_allow_lds(reinterpret_cast<const void*>(kern), (int)lds) != hipSuccess) { st = MDQE_ELAUNCH; return; }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, a);
  });
  return st;
}

// ---- surfaces -----------------------------------------------------------------------------------------------------------------------
// The dynamic LDS of a surface launch, in bytes: the 32-bit planes first (luma Hn, then U and V Hn), then the 16-bit planes: luma source
// and Hw, U and V source and the pairs' Hw, then the results.
struct WithinYuvLds {
  int hny, hnc, sy, hwy, sc, hwc, ry, rc, end;
  __host__ __device__ WithinYuvLds(int R, int Rc) {
    const int SH = TH + 2 * R, SW = TW + 2 * R, CH = CTH + 2 * Rc, CW = CTW + 2 * Rc;
    const int ky = kept_sums(TH, TW, R), kc = kept_sums(CTH, CTW, Rc);
    hny = 0;
    hnc = hny + 4 * ky;
    sy = hnc + 4 * 2 * kc;
    hwy = sy + 2 * SH * SW;
    sc = hwy + 2 * ky;
    hwc = sc + 2 * 2 * CH * CW;
    ry = hwc + 2 * kc;
    rc = ry + 2 * TH * TW;
    end = rc + 2 * 2 * CTH * CTW;
  }
};

template <int FMT, int CR, bool CF>               // CF: as the RGB kernel's, for the LUMA radius; the chroma passes go by their own
__global__ __launch_bounds__(256) void render_blur_within_yuv_kernel(const BlurYuvArgs a) {
  extern __shared__ __align__(16) unsigned char dyn[];
  __shared__ uint32_t pal[256];
  __shared__ unsigned char act[256];
  __shared__ uint32_t taps[MAX_R + 1];
  __shared__ uint32_t taps_c[MAX_RC + 1];
  __shared__ int flag;
  using ACC = typename std::conditional<FMT == 0, uint32_t, uint64_t>::type;   // N of 10-bit values needs more than 32 bits
  const TileArgs& t = a.t;
  const int tid = (int)threadIdx.x;
  load_taps(taps_c, a.taps_c, a.n_taps_c, MAX_RC, tid);
  const TilePos p = tile_begin(t, pack_yuv(a.palette + 3 * tid), pal, act, taps, &flag, tid);
  const unsigned char* yf = a.y + p.f * a.y_stride;                  // the frame's planes
  const unsigned char* cf = a.uv + p.f * a.uv_stride;
  const unsigned char* labf = t.labels + (long)p.f * t.H * t.W;      // the frame's labels
  const WithinYuvLds at(t.radius, a.radius_c);
  const unsigned short* ry = (const unsigned short*)(dyn + at.ry);     // [TH][TW]: blurred luma values
  const unsigned short* rc = (const unsigned short*)(dyn + at.rc);     // [2][CTH][CTW]: blurred U, V of the pairs
  if (flag != 0) {                                                    // (uniform over the block)
    const int R = t.radius, SH = TH + 2 * R, SW = TW + 2 * R;
    const int Rc = a.radius_c, CH = CTH + 2 * Rc, CW = CTW + 2 * Rc;
    const int PH = (t.H + 1) / 2, PW = (t.W + 1) / 2;                 // the chroma plane, in pairs
    unsigned short* sy = (unsigned short*)(dyn + at.sy);
    unsigned short* sc = (unsigned short*)(dyn + at.sc);
    uint32_t* hny = (uint32_t*)(dyn + at.hny);
    uint32_t* hnc = (uint32_t*)(dyn + at.hnc);
    unsigned short* hwy = (unsigned short*)(dyn + at.hwy);
    unsigned short* hwc = (unsigned short*)(dyn + at.hwc);
    unsigned short* wy = (unsigned short*)(dyn + at.ry);
    unsigned short* wc = (unsigned short*)(dyn + at.rc);
    for (int r = tid >> 7; r < SH; r += 2) {                          // (SW <= 128)
      const int c = tid & 127;
      if (c >= SW) continue;
      const int Y = clampi(p.Y0 - R + r, t.H - 1), X = clampi(p.X0 - R + c, t.W - 1);
      const bool m = act[labf[(long)Y * t.W + X]] == 3;
      sy[r * SW + c] = m ? (unsigned short)(value_of<FMT>(row_raw<FMT>(yf + (long)Y * a.y_pitch, X)) | 0x8000u) : (unsigned short)0;
    }
    for (int r = tid >> 6; r < CH; r += 4) {                          // (CW <= 64)
      const int c = tid & 63;
      if (c >= CW) continue;
      const int Y = clampi(p.Y0 / 2 - Rc + r, PH - 1), X = clampi(p.X0 / 2 - Rc + c, PW - 1);
      const unsigned char* l = labf + (long)(2 * Y) * t.W + 2 * X;    // the pair's block: a member when any in-picture pixel is
      const bool down = 2 * Y + 1 < t.H, right = 2 * X + 1 < t.W;
      bool m = act[l[0]] == 3;
      if (right) m |= act[l[1]] == 3;
      if (down) m |= act[l[t.W]] == 3;
      if (down && right) m |= act[l[t.W + 1]] == 3;
      const unsigned char* q = cf + (long)Y * a.uv_pitch;
      sc[r * CW + c] = m ? (unsigned short)(value_of<FMT>(row_raw<FMT>(q, 2 * X)) | 0x8000u) : (unsigned short)0;
      sc[CH * CW + r * CW + c] = m ? (unsigned short)(value_of<FMT>(row_raw<FMT>(q, 2 * X + 1)) | 0x8000u) : (unsigned short)0;
    }
    __syncthreads();
    with_radius_of<CF>(R, [&](auto RR) {
      constexpr int K = decltype(RR)::value;
      if constexpr (K <= ROWS_FIRST_TO) row_pass_yuv<TW, 1, K>(sy, SW, 0, hny, 0, hwy, taps, SH, tid);
      else column_pass_yuv<TH, TW, 1, K>(sy, 0, hny, hwy, taps, tid);
    });
    with_radius(Rc, [&](auto RR) {                                    // (Rc <= 16)
      constexpr int K = decltype(RR)::value > MAX_RC ? MAX_RC : decltype(RR)::value;
      if constexpr (K <= ROWS_FIRST_TO) row_pass_yuv<CTW, 2, K>(sc, CW, CH * CW, hnc, CH * CTW, hwc, taps_c, CH, tid);
      else column_pass_yuv<CTH, CTW, 2, K>(sc, CH * CW, hnc, hwc, taps_c, tid);
    });
    __syncthreads();
    auto fin_y = [&](int i, const ACC* n, uint32_t D) {
      if (sy[(i / TW + R) * SW + i % TW + R] >> 15) wy[i] = (unsigned short)rdiv(n[0], D);
    };
    auto fin_c = [&](int i, const ACC* n, uint32_t D) {
      if (sc[(i / CTW + Rc) * CW + i % CTW + Rc] >> 15) {
        wc[i] = (unsigned short)rdiv(n[0], D);
        wc[CTH * CTW + i] = (unsigned short)rdiv(n[1], D);
      }
    };
    with_radius_of<CF>(R, [&](auto RR) {
      constexpr int K = decltype(RR)::value;
      if constexpr (K <= ROWS_FIRST_TO) column_pass_within<TW, 1, K, ACC>(hny, 0, hwy, taps, TH, tid, fin_y);
      else row_pass_within<TH, TW, 1, K, ACC>(hny, hwy, taps, tid, fin_y);
    });
    with_radius(Rc, [&](auto RR) {
      constexpr int K = decltype(RR)::value > MAX_RC ? MAX_RC : decltype(RR)::value;
      if constexpr (K <= ROWS_FIRST_TO) column_pass_within<CTW, 2, K, ACC>(hnc, CH * CTW, hwc, taps_c, CTH, tid, fin_c);
      else row_pass_within<CTH, CTW, 2, K, ACC>(hnc, hwc, taps_c, tid, fin_c);
    });
    __syncthreads();
  }
  paint_blur_blocks<FMT, CR>(a, p, pal, act, ry, rc, tid);
}

template <int FMT>
int launch_within_yuv(int contour, dim3 grid, size_t lds, hipStream_t stream, const BlurYuvArgs& a) {
  int st = MDQE_OK;
  with_contour(contour, [&](auto R) {
    if (a.t.radius <= ROWS_FIRST_TO) {                                 // (never above 64 KB)
      hipLaunchKernelGGL((render_blur_within_yuv_kernel<FMT, decltype(R)::value, false>), grid, dim3(256), lds, stream, a);
      return;
    }
    auto kern = render_blur_within_yuv_kernel<FMT, decltype(R)::value, true>;
    if (lds > LDS_ASK && mdqe_allow_lds(reinterpret_cast<const void*>(kern), (int)lds) != hipSuccess) { st = MDQE_ELAUNCH; return; }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, stream, a);
  });
  return st;
}

}  // namespace

extern "C" int mdqe_render_blur_within_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                                          const unsigned char* labels, int F, int Ho, int Wo,
                                          const unsigned char* palette, const unsigned char* action, int a256, int contour,
                                          const unsigned short* taps, int radius, unsigned char* out, int f_off, void* stream) {
  BlurArgs a;
  long tiles = 0;
  const int st = blur_rgb_call(frames, frame_stride, h0, w0, labels, F, Ho, Wo, palette, action, a256, contour, taps, radius, out, f_off, a, tiles);
  if (st != MDQE_OK || F == 0) return st;
  a.src_bytes = 4 * (TH + 2 * a.t.radius) * (TW + 2 * a.t.radius);    // (>= 4 * TH * TW)
  const size_t lds = (size_t)a.src_bytes + (size_t)kept_sums(TH, TW, a.t.radius) * (3 * sizeof(uint32_t) + sizeof(unsigned short));     // <= 69632
  mdqe_clear_error();
  const dim3 grid((unsigned)tiles);
  int ls;
  if (frames == nullptr) ls = launch_within<0>(contour, grid, lds, (hipStream_t)stream, a);
  else if (is_u8) ls = launch_within<1>(contour, grid, lds, (hipStream_t)stream, a);
  else ls = launch_within<2>(contour, grid, lds, (hipStream_t)stream, a);
  const int after = mdqe_launch_status();
  return ls != MDQE_OK ? ls : after;
}

extern "C" int mdqe_render_blur_within_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                                int F, int H, int W, int fmt, const unsigned char* labels,
                                                const unsigned short* palette_yuv, const unsigned char* action, int a256, int contour,
                                                const unsigned short* taps, int radius, const unsigned short* taps_c, int radius_c,
                                                void* out_y, long out_y_pitch, long out_y_stride,
                                                void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream) {
  BlurYuvArgs a;
  long tiles = 0;
  const int st = blur_yuv_call(y, y_pitch, y_stride, uv, uv_pitch, uv_stride, F, H, W, fmt, labels, palette_yuv, action, a256, contour, taps, radius,
                               taps_c, radius_c, out_y, out_y_pitch, out_y_stride, out_uv, out_uv_pitch, out_uv_stride, f_off, a, tiles);
  if (st != MDQE_OK || F == 0) return st;
  const size_t lds = (size_t)WithinYuvLds(a.t.radius, a.radius_c).end;                       // <= 51200
  mdqe_clear_error();
  const dim3 grid((unsigned)tiles);
  const int ls = fmt == 0 ? launch_within_yuv<0>(contour, grid, lds, (hipStream_t)stream, a)
                          : launch_within_yuv<1>(contour, grid, lds, (hipStream_t)stream, a);
  const int after = mdqe_launch_status();
  return ls != MDQE_OK ? ls : after;
}
