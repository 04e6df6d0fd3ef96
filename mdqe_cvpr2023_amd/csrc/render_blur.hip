// The blur overlay: a label map painted with a PER-LABEL action -- keep the source, tint it as render.hip / render_yuv.hip do, or replace it
// by a separable Gaussian blur of the picture (action 3, a redaction blur).  ONE definition, integers only (include/mdqe_hip.h has the
// rule); tests/_blur_ref.py restates it in numpy and every comparison is exact.
//
// A blurred pixel needs its neighbours up to `radius` away, so a thread block owns a TILE of 16 x 64 output pixels of one frame plus a
// halo: 256 threads, phases between barriers:
//   1 flag    every label of the tile is read once; a pixel whose action is 3 sets the tile's LDS flag (a plain store of 1).  A tile
//             that flags nothing goes straight to the paint phase: its source is read once, with no halo;
//   2 load    a flagged tile loads (16 + 2R) x (64 + 2R) source values, coordinates clamped to the picture (the border is replicated),
//             through source_px (RGB: three byte planes in LDS; surfaces: luma, U and V as 16-bit planes, the chroma tile being the
//             8 x 32 pairs under the luma tile with its own radius and clamped to its own plane);
//   3 rows    the horizontal pass, one position of all planes per thread and step, into 16-bit LDS planes of (16 + 2R) x 64:
//             h = (sum + 128) >> 8 is at most 16368.  The two taps of a distance share one multiply (s[-d] + s[d] first).  The kernel's
//             R is the table's radius rounded up to one of 0, 4, 8, 16, 24, 32 with zero taps beyond it, and the tap loops are
//             unrolled for that R: the passes wait on LDS latency, and loads in flight are what hides it;
//   4 columns the vertical pass over those planes, (sum + 32768) >> 16, into the tile's result plane in LDS (RGB: one packed dword per
//             pixel, which takes the place of the dead source planes);
//   5 paint   the painters of render.hip and render_yuv.hip with the action selecting the value: RGB in groups of 4 pixels laid out from
//             the OUTPUT address (paint_rgb_tile: three aligned dword stores per group; a group cut by the tile's side stores bytes);
//             surfaces one 2 x 2 block per thread, single samples at any alignment (paint_blur_blocks).
// Why 16 x 64: the LDS is sized per launch from the radius (dynamic LDS: 3 (16 + 2R)(64 + 2R) bytes of source and 6 (16 + 2R) 64 of
// rows for RGB -- 61440 bytes at R = 32, 19.5 KB at R = 8), and at R = 32 this is the largest tile of 64 columns that stays under 64 KB
// with all three channels resident, so the source is converted (float32 frames) and sampled once per halo pixel.  The price is read
// amplification at large radii: (16 + 2R)(64 + 2R) / 1024 source values per output pixel, 10 at R = 32, served by L2.  The three
// channels are NOT packed into one register: a row sum reaches 2^20 and a column sum 2^26, more than a 16-bit lane half holds.  The taps
// live in LDS as dwords (they are uniform).  Both passes run over the whole tile of a flagged tile, whatever the labels: no
// data-dependent order, no atomics anywhere, identical from run to run.  This file holds what is the plain blur's own: the two passes, the
// LDS plans, the load phases and the launches.  The rule's pieces (source pixel, tints, sample helpers, contour test and dispatch) are
// render_rule.h's, shared with the other painters; the RGB paint phase is render_tile_paint.h's, shared with the mosaic; the tile scheme
// (the tile's position, phase 1 with the tables' load, the padded radii), the argument structs with the entries' checks and the surface
// paint phase are render_blur_tile.h's, shared with render_blur_within.hip, the blur that stops at region borders.
#include "render_blur_tile.h"

namespace {

// phase 3: h[r][c] = (sum_d taps[|d|] * src[r][c + R + d] + 128) >> 8 for `rows` rows of COLS columns of NP planes at once; src rows
// are `pitch` samples apart and hold COLS + 2R samples, planes `splane` (src) and `hplane` (h) samples apart.
// taps[d] * (s[-d] + s[d]) <= 4096 * 2046 and the sum <= 4096 * 1023: 32 bits hold both.
template <int COLS, int NP, int R, class T>
__device__ __forceinline__ void row_pass(const T* src, int pitch, int splane, unsigned short* h, int hplane, const uint32_t* taps,
                                         int rows, int tid) {
  for (int i = tid; i < rows * COLS; i += 256) {
    const int r = i / COLS, c = i % COLS;
    const T* q = src + r * pitch + c + R;
    uint32_t acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = taps[0] * (uint32_t)q[p * splane];
#pragma unroll
    for (int d = 1; d <= R; ++d) {
      const uint32_t w = taps[d];
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p] += w * ((uint32_t)q[p * splane - d] + (uint32_t)q[p * splane + d]);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) h[p * hplane + i] = (unsigned short)((acc[p] + 128u) >> 8);
  }
}

// phase 4: put(i, p, (sum_d taps[|d|] * h[r + R + d][c] + 32768) >> 16) for i = r * COLS + c over `rows` rows of plane p; h holds
// rows + 2R rows per plane.  h <= 16368: taps[d] * (h[-d] + h[d]) < 2^27 and the sum < 2^26.
template <int COLS, int NP, int R, class Put>
__device__ __forceinline__ void column_pass(const unsigned short* h, int hplane, const uint32_t* taps, int rows, int tid, Put put) {
  for (int i = tid; i < rows * COLS; i += 256) {
    const unsigned short* q = h + i + R * COLS;
    uint32_t acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = taps[0] * (uint32_t)q[p * hplane];
#pragma unroll
    for (int d = 1; d <= R; ++d) {
      const uint32_t w = taps[d];
#pragma unroll
      for (int p = 0; p < NP; ++p) acc[p] += w * ((uint32_t)q[p * hplane - d * COLS] + (uint32_t)q[p * hplane + d * COLS]);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) put(i, p, (acc[p] + 32768u) >> 16);
  }
}

// ---- RGB ----------------------------------------------------------------------------------------------------------------------------
template <int KIND, int CR>
__global__ __launch_bounds__(256) void render_blur_kernel(const BlurArgs a) {
  extern __shared__ __align__(16) unsigned char dyn[];
  __shared__ uint32_t pal[256];
  __shared__ unsigned char act[256];
  __shared__ uint32_t taps[MAX_R + 1];
  __shared__ int flag;
  const TileArgs& t = a.t;
  const int tid = (int)threadIdx.x;
  const TilePos p = tile_begin(t, pack_rgb(a.palette + 3 * tid), pal, act, taps, &flag, tid);
  const uint32_t* res = (const uint32_t*)dyn;                          // [TH][TW]: the blurred pixel, c0 | c1 << 8 | c2 << 16 (bits 24.. unused)
  if (flag != 0) {                                                    // (uniform over the block)
    const int R = t.radius, SH = TH + 2 * R, SW = TW + 2 * R, plane = SH * SW;
    unsigned char* s = dyn;                                           // [3][SH][SW]
    unsigned short* h = (unsigned short*)(dyn + a.src_bytes);         // [3][SH][TW]
    for (int r = tid >> 7; r < SH; r += 2) {                          // (SW <= 128)
      const int c = tid & 127;
      if (c >= SW) continue;
      const uint32_t px = source_of<KIND>(a.src, a.ident, p.f, clampi(p.Y0 - R + r, t.H - 1), clampi(p.X0 - R + c, t.W - 1), t.H, t.W);
      unsigned char* q = s + r * SW + c;
      q[0] = (unsigned char)px; q[plane] = (unsigned char)(px >> 8); q[2 * plane] = (unsigned char)(px >> 16);
    }
    __syncthreads();
    with_radius(R, [&](auto RR) { row_pass<TW, 3, decltype(RR)::value>(s, SW, plane, h, SH * TW, taps, SH, tid); });
    __syncthreads();
    with_radius(R, [&](auto RR) {
      column_pass<TW, 3, decltype(RR)::value>(h, SH * TW, taps, TH, tid, [&](int i, int k, uint32_t v) { dyn[4 * i + k] = (unsigned char)v; });
    });
    __syncthreads();
  }
  paint_blur_rgb<KIND, CR>(a, p, pal, act, res, tid);
}

template <int KIND>
void launch_blur(int contour, dim3 grid, size_t lds, hipStream_t stream, const BlurArgs& a) {
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_blur_kernel<KIND, decltype(R)::value>), grid, dim3(256), lds, stream, a);
  });
}

// ---- surfaces -----------------------------------------------------------------------------------------------------------------------
// The dynamic LDS of a surface launch, in 16-bit samples: luma source and rows, U and V source and rows, then the results.
struct YuvLds {
  int sy, hy, sc, hc, ry, rc, end;
  __host__ __device__ YuvLds(int R, int Rc) {
    const int SH = TH + 2 * R, SW = TW + 2 * R, CH = CTH + 2 * Rc, CW = CTW + 2 * Rc;
    sy = 0;
    hy = sy + SH * SW;
    sc = hy + SH * TW;
    hc = sc + 2 * CH * CW;
    ry = hc + 2 * CH * CTW;
    rc = ry + TH * TW;
    end = rc + 2 * CTH * CTW;
  }
};

template <int FMT, int CR>
__global__ __launch_bounds__(256) void render_blur_yuv_kernel(const BlurYuvArgs a) {
  extern __shared__ __align__(16) unsigned char dyn[];
  __shared__ uint32_t pal[256];
  __shared__ unsigned char act[256];
  __shared__ uint32_t taps[MAX_R + 1];
  __shared__ uint32_t taps_c[MAX_RC + 1];
  __shared__ int flag;
  const TileArgs& t = a.t;
  const int tid = (int)threadIdx.x;
  load_taps(taps_c, a.taps_c, a.n_taps_c, MAX_RC, tid);
  const TilePos p = tile_begin(t, pack_yuv(a.palette + 3 * tid), pal, act, taps, &flag, tid);
  const unsigned char* yf = a.y + p.f * a.y_stride;                  // the frame's planes
  const unsigned char* cf = a.uv + p.f * a.uv_stride;
  const YuvLds at(t.radius, a.radius_c);
  unsigned short* lds = (unsigned short*)dyn;
  const unsigned short* ry = lds + at.ry;                              // [TH][TW]: blurred luma values
  const unsigned short* rc = lds + at.rc;                              // [2][CTH][CTW]: blurred U, V of the pairs
  if (flag != 0) {                                                    // (uniform over the block)
    const int R = t.radius, SH = TH + 2 * R, SW = TW + 2 * R;
    const int Rc = a.radius_c, CH = CTH + 2 * Rc, CW = CTW + 2 * Rc;
    const int PH = (t.H + 1) / 2, PW = (t.W + 1) / 2;                 // the chroma plane, in pairs
    for (int r = tid >> 7; r < SH; r += 2) {                          // (SW <= 128)
      const int c = tid & 127;
      if (c >= SW) continue;
      const int Y = clampi(p.Y0 - R + r, t.H - 1), X = clampi(p.X0 - R + c, t.W - 1);
      lds[at.sy + r * SW + c] = (unsigned short)value_of<FMT>(row_raw<FMT>(yf + (long)Y * a.y_pitch, X));
    }
    for (int r = tid >> 6; r < CH; r += 4) {                          // (CW <= 64)
      const int c = tid & 63;
      if (c >= CW) continue;
      const int Y = clampi(p.Y0 / 2 - Rc + r, PH - 1), X = clampi(p.X0 / 2 - Rc + c, PW - 1);
      const unsigned char* q = cf + (long)Y * a.uv_pitch;
      lds[at.sc + r * CW + c] = (unsigned short)value_of<FMT>(row_raw<FMT>(q, 2 * X));
      lds[at.sc + CH * CW + r * CW + c] = (unsigned short)value_of<FMT>(row_raw<FMT>(q, 2 * X + 1));
    }
    __syncthreads();
    with_radius(R, [&](auto RR) { row_pass<TW, 1, decltype(RR)::value>(lds + at.sy, SW, 0, lds + at.hy, 0, taps, SH, tid); });
    with_radius(Rc, [&](auto RR) {                                    // (Rc <= 16)
      row_pass<CTW, 2, (decltype(RR)::value > MAX_RC ? MAX_RC : decltype(RR)::value)>(lds + at.sc, CW, CH * CW, lds + at.hc, CH * CTW, taps_c, CH, tid);
    });
    __syncthreads();
    with_radius(R, [&](auto RR) {
      column_pass<TW, 1, decltype(RR)::value>(lds + at.hy, 0, taps, TH, tid, [&](int i, int, uint32_t v) { lds[at.ry + i] = (unsigned short)v; });
    });
    with_radius(Rc, [&](auto RR) {
      column_pass<CTW, 2, (decltype(RR)::value > MAX_RC ? MAX_RC : decltype(RR)::value)>(
          lds + at.hc, CH * CTW, taps_c, CTH, tid, [&](int i, int k, uint32_t v) { lds[at.rc + k * CTH * CTW + i] = (unsigned short)v; });
    });
    __syncthreads();
  }
  paint_blur_blocks<FMT, CR>(a, p, pal, act, ry, rc, tid);
}

template <int FMT>
void launch_by(int contour, dim3 grid, size_t lds, hipStream_t stream, const BlurYuvArgs& a) {
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_blur_yuv_kernel<FMT, decltype(R)::value>), grid, dim3(256), lds, stream, a);
  });
}

}  // namespace

extern "C" int mdqe_render_blur_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                                   const unsigned char* labels, int F, int Ho, int Wo,
                                   const unsigned char* palette, const unsigned char* action, int a256, int contour,
                                   const unsigned short* taps, int radius, unsigned char* out, int f_off, void* stream) {
  BlurArgs a;
  long tiles = 0;
  const int st = blur_rgb_call(frames, frame_stride, h0, w0, labels, F, Ho, Wo, palette, action, a256, contour, taps, radius, out, f_off, a, tiles);
  if (st != MDQE_OK || F == 0) return st;
  const int SH = TH + 2 * a.t.radius, SW = TW + 2 * a.t.radius;       // (SW: a multiple of 4)
  a.src_bytes = 3 * SH * SW > 4 * TH * TW ? 3 * SH * SW : 4 * TH * TW;
  const size_t lds = (size_t)a.src_bytes + (size_t)(3 * SH * TW) * sizeof(unsigned short);     // <= 61440
  mdqe_clear_error();
  const dim3 grid((unsigned)tiles);
  if (frames == nullptr) launch_blur<0>(contour, grid, lds, (hipStream_t)stream, a);
  else if (is_u8) launch_blur<1>(contour, grid, lds, (hipStream_t)stream, a);
  else launch_blur<2>(contour, grid, lds, (hipStream_t)stream, a);
  return mdqe_launch_status();
}

extern "C" int mdqe_render_blur_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
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
  const size_t lds = (size_t)YuvLds(a.t.radius, a.radius_c).end * sizeof(unsigned short);       // <= 49152
  mdqe_clear_error();
  const dim3 grid((unsigned)tiles);
  if (fmt == 0) launch_by<0>(contour, grid, lds, (hipStream_t)stream, a);
  else launch_by<1>(contour, grid, lds, (hipStream_t)stream, a);
  return mdqe_launch_status();
}
