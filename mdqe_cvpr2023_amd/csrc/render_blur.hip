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
//   5 paint   the painters of render.hip and render_yuv.hip with the action selecting the value, as render_mosaic.hip's: RGB in groups
//             of 4 pixels laid out from the OUTPUT address (three aligned dword stores per group; a group cut by the tile's side stores
//             bytes); surfaces one 2 x 2 block per thread, single samples at any alignment.
// Why 16 x 64: the LDS is sized per launch from the radius (dynamic LDS: 3 (16 + 2R)(64 + 2R) bytes of source and 6 (16 + 2R) 64 of
// rows for RGB -- 61440 bytes at R = 32, 19.5 KB at R = 8), and at R = 32 this is the largest tile of 64 columns that stays under 64 KB
// with all three channels resident, so the source is converted (float32 frames) and sampled once per halo pixel.  The price is read
// amplification at large radii: (16 + 2R)(64 + 2R) / 1024 source values per output pixel, 10 at R = 32, served by L2.  The three
// channels are NOT packed into one register: a row sum reaches 2^20 and a column sum 2^26, more than a 16-bit lane half holds.  The taps
// live in LDS as dwords (they are uniform).  Both passes run over the whole tile of a flagged tile, whatever the labels: no
// data-dependent order, no atomics anywhere, identical from run to run.  The rule's pieces (source pixel, tints, sample helpers, contour
// test and dispatch) and the entries' checks are render_rule.h's, shared with the other painters; the tile scheme (the tile's position, the
// flag phase, the padded radii) is render_blur_tile.h's, shared with render_blur_within.hip, the blur that stops at region borders.
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
struct BlurArgs {
  TileArgs t;
  RgbSource src;
  const unsigned char* palette;  // [256, 3]
  unsigned char* out;            // at frame f_off already: [F, Ho, Wo, 3]
  unsigned head;                 // out address mod 4: groups of 4 pixels start at flat pixels = head (mod 4)
  int ident;
  int items;                     // paint items (groups of 4 pixels) per tile row
  uint32_t m_items;
  int pitch;                     // bytes between the rows of a source plane in LDS: 64 + 2R
  int src_bytes;                 // the source planes' share of the dynamic LDS (>= 4 * TH * TW: the result plane takes its place)
};

// the source pixel of output pixel (f, Y, X)
template <int KIND>
__device__ __forceinline__ uint32_t source_of(const BlurArgs& a, int f, int Y, int X) {
  return source_px<KIND>(a.src, a.ident, (long)f * a.src.frame_stride, Y, X, a.t.H, a.t.W);
}

template <int KIND, int CR>
__global__ __launch_bounds__(256) void render_blur_kernel(const BlurArgs a) {
  extern __shared__ __align__(16) unsigned char dyn[];
  __shared__ uint32_t pal[256];
  __shared__ unsigned char act[256];
  __shared__ uint32_t taps[MAX_R + 1];
  __shared__ int flag;
  const TileArgs& t = a.t;
  const int tid = (int)threadIdx.x;
  pal[tid] = pack_rgb(a.palette + 3 * tid);
  act[tid] = t.action[tid];
  if (tid <= MAX_R) taps[tid] = tid < t.n_taps ? (uint32_t)t.taps[tid] : 0u;
  if (tid == 0) flag = 0;
  __syncthreads();
  const TilePos p = tile_pos(t);
  flag_tile(t, p, act, &flag, tid);
  __syncthreads();
  const uint32_t* res = (const uint32_t*)dyn;                          // [TH][TW]: the blurred pixel, c0 | c1 << 8 | c2 << 16 (bits 24.. unused)
  if (flag != 0) {                                                    // (uniform over the block)
    const int R = t.radius, SH = TH + 2 * R, SW = TW + 2 * R, plane = SH * a.pitch;
    unsigned char* s = dyn;                                           // [3][SH][pitch]
    unsigned short* h = (unsigned short*)(dyn + a.src_bytes);         // [3][SH][TW]
    for (int r = tid >> 7; r < SH; r += 2) {                          // (SW <= 128)
      const int c = tid & 127;
      if (c >= SW) continue;
      const uint32_t px = source_of<KIND>(a, p.f, clampi(p.Y0 - R + r, t.H - 1), clampi(p.X0 - R + c, t.W - 1));
      unsigned char* q = s + r * a.pitch + c;
      q[0] = (unsigned char)px; q[plane] = (unsigned char)(px >> 8); q[2 * plane] = (unsigned char)(px >> 16);
    }
    __syncthreads();
    with_radius(R, [&](auto RR) { row_pass<TW, 3, decltype(RR)::value>(s, a.pitch, plane, h, SH * TW, taps, SH, tid); });
    __syncthreads();
    with_radius(R, [&](auto RR) {
      column_pass<TW, 3, decltype(RR)::value>(h, SH * TW, taps, TH, tid, [&](int i, int k, uint32_t v) { dyn[4 * i + k] = (unsigned char)v; });
    });
    __syncthreads();
  }
  // paint: item j of tile row r is the j-th group of 4 flat pixels that meets the row's segment
  for (int it = tid; it < p.th * a.items; it += 256) {
    const int r = mdiv(it, a.m_items), j = it - r * a.items;
    const int Y = p.Y0 + r;
    const long row = ((long)p.f * t.H + Y) * t.W;                    // flat pixel of (f, Y, 0), < 2^31
    const long seg = row + p.X0;                                      // the segment: flat pixels [seg, seg + tw)
    const long ps = 4 * ((seg + 4 - a.head) / 4 + j) + a.head - 4;    // the group's first flat pixel (may lie before seg)
    const long lo = ps > seg ? ps : seg, hi = ps + 4 < seg + p.tw ? ps + 4 : seg + p.tw;
    if (lo >= hi) continue;
    const bool whole = hi - lo == 4;
    uint32_t l4 = 0u, c0 = 0u, c1 = 0u, c2 = 0u;
    const bool wide_src = KIND == 1 && whole && a.ident;
    if (whole) l4 = ld4(t.labels + ps);
    if (wide_src) {
      const unsigned char* q = (const unsigned char*)a.src.frames + (long)p.f * a.src.frame_stride + (long)Y * a.src.w0 + (int)(ps - row);
      c0 = ld4(q); c1 = ld4(q + a.src.plane); c2 = ld4(q + 2 * a.src.plane);
    }
    uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long q = ps + k;
      if (q < lo || q >= hi) continue;
      const int X = (int)(q - row);
      const uint32_t l = whole ? (l4 >> 8 * k) & 0xFFu : (uint32_t)t.labels[q];
      const uint32_t ac = act[l];
      if (ac == 3u) {
        px[k] = res[r * TW + (X - p.X0)] & 0x00FFFFFFu;
        continue;
      }
      const uint32_t s = wide_src ? ((c0 >> 8 * k) & 0xFFu) | ((c1 >> 8 * k) & 0xFFu) << 8 | ((c2 >> 8 * k) & 0xFFu) << 16
                                  : source_of<KIND>(a, p.f, Y, X);
      px[k] = ac != 1u ? s : tint(s, pal[l], edge_at<CR>(t.labels + q, l, Y, X, t.H, t.W), t.a256);
    }
    unsigned char* o = a.out + 3L * ps;
    if (whole) {
      uint32_t* o4 = (uint32_t*)o;                                    // 4-byte aligned by the groups' layout
      o4[0] = px[0] | px[1] << 24;
      o4[1] = px[1] >> 8 | px[2] << 16;
      o4[2] = px[2] >> 16 | px[3] << 8;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (ps + k >= lo && ps + k < hi) {
          o[3 * k] = (unsigned char)px[k]; o[3 * k + 1] = (unsigned char)(px[k] >> 8); o[3 * k + 2] = (unsigned char)(px[k] >> 16);
        }
    }
  }
}

template <int KIND>
void launch_blur(int contour, dim3 grid, size_t lds, hipStream_t stream, const BlurArgs& a) {
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_blur_kernel<KIND, decltype(R)::value>), grid, dim3(256), lds, stream, a);
  });
}

// ---- surfaces -----------------------------------------------------------------------------------------------------------------------
constexpr int CTH = TH / 2, CTW = TW / 2;        // the chroma tile: the pairs under the luma tile

struct BlurYuvArgs {
  TileArgs t;
  const unsigned short* taps_c;                  // [n_taps_c]
  int n_taps_c, radius_c;                        // (as TileArgs' n_taps and radius)
  const unsigned char* y;
  const unsigned char* uv;
  const unsigned short* palette;                 // [256, 3]: Y, U, V in sample units
  unsigned char* oy;                             // at frame f_off already
  unsigned char* ouv;
  long y_pitch, y_stride, uv_pitch, uv_stride;   // bytes
  long oy_pitch, oy_stride, ouv_pitch, ouv_stride;
};

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
  pal[tid] = pack_yuv(a.palette + 3 * tid);
  act[tid] = t.action[tid];
  if (tid <= MAX_R) taps[tid] = tid < t.n_taps ? (uint32_t)t.taps[tid] : 0u;
  if (tid <= MAX_RC) taps_c[tid] = tid < a.n_taps_c ? (uint32_t)a.taps_c[tid] : 0u;
  if (tid == 0) flag = 0;
  __syncthreads();
  const TilePos p = tile_pos(t);
  constexpr int BPS = FMT ? 2 : 1;                                   // bytes per sample
  const unsigned char* yf = a.y + p.f * a.y_stride;                  // the frame's planes
  const unsigned char* cf = a.uv + p.f * a.uv_stride;
  const unsigned char* y0 = yf + (long)p.Y0 * a.y_pitch + (long)p.X0 * BPS;               // sample (Y0, X0)
  const unsigned char* c0p = cf + (long)(p.Y0 / 2) * a.uv_pitch + (long)p.X0 * BPS;       // pair (Y0 / 2, X0 / 2)
  unsigned char* oy0 = a.oy + p.f * a.oy_stride + (long)p.Y0 * a.oy_pitch + (long)p.X0 * BPS;
  unsigned char* oc0 = a.ouv + p.f * a.ouv_stride + (long)(p.Y0 / 2) * a.ouv_pitch + (long)p.X0 * BPS;
  const unsigned char* lab0 = t.labels + ((long)p.f * t.H + p.Y0) * t.W + p.X0;
  flag_tile(t, p, act, &flag, tid);
  __syncthreads();
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
  // paint: item j of row pair rp is the 2 x 2 block at column 2 * j of the tile
  const int chr = (p.th + 1) / 2;
  for (int it = tid; it < chr * CTW; it += 256) {
    const int rp = it / CTW, j = it % CTW;
    const int cb = 2 * j;                                             // column inside the tile
    if (cb >= p.tw) continue;
    const int r0 = p.Y0 + 2 * rp, c0 = p.X0 + cb;
    const int nr = r0 + 1 < t.H ? 2 : 1, nc = c0 + 1 < t.W ? 2 : 1;
    const unsigned char* yrow = y0 + (long)(2 * rp) * a.y_pitch;
    const unsigned char* crow = c0p + (long)rp * a.uv_pitch;
    unsigned char* oyrow = oy0 + (long)(2 * rp) * a.oy_pitch;
    unsigned char* ocrow = oc0 + (long)rp * a.ouv_pitch;
    const unsigned char* lab = lab0 + (long)(2 * rp) * t.W + cb;
    const uint32_t ru = row_raw<FMT>(crow, cb), rv = row_raw<FMT>(crow, cb + 1);
    const uint32_t U = value_of<FMT>(ru), V = value_of<FMT>(rv);
    uint32_t su = 0u, sv = 0u;
    bool kept = true;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (row >= nr || k >= nc) continue;
        const unsigned char* q = lab + (long)row * t.W + k;
        const uint32_t l = q[0], ac = act[l];
        const uint32_t raw = row_raw<FMT>(yrow + (long)row * a.y_pitch, cb + k);
        uint32_t o = raw;
        if (ac == 3u) {                                               // (only in a flagged tile)
          o = stored<FMT>((uint32_t)ry[(2 * rp + row) * TW + cb + k]);
          su += rc[rp * CTW + j]; sv += rc[CTH * CTW + rp * CTW + j];
          kept = false;
        } else if (ac == 1u) {
          const bool edge = edge_at<CR>(q, l, r0 + row, c0 + k, t.H, t.W);
          const uint32_t col = pal[l];
          o = stored<FMT>(tint1(value_of<FMT>(raw), comp<FMT>(col, 0), edge, t.a256));
          su += tint1(U, comp<FMT>(col, 1), edge, t.a256);
          sv += tint1(V, comp<FMT>(col, 2), edge, t.a256);
          kept = false;
        } else {
          su += U; sv += V;
        }
        row_put<FMT>(oyrow + (long)row * a.oy_pitch, cb + k, o);
      }
    }
    const uint32_t sh = (uint32_t)(nr * nc) >> 1;                       // n = 1, 2, 4: n / 2 = log2(n) = 0, 1, 2
    row_put<FMT>(ocrow, cb, kept ? ru : stored<FMT>((su + sh) >> sh));
    row_put<FMT>(ocrow, cb + 1, kept ? rv : stored<FMT>((sv + sh) >> sh));
  }
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
  MDQE_REQUIRE(radius >= 0 && radius <= MAX_R);
  BlurArgs a;
  const int st = rgb_call(frames, frame_stride, h0, w0, labels, F, Ho, Wo, palette, action, true, a256, contour, out, f_off, a.src, a.ident, a.out);
  if (st != MDQE_OK || F == 0) return st;
  MDQE_CHECK_PTR(taps);
  MDQE_REQUIRE(((uintptr_t)taps & 1u) == 0);
  const long tiles = tile_args(a.t, labels, action, taps, radius, F, Ho, Wo, a256);
  a.palette = palette;
  a.head = (unsigned)((uintptr_t)a.out & 3u);
  // a segment of TW pixels meets at most TW / 4 + 1 groups; exactly TW / 4 where every segment starts a group (Wo is a multiple of 4
  // and so is the output address)
  a.items = TW / 4 + ((Wo & 3) == 0 && a.head == 0 ? 0 : 1);
  a.m_items = magic(a.items);
  const int SH = TH + 2 * a.t.radius;
  a.pitch = TW + 2 * a.t.radius;                                      // (a multiple of 4)
  a.src_bytes = 3 * SH * a.pitch > 4 * TH * TW ? 3 * SH * a.pitch : 4 * TH * TW;
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
  MDQE_REQUIRE(radius >= 0 && radius <= MAX_R && radius_c >= 0 && radius_c <= MAX_RC);
  // not in place: the taps read samples that other threads write
  SurfaceOut o;
  const int st = surface_call(y, y_pitch, y_stride, uv, uv_pitch, uv_stride, F, H, W, fmt, labels, palette_yuv, action, true, false, a256,
                              contour, out_y, out_y_pitch, out_y_stride, out_uv, out_uv_pitch, out_uv_stride, f_off, o);
  if (st != MDQE_OK || F == 0) return st;
  MDQE_CHECK_PTR(taps);
  MDQE_CHECK_PTR(taps_c);
  MDQE_REQUIRE((((uintptr_t)taps | (uintptr_t)taps_c) & 1u) == 0);
  {
    // the overlap refusals of surface_call, for the two tap tables
    const long bps = fmt ? 2 : 1, yb = bps * W, cb = bps * 2 * ((W + 1L) / 2), CH = (H + 1L) / 2;
    const Plane ty = plane_of(o.oy, out_y_pitch, out_y_stride, F, H, yb), tc = plane_of(o.ouv, out_uv_pitch, out_uv_stride, F, CH, cb);
    const Plane s1 = plane_of(taps, 2L * (radius + 1), 0, 1, 1, 2L * (radius + 1));
    const Plane s2 = plane_of(taps_c, 2L * (radius_c + 1), 0, 1, 1, 2L * (radius_c + 1));
    MDQE_REQUIRE(apart(s1, ty) && apart(s1, tc) && apart(s2, ty) && apart(s2, tc));
  }
  BlurYuvArgs a;
  const long tiles = tile_args(a.t, labels, action, taps, radius, F, H, W, a256);
  a.taps_c = taps_c;
  a.n_taps_c = radius_c + 1;
  a.radius_c = padded(radius_c);
  a.y = (const unsigned char*)y;
  a.uv = (const unsigned char*)uv;
  a.palette = palette_yuv;
  a.oy = o.oy;
  a.ouv = o.ouv;
  a.y_pitch = y_pitch; a.y_stride = y_stride; a.uv_pitch = uv_pitch; a.uv_stride = uv_stride;
  a.oy_pitch = out_y_pitch; a.oy_stride = out_y_stride; a.ouv_pitch = out_uv_pitch; a.ouv_stride = out_uv_stride;
  const size_t lds = (size_t)YuvLds(a.t.radius, a.radius_c).end * sizeof(unsigned short);       // <= 49152
  mdqe_clear_error();
  const dim3 grid((unsigned)tiles);
  if (fmt == 0) launch_by<0>(contour, grid, lds, (hipStream_t)stream, a);
  else launch_by<1>(contour, grid, lds, (hipStream_t)stream, a);
  return mdqe_launch_status();
}
