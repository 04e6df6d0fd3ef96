// The tile scheme of the two blur painters, said once: what render_blur.hip (the plain Gaussian) and render_blur_within.hip (the
// edge-stopping one) share.  A thread block of 256 threads owns a tile of 16 x 64 output pixels of one frame; a tile is filtered only
// when one of its pixels has action 3; the tap loops are compiled once per padded radius.  Here: the tile's position and the flag phase,
// the kernels' first phase (`tile_begin`), the argument structs of the RGB and of the surface kernels with the entries' checks that fill
// them (`blur_rgb_call`, `blur_yuv_call`), and the surface paint phase (`paint_blur_blocks`); the RGB paint phase is
// render_tile_paint.h's, shared with the mosaic.  The kernels, their LDS plans, their passes and their launches stay in the two .hip files.
#pragma once
#include "render_tile_paint.h"

namespace {

constexpr int TH = 16, TW = 64;                  // the tile, in output pixels
constexpr int CTH = TH / 2, CTW = TW / 2;        // a surface's chroma tile: the pairs under the luma tile
constexpr int MAX_R = 32, MAX_RC = 16;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

struct TileArgs {
  const unsigned char* labels;   // [F, H, W]
  const unsigned char* action;   // [256]
  const unsigned short* taps;    // [n_taps]
  int n_taps;                    // the table's radius + 1
  int radius;                    // the kernel's radius: `padded` (the table's rounded up), the taps beyond the table's 0
  int H, W;
  unsigned tiles_x, tiles_y;
  uint32_t a256;
};

__device__ __forceinline__ TilePos tile_pos(const TileArgs& a) {
  unsigned b = blockIdx.x;
  const unsigned tx = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned ty = b % a.tiles_y;
  TilePos p;
  p.f = (int)(b / a.tiles_y);
  p.Y0 = (int)ty * TH;
  p.X0 = (int)tx * TW;
  p.th = a.H - p.Y0 < TH ? a.H - p.Y0 : TH;
  p.tw = a.W - p.X0 < TW ? a.W - p.X0 : TW;
  return p;
}

// phase 1: *flag = 1 where a pixel of the tile has action 3 (between the caller's barriers; *flag was zeroed before the first)
__device__ __forceinline__ void flag_tile(const TileArgs& a, const TilePos& p, const unsigned char* act, int* flag, int tid) {
  const unsigned char* lab0 = a.labels + ((long)p.f * a.H + p.Y0) * a.W + p.X0;
  for (int i = tid; i < p.th * TW; i += 256) {
    const int r = i / TW, c = i % TW;
    if (c < p.tw && act[lab0[(long)r * a.W + c]] == 3) *flag = 1;
  }
}

// thread tid's share of a tap table in LDS: max_r + 1 dwords, zero beyond the table's n taps (before a barrier)
__device__ __forceinline__ void load_taps(uint32_t* lds, const unsigned short* taps, int n, int max_r, int tid) {
  if (tid <= max_r) lds[tid] = tid < n ? (uint32_t)taps[tid] : 0u;
}

// A kernel's first phase: the palette (thread tid's row, packed by the caller: pack_rgb or pack_yuv), the action table and the taps go
// to LDS and the tile is flagged, with the barriers before and after.  -> the tile's position; *flag says whether the tile is filtered.
__device__ __forceinline__ TilePos tile_begin(const TileArgs& t, uint32_t pal_row, uint32_t* pal, unsigned char* act, uint32_t* taps,
                                              int* flag, int tid) {
  pal[tid] = pal_row;
  act[tid] = t.action[tid];
  load_taps(taps, t.taps, t.n_taps, MAX_R, tid);
  if (tid == 0) *flag = 0;
  __syncthreads();
  const TilePos p = tile_pos(t);
  flag_tile(t, p, act, flag, tid);
  __syncthreads();
  return p;
}

// The radius a launch runs with: the table's rounded up to the next of 0, 4, 8, 16, 24, 32, with zero taps beyond the table's.  The
// passes are compiled once per such radius with their tap loops fully unrolled (`with_radius`): they wait on LDS latency, and only
// many independent loads in flight hide it (measured: a loop of 4 distances per step ran 2.8 times as long at radius 32).
int padded(int r) { return r == 0 ? 0 : r <= 4 ? 4 : r <= 8 ? 8 : (r + 7) & ~7; }

template <class Fn>
__device__ __forceinline__ void with_radius(int R, Fn&& fn) {
  switch (R) {
    case 0: fn(std::integral_constant<int, 0>()); break;
    case 4: fn(std::integral_constant<int, 4>()); break;
    case 8: fn(std::integral_constant<int, 8>()); break;
    case 16: fn(std::integral_constant<int, 16>()); break;
    case 24: fn(std::integral_constant<int, 24>()); break;
    default: fn(std::integral_constant<int, 32>()); break;
  }
}

// the tile part of a launch's arguments; -> the number of tiles
long tile_args(TileArgs& t, const unsigned char* labels, const unsigned char* action, const unsigned short* taps, int radius,
               int F, int H, int W, int a256) {
  t.labels = labels;
  t.action = action;
  t.taps = taps;
  t.n_taps = radius + 1;
  t.radius = padded(radius);
  t.H = H; t.W = W;
  t.tiles_x = (unsigned)((W + TW - 1) / TW);
  t.tiles_y = (unsigned)((H + TH - 1) / TH);
  t.a256 = (uint32_t)a256;
  return (long)F * t.tiles_y * t.tiles_x;                             // <= F * H * W < 2^31
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
  int src_bytes;                 // the source's share of the dynamic LDS (>= 4 * TH * TW: the result plane takes its place); the entry's
};

// What an RGB entry does before it sizes its LDS: the checks (rgb_call's, then the tap table's) and every field of `a` but src_bytes.
// -> the status and the number of tiles; the entry launches where the status is MDQE_OK and F > 0.
int blur_rgb_call(const void* frames, long frame_stride, int h0, int w0, const unsigned char* labels, int F, int Ho, int Wo,
                  const unsigned char* palette, const unsigned char* action, int a256, int contour, const unsigned short* taps, int radius,
                  unsigned char* out, int f_off, BlurArgs& a, long& tiles) {
  MDQE_REQUIRE(radius >= 0 && radius <= MAX_R);
  const int st = rgb_call(frames, frame_stride, h0, w0, labels, F, Ho, Wo, palette, action, true, a256, contour, out, f_off, a.src, a.ident, a.out);
  if (st != MDQE_OK || F == 0) return st;
  MDQE_CHECK_PTR(taps);
  MDQE_REQUIRE(((uintptr_t)taps & 1u) == 0);
  tiles = tile_args(a.t, labels, action, taps, radius, F, Ho, Wo, a256);
  a.palette = palette;
  a.head = (unsigned)((uintptr_t)a.out & 3u);
  a.items = paint_items(TW, Wo, a.head);
  a.m_items = magic(a.items);
  return MDQE_OK;
}

// the RGB paint phase of both kernels: action 3 takes the blurred pixel res[r][x], action 1 tints, every other action keeps
template <int KIND, int CR>
__device__ __forceinline__ void paint_blur_rgb(const BlurArgs& a, const TilePos& p, const uint32_t* pal, const unsigned char* act,
                                               const uint32_t* res, int tid) {
  paint_rgb_tile<KIND, CR, 3u>(
      a.t.labels, a.t.H, a.t.W, a.t.a256, a.src, a.ident, a.out, a.head, p, a.items, a.m_items, pal, act, tid,
      [&](int r) { return [row = res + r * TW](int x) { return row[x] & 0x00FFFFFFu; }; }, [](uint32_t ac) { return ac == 1u; });
}

// ---- surfaces -----------------------------------------------------------------------------------------------------------------------
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

// What a surface entry does before it sizes its LDS: the checks (surface_call's, then the tap tables') and every field of `a`.
// -> the status and the number of tiles; the entry launches where the status is MDQE_OK and F > 0.
int blur_yuv_call(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride, int F, int H, int W, int fmt,
                  const unsigned char* labels, const unsigned short* palette_yuv, const unsigned char* action, int a256, int contour,
                  const unsigned short* taps, int radius, const unsigned short* taps_c, int radius_c, void* out_y, long out_y_pitch,
                  long out_y_stride, void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, BlurYuvArgs& a, long& tiles) {
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
  tiles = tile_args(a.t, labels, action, taps, radius, F, H, W, a256);
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
  return MDQE_OK;
}

// The surface paint phase of both kernels: item j of row pair rp is the 2 x 2 block at column 2 * j of the tile, one block per thread
// and step, single samples at any alignment.  ry: [TH][TW] blurred luma values, rc: [2][CTH][CTW] blurred U, V of the pairs (both
// looked at for pixels of action 3 only, which lie in a flagged tile); pal, act: the LDS tables.
template <int FMT, int CR>
__device__ __forceinline__ void paint_blur_blocks(const BlurYuvArgs& a, const TilePos& p, const uint32_t* pal, const unsigned char* act,
                                                  const unsigned short* ry, const unsigned short* rc, int tid) {
  const TileArgs& t = a.t;
  constexpr int BPS = FMT ? 2 : 1;                                   // bytes per sample
  const unsigned char* y0 = a.y + p.f * a.y_stride + (long)p.Y0 * a.y_pitch + (long)p.X0 * BPS;             // sample (Y0, X0)
  const unsigned char* c0p = a.uv + p.f * a.uv_stride + (long)(p.Y0 / 2) * a.uv_pitch + (long)p.X0 * BPS;   // pair (Y0 / 2, X0 / 2)
  unsigned char* oy0 = a.oy + p.f * a.oy_stride + (long)p.Y0 * a.oy_pitch + (long)p.X0 * BPS;
  unsigned char* oc0 = a.ouv + p.f * a.ouv_stride + (long)(p.Y0 / 2) * a.ouv_pitch + (long)p.X0 * BPS;
  const unsigned char* lab0 = t.labels + ((long)p.f * t.H + p.Y0) * t.W + p.X0;
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
        if (ac == 3u) {
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

}  // namespace
