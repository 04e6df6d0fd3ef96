// The RGB paint phase of the tile painters, said once: what render_mosaic.hip, render_blur.hip and render_blur_within.hip share.  A
// thread block of 256 threads owns a tile of one frame's output pixels, works out one special value per pixel in LDS (a cell's mean, a
// blurred pixel) and then paints the tile: groups of 4 flat pixels laid out from the OUTPUT address, three aligned dword stores per
// group, bytes for a group cut by the tile's side.  The tile's size and what its special value is stay with each kernel: the painter
// sees the tile's position, the items of a row and a functor that reads the value.
#pragma once
#include "render_rule.h"

namespace {

uint32_t magic(int d) { return (uint32_t)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); }   // d >= 2
__device__ __forceinline__ int mdiv(int n, uint32_t m) { return (int)__umulhi((uint32_t)n, m); }

struct TilePos { int f, Y0, X0, th, tw; };                            // frame, origin, in-picture rows and columns of the tile

// the source pixel of output pixel (f, Y, X) of an H x W picture
template <int KIND>
__device__ __forceinline__ uint32_t source_of(const RgbSource& src, int ident, int f, int Y, int X, int H, int W) {
  return source_px<KIND>(src, ident, (long)f * src.frame_stride, Y, X, H, W);
}

// The paint items (groups of 4 pixels) of a tile row of `tw` pixels: a segment of tw pixels meets at most tw / 4 + 1 groups; exactly
// tw / 4 where every segment starts a group (Wo and tw are multiples of 4 and so is the output address `head`).
int paint_items(int tw, int Wo, unsigned head) { return tw / 4 + ((Wo & 3) == 0 && head == 0 ? 0 : 1); }

// Item j of tile row r is the j-th group of 4 flat pixels that meets the row's segment.  `head`: the out address mod 4 (groups start at
// flat pixels = head mod 4); m_items: magic(items); pal, act: the LDS tables.  A pixel of action TAKE becomes taken(r)(x) for column x
// of tile row r (a packed pixel, bits 24.. zero; taken(r) is asked once per item, so what belongs to the row is worked out once); any
// other action a tints as render.hip does where tints(a), else keeps the source.
template <int KIND, int R, uint32_t TAKE, class Taken, class Tints>
__device__ __forceinline__ void paint_rgb_tile(const unsigned char* labels, int H, int W, uint32_t a256, const RgbSource& src, int ident,
                                               unsigned char* out, unsigned head, const TilePos& p, int items, uint32_t m_items,
                                               const uint32_t* pal, const unsigned char* act, int tid, Taken taken, Tints tints) {
  for (int it = tid; it < p.th * items; it += 256) {
    const int r = mdiv(it, m_items), j = it - r * items;
    const int Y = p.Y0 + r;
    const long row = ((long)p.f * H + Y) * W;                         // flat pixel of (f, Y, 0), < 2^31
    const long seg = row + p.X0;                                      // the segment: flat pixels [seg, seg + tw)
    const long ps = 4 * ((seg + 4 - head) / 4 + j) + head - 4;        // the group's first flat pixel (may lie before seg)
    const long lo = ps > seg ? ps : seg, hi = ps + 4 < seg + p.tw ? ps + 4 : seg + p.tw;
    if (lo >= hi) continue;
    const auto taken_at = taken(r);
    const bool whole = hi - lo == 4;
    uint32_t l4 = 0u, c0 = 0u, c1 = 0u, c2 = 0u;
    const bool wide_src = KIND == 1 && whole && ident;
    if (whole) l4 = ld4(labels + ps);
    if (wide_src) {
      const unsigned char* q = (const unsigned char*)src.frames + (long)p.f * src.frame_stride + (long)Y * src.w0 + (int)(ps - row);
      c0 = ld4(q); c1 = ld4(q + src.plane); c2 = ld4(q + 2 * src.plane);
    }
    uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long q = ps + k;
      if (q < lo || q >= hi) continue;
      const int X = (int)(q - row);
      const uint32_t l = whole ? (l4 >> 8 * k) & 0xFFu : (uint32_t)labels[q];
      const uint32_t ac = act[l];
      if (ac == TAKE) {
        px[k] = taken_at(X - p.X0);
        continue;
      }
      const uint32_t s = wide_src ? ((c0 >> 8 * k) & 0xFFu) | ((c1 >> 8 * k) & 0xFFu) << 8 | ((c2 >> 8 * k) & 0xFFu) << 16
                                  : source_of<KIND>(src, ident, p.f, Y, X, H, W);
      px[k] = tints(ac) ? tint(s, pal[l], edge_at<R>(labels + q, l, Y, X, H, W), a256) : s;
    }
    unsigned char* o = out + 3L * ps;
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

}  // namespace
