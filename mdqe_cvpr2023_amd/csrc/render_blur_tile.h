// The tile scheme of the two blur painters, said once: what render_blur.hip (the plain Gaussian) and render_blur_within.hip (the
// edge-stopping one) share.  A thread block of 256 threads owns a tile of 16 x 64 output pixels of one frame; a tile is filtered only
// when one of its pixels has action 3; the tap loops are compiled once per padded radius.  The kernels, their LDS plans, their passes
// and their painters stay in the two .hip files.
#pragma once
#include "render_rule.h"

namespace {

constexpr int TH = 16, TW = 64;                  // the tile, in output pixels
constexpr int MAX_R = 32, MAX_RC = 16;

uint32_t magic(int d) { return (uint32_t)(((1ull << 32) + (unsigned)d - 1) / (unsigned)d); }   // d >= 2
__device__ __forceinline__ int mdiv(int n, uint32_t m) { return (int)__umulhi((uint32_t)n, m); }
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

struct TilePos { int f, Y0, X0, th, tw; };                            // frame, origin, in-picture rows and columns of the tile

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

}  // namespace
