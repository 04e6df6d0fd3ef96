// The mosaic overlay: a label map painted with a PER-LABEL action -- keep the source, tint it as render.hip / render_yuv.hip do, or replace
// it by the mean of its cell x cell square of the picture (a redaction mosaic).  ONE definition, integers only (include/mdqe_hip.h has the
// rule); tests/_mosaic_ref.py restates it in numpy with loops over cells and every comparison is exact.
//
// A cell's mean needs every sample of the cell, so a thread block owns WHOLE cells: a tile of ny x nx cells of one frame (tile_of: about
// 16 x 64 pixels for cells up to 16, one or two cells above that, never more than 256 cells), 256 threads, four phases between barriers:
//   1 flags   every label of the tile is read once (4 at a time where the map and W are multiples of 4 bytes); a pixel whose action is 2
//             sets its cell's LDS flag (a plain store of 1);
//   2 sums    only flagged cells are reduced -- a tile that flags nothing skips the phase wave by wave and its source is read once, by
//             phase 4.  Consecutive lanes are consecutive pixels of a row (cell a multiple of 4: runs of 4 pixels, summed in the lane
//             first; uint8 frames at the output's size and aligned NV12 rows with one v_sad_u8 per dword); with G the largest power
//             of two in `cell`, the G (G / 4) lanes of a group lie in one row of one cell (the tile width, 256 and 64 are multiples of
//             G), so a butterfly of wave shuffles adds them up and the group's first lane adds the result to the cell's LDS counters
//             (ds_add_u32: integer sums are the same in any order; nothing touches global memory).  Channels 0 and 2 (U and V) ride
//             in one register: 64 values of at most 1023 stay below 2^16;
//   3 means   one thread per flagged cell: (sum + n / 2) / n over the n in-picture samples, the one integer division of a cell, packed
//             into one LDS dword per cell;
//   4 paint   the painters of render.hip and render_yuv.hip with the action selecting the value.  RGB: groups of 4 pixels laid out from
//             the OUTPUT address as there (three aligned dword stores per group; a group cut by the tile's side stores its pixels as
//             bytes), labels and uint8 frames of a whole group read 4 bytes at a time.  Surfaces: a thread owns 2 rows x PX pixels,
//             PX = 4 with 4-byte (P010: 8-byte) accesses where every pointer, pitch, stride and W are multiples of 4 bytes, else PX = 2
//             and single samples.  Contour neighbours are looked at for tinted pixels only, straight from the label map (L1).
// With the mosaic on the background nearly every cell is reduced: the frame is read twice, the second time from L2 (a tile's 3 to 12 KB
// were touched microseconds before).  No atomics on global memory, no data-dependent order anywhere: identical from run to run.
// Row and cell indices inside a tile come from multiplications by ceil(2^32 / d) (exact while n * d < 2^32; a tile has fewer than 2^13
// pixels and d <= 124).
// Both kernels say a phase once: the LDS block (TileLds, init_lds), tile_pos, flag_cells, the sum loop (sum_flagged over what a lane adds
// up: RgbSum, LumaSum, ChromaSum; the fast loads are the loader each kernel passes in) and cell_means.  The rule's pieces (source pixel,
// tints, sample helpers, contour test and dispatch) and the entries' checks are render_rule.h's, shared with the plain painters; the RGB
// paint phase (paint_rgb_tile, with the groups' count and the multiplications by ceil(2^32 / d)) is render_tile_paint.h's, shared with
// the two blurs.  The surface paint phase is this file's own: 2 rows x PX pixels per thread with chunked loads.
#include "render_tile_paint.h"

namespace {

constexpr int MAX_CELLS = 256;

struct Tile { int ny, nx; };
// ny x nx cells: about 16 rows by 64 columns, at least one cell, the width a multiple of 4 (cell is even; an odd count of cells of
// 4k + 2 pixels gets one more).  cell = 2: 8 x 32 = 256 cells.
Tile tile_of(int cell) {
  int ny = 16 / cell, nx = 64 / cell;
  if (ny < 1) ny = 1;
  if (nx < 1) nx = 1;
  if ((nx * cell) & 3) ++nx;
  return {ny, nx};
}

struct TileArgs {
  const unsigned char* labels;   // [F, H, W]
  const unsigned char* action;   // [256]
  int H, W;
  int cell, ny, nx, G;           // G: lanes of a reduction group
  int TH, TW;                    // ny * cell, nx * cell
  unsigned tiles_x, tiles_y;
  uint32_t m_tw, m_cell, m_items, m_htw, m_q;   // magic of TW, cell, items per row (pair), TW / 2, TW / 4
  int lab4;                      // labels and W are multiples of 4 bytes: a row of a tile is read 4 labels at a time
  int items;                     // paint items per tile row (RGB) or row pair (surfaces)
  uint32_t a256;
};

__device__ __forceinline__ TilePos tile_pos(const TileArgs& a) {
  unsigned b = blockIdx.x;
  const unsigned tx = b % a.tiles_x;
  b /= a.tiles_x;
  const unsigned ty = b % a.tiles_y;
  TilePos p;
  p.f = (int)(b / a.tiles_y);
  p.Y0 = (int)ty * a.TH;
  p.X0 = (int)tx * a.TW;
  p.th = a.H - p.Y0 < a.TH ? a.H - p.Y0 : a.TH;
  p.tw = a.W - p.X0 < a.TW ? a.W - p.X0 : a.TW;
  return p;
}

// phase 1: flag[cell] = 1 where a pixel of the cell has action 2 (between the caller's barriers)
__device__ __forceinline__ void flag_cells(const TileArgs& a, const TilePos& p, const unsigned char* act, uint32_t* flag) {
  const unsigned char* lab0 = a.labels + ((long)p.f * a.H + p.Y0) * a.W + p.X0;
  if (a.lab4) {                                                       // (W and the tile's width are multiples of 4: so is tw)
    const int Q = a.TW >> 2;
    for (int i = threadIdx.x; i < p.th * Q; i += 256) {
      const int r = mdiv(i, a.m_q), c = 4 * (i - r * Q);
      if (c >= p.tw) continue;
      const uint32_t l4 = *(const uint32_t*)(lab0 + (long)r * a.W + c);
      const int cyn = mdiv(r, a.m_cell) * a.nx;
      // (cell is even: pixels c, c + 1 share a cell and so do c + 2, c + 3)
      if (act[l4 & 0xFFu] == 2 || act[(l4 >> 8) & 0xFFu] == 2) flag[cyn + mdiv(c, a.m_cell)] = 1u;
      if (act[(l4 >> 16) & 0xFFu] == 2 || act[l4 >> 24] == 2) flag[cyn + mdiv(c + 2, a.m_cell)] = 1u;
    }
    return;
  }
  for (int i = threadIdx.x; i < p.th * a.TW; i += 256) {
    const int r = mdiv(i, a.m_tw), c = i - r * a.TW;
    if (c < p.tw && act[lab0[(long)r * a.W + c]] == 2) flag[mdiv(r, a.m_cell) * a.nx + mdiv(c, a.m_cell)] = 1u;
  }
}

// in-picture rows / columns of cell (cy, cx) of the tile
__device__ __forceinline__ int cell_extent(int cell, int k, int have) { return have - k * cell < cell ? have - k * cell : cell; }

// A block's LDS: the palette rows (packed by the kernel's format), the action table, and per cell of the tile its flag, sums and mean.
// A view of five arrays that each kernel declares itself (TILE_LDS): as members of ONE struct in LDS the compiler addressed them
// differently and the kernels' code was no longer the measured one.
struct TileLds {
  uint32_t (&pal)[256];
  unsigned char (&act)[256];
  uint32_t (&flag)[MAX_CELLS];
  uint32_t (&sum)[3][MAX_CELLS];
  uint32_t (&mean)[MAX_CELLS];
};
#define TILE_LDS(name)                                                                                              \
  __shared__ uint32_t pal[256];                                                                                     \
  __shared__ unsigned char act[256];                                                                                \
  __shared__ uint32_t flag[MAX_CELLS];                                                                              \
  __shared__ uint32_t sum[3][MAX_CELLS];                                                                            \
  __shared__ uint32_t mean[MAX_CELLS];                                                                              \
  const TileLds name{pal, act, flag, sum, mean}

// thread tid's share of the prologue (before the first barrier): its palette row, its action, and zeroes
__device__ __forceinline__ void init_lds(const TileLds& lds, const TileArgs& t, int tid, uint32_t pal_row) {
  lds.pal[tid] = pal_row;
  lds.act[tid] = t.action[tid];
  lds.flag[tid] = 0u;
  lds.sum[0][tid] = 0u; lds.sum[1][tid] = 0u; lds.sum[2][tid] = 0u;
}

// What a lane adds up in phase 2, with the wave-shuffle step of the butterfly and the add to the cell's LDS counters.  RGB: channels 0
// and 2 in one register, channel 1 in another; a surface's luma: one register; its chroma: U | V << 16 in one.
struct RgbSum {
  uint32_t v02 = 0u, v1 = 0u;
  __device__ __forceinline__ void px(uint32_t s) { v02 += s & 0x00FF00FFu; v1 += (s >> 8) & 0xFFu; }
  __device__ __forceinline__ void shuffle_add(int d) { v02 += (uint32_t)__shfl_xor((int)v02, d); v1 += (uint32_t)__shfl_xor((int)v1, d); }
  __device__ __forceinline__ void add_to(const TileLds& lds, int ci) const {
    atomicAdd(&lds.sum[0][ci], v02 & 0xFFFFu);
    atomicAdd(&lds.sum[1][ci], v1);
    atomicAdd(&lds.sum[2][ci], v02 >> 16);
  }
};
struct LumaSum {
  uint32_t v = 0u;
  __device__ __forceinline__ void shuffle_add(int d) { v += (uint32_t)__shfl_xor((int)v, d); }
  __device__ __forceinline__ void add_to(const TileLds& lds, int ci) const { atomicAdd(&lds.sum[0][ci], v); }
};
struct ChromaSum {
  uint32_t v = 0u;
  __device__ __forceinline__ void shuffle_add(int d) { v += (uint32_t)__shfl_xor((int)v, d); }
  __device__ __forceinline__ void add_to(const TileLds& lds, int ci) const {
    atomicAdd(&lds.sum[1][ci], v & 0xFFFFu);
    atomicAdd(&lds.sum[2][ci], v >> 16);
  }
};

// phase 2: the sums of the flagged cells over `rows` rows of Q lanes, lane j of a row taking the N consecutive samples from column
// c = N * j (in the picture while c < cols) as load(r, c) -> V.  SUB = 2: a chroma plane, whose pair (r, c) lies under pixel (2r, 2c).
// Consecutive lanes are consecutive samples of a row and the `lanes` (a power of two) lanes of a group lie in one row of one cell, so a
// butterfly of wave shuffles adds them up and the group's first lane -- the smallest column, in the picture if any is -- adds the
// result to the cell's counters.  m_q: the magic of Q.
template <int N, int SUB, class V, class Load>
__device__ __forceinline__ void sum_flagged(const TileArgs& t, const TileLds& lds, int tid, int rows, int cols, int Q, uint32_t m_q, int lanes, Load load) {
  for (int i0 = 0; i0 < rows * Q; i0 += 256) {                         // (the same trip count for every lane: the shuffles need all of them)
    const int i = i0 + tid;
    const int r = mdiv(i, m_q), c = N * (i - r * Q);
    const int ci = mdiv(SUB * r, t.m_cell) * t.nx + mdiv(SUB * c, t.m_cell);
    const bool on = i < rows * Q && c < cols && lds.flag[ci] != 0u;
    if (!__any(on)) continue;                                         // (uniform over the wave)
    V v;
    if (on) v = load(r, c);
    for (int d = 1; d < lanes; d <<= 1) v.shuffle_add(d);
    if (on && (tid & (lanes - 1)) == 0) v.add_to(lds, ci);
  }
}

// phase 3: one thread per flagged cell: (sum + n / 2) / n over the n in-picture samples (> 0: the cell has a flagged pixel), the three
// means packed BITS apart into the cell's LDS dword.  CHROMA: sums 1 and 2 are over the pairs under the cell, not over its pixels.
template <int BITS, bool CHROMA>
__device__ __forceinline__ void cell_means(const TileArgs& t, const TilePos& p, const TileLds& lds, int tid) {
  if (tid < t.ny * t.nx && lds.flag[tid] != 0u) {
    const int cy = tid / t.nx, cx = tid - cy * t.nx;
    const int hh = cell_extent(t.cell, cy, p.th), ww = cell_extent(t.cell, cx, p.tw);
    const uint32_t n = (uint32_t)(hh * ww), nc = CHROMA ? (uint32_t)(((hh + 1) / 2) * ((ww + 1) / 2)) : n;
    lds.mean[tid] = (lds.sum[0][tid] + n / 2) / n | (lds.sum[1][tid] + nc / 2) / nc << BITS | (lds.sum[2][tid] + nc / 2) / nc << 2 * BITS;
  }
}

// ---- RGB ----------------------------------------------------------------------------------------------------------------------------
struct MosaicArgs {
  TileArgs t;
  RgbSource src;
  const unsigned char* palette;  // [256, 3]
  unsigned char* out;            // at frame f_off already: [F, Ho, Wo, 3]
  unsigned head;                 // out address mod 4: groups of 4 pixels start at flat pixels = head (mod 4)
  int ident;
};

template <int KIND, int R>
__global__ __launch_bounds__(256) void render_mosaic_kernel(const MosaicArgs a) {
  TILE_LDS(lds);
  const TileArgs& t = a.t;
  const int tid = (int)threadIdx.x;
  init_lds(lds, t, tid, pack_rgb(a.palette + 3 * tid));
  __syncthreads();
  const TilePos p = tile_pos(t);
  flag_cells(t, p, lds.act, lds.flag);
  __syncthreads();
  // G >= 4 (cell a multiple of 4): a lane sums 4 consecutive pixels of a row, which share a cell, and a group is G / 4 lanes (uint8
  // frames at the output's size: one v_sad_u8 per plane); else one pixel per lane, groups of G = 2
  if (t.G >= 4)
    sum_flagged<4, 1, RgbSum>(t, lds, tid, p.th, p.tw, t.TW >> 2, t.m_q, t.G >> 2, [&](int r, int c) {
      RgbSum v;
      if (KIND == 1 && a.ident && c + 4 <= p.tw) {
        const unsigned char* q = (const unsigned char*)a.src.frames + (long)p.f * a.src.frame_stride + (long)(p.Y0 + r) * a.src.w0 + p.X0 + c;
        v.v02 = __builtin_amdgcn_sad_u8(ld4(q), 0u, 0u) | __builtin_amdgcn_sad_u8(ld4(q + 2 * a.src.plane), 0u, 0u) << 16;   // byte sums
        v.v1 = __builtin_amdgcn_sad_u8(ld4(q + a.src.plane), 0u, 0u);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c + k < p.tw) v.px(source_of<KIND>(a.src, a.ident, p.f, p.Y0 + r, p.X0 + c + k, t.H, t.W));
      }
      return v;
    });
  else
    sum_flagged<1, 1, RgbSum>(t, lds, tid, p.th, p.tw, t.TW, t.m_tw, t.G, [&](int r, int c) {
      RgbSum v;
      v.px(source_of<KIND>(a.src, a.ident, p.f, p.Y0 + r, p.X0 + c, t.H, t.W));
      return v;
    });
  __syncthreads();
  cell_means<8, false>(t, p, lds, tid);
  __syncthreads();
  // paint (render_tile_paint.h): action 2 takes the cell's mean, every other action but 0 tints
  paint_rgb_tile<KIND, R, 2u>(
      t.labels, t.H, t.W, t.a256, a.src, a.ident, a.out, a.head, p, t.items, t.m_items, lds.pal, lds.act, tid,
      [&](int r) { return [&lds, &t, cyn = mdiv(r, t.m_cell) * t.nx](int x) { return lds.mean[cyn + mdiv(x, t.m_cell)]; }; },
      [](uint32_t ac) { return ac != 0u; });
}

template <int KIND>
void launch_mosaic(int contour, dim3 grid, hipStream_t stream, const MosaicArgs& a) {
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_mosaic_kernel<KIND, decltype(R)::value>), grid, dim3(256), 0, stream, a);
  });
}

// the tile part of a launch's arguments; -> the number of tiles
long tile_args(TileArgs& t, const unsigned char* labels, const unsigned char* action, int F, int H, int W, int cell, int a256) {
  const Tile tl = tile_of(cell);
  t.labels = labels;
  t.action = action;
  t.H = H; t.W = W;
  t.cell = cell; t.ny = tl.ny; t.nx = tl.nx;
  t.G = cell & -cell;
  t.TH = tl.ny * cell; t.TW = tl.nx * cell;
  t.tiles_x = (unsigned)((W + t.TW - 1) / t.TW);
  t.tiles_y = (unsigned)((H + t.TH - 1) / t.TH);
  t.m_tw = magic(t.TW);
  t.m_cell = magic(cell);
  t.m_htw = magic(t.TW / 2);
  t.m_q = magic(t.TW / 4);
  t.lab4 = (((uintptr_t)labels | (uintptr_t)W) & 3u) == 0;
  t.a256 = (uint32_t)a256;
  return (long)F * t.tiles_y * t.tiles_x;                             // <= F * H * W < 2^31
}

// ---- surfaces -----------------------------------------------------------------------------------------------------------------------
struct MosaicYuvArgs {
  TileArgs t;
  const unsigned char* y;
  const unsigned char* uv;
  const unsigned short* palette;                 // [256, 3]: Y, U, V in sample units
  unsigned char* oy;                             // at frame f_off already
  unsigned char* ouv;
  long y_pitch, y_stride, uv_pitch, uv_stride;   // bytes
  long oy_pitch, oy_stride, ouv_pitch, ouv_stride;
};

// One 2 x 2 block (columns c, c + 1 of rows r0, r0 + 1; nr x nc of them in the picture): the rule as written, on stored samples ry, ru,
// rv handed in and the block's labels read at `lab` (the label of (r0, c)).  m: the packed means of the block's cell.
template <int FMT, int R>
__device__ __forceinline__ void block2x2(const TileArgs& t, const uint32_t* pal, const unsigned char* act, uint32_t m,
                                         const unsigned char* lab, int r0, int c, int nr, int nc,
                                         const uint32_t (&ry)[2][2], uint32_t ru, uint32_t rv, uint32_t (&oy)[2][2], uint32_t& ou, uint32_t& ov) {
  const uint32_t U = value_of<FMT>(ru), V = value_of<FMT>(rv);
  uint32_t su = 0u, sv = 0u, any = 0u;
#pragma unroll
  for (int row = 0; row < 2; ++row) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      oy[row][k] = 0u;
      if (row >= nr || k >= nc) continue;
      const unsigned char* q = lab + (long)row * t.W + k;
      const uint32_t l = q[0], ac = act[l];
      any |= ac;
      if (ac == 0u) {
        oy[row][k] = ry[row][k];
        su += U; sv += V;
      } else if (ac == 2u) {
        oy[row][k] = stored<FMT>(comp<FMT>(m, 0));
        su += comp<FMT>(m, 1); sv += comp<FMT>(m, 2);
      } else {
        const bool edge = edge_at<R>(q, l, r0 + row, c + k, t.H, t.W);
        const uint32_t col = pal[l];
        oy[row][k] = stored<FMT>(tint1(value_of<FMT>(ry[row][k]), comp<FMT>(col, 0), edge, t.a256));
        su += tint1(U, comp<FMT>(col, 1), edge, t.a256);
        sv += tint1(V, comp<FMT>(col, 2), edge, t.a256);
      }
    }
  }
  const uint32_t sh = (uint32_t)(nr * nc) >> 1;                       // n = 1, 2, 4: n / 2 = log2(n) = 0, 1, 2
  ou = any != 0u ? stored<FMT>((su + sh) >> sh) : ru;
  ov = any != 0u ? stored<FMT>((sv + sh) >> sh) : rv;
}

template <int FMT, int PX, int R>
__global__ __launch_bounds__(256) void render_mosaic_yuv_kernel(const MosaicYuvArgs a) {
  TILE_LDS(lds);
  const TileArgs& t = a.t;
  const int tid = (int)threadIdx.x;
  init_lds(lds, t, tid, pack_yuv(a.palette + 3 * tid));
  __syncthreads();
  const TilePos p = tile_pos(t);
  constexpr int BPS = FMT ? 2 : 1;                                   // bytes per sample
  const unsigned char* y0 = a.y + p.f * a.y_stride + (long)p.Y0 * a.y_pitch + (long)p.X0 * BPS;          // sample (Y0, X0)
  const unsigned char* c0p = a.uv + p.f * a.uv_stride + (long)(p.Y0 / 2) * a.uv_pitch + (long)p.X0 * BPS;  // pair (Y0 / 2, X0 / 2)
  unsigned char* oy0 = a.oy + p.f * a.oy_stride + (long)p.Y0 * a.oy_pitch + (long)p.X0 * BPS;
  unsigned char* oc0 = a.ouv + p.f * a.ouv_stride + (long)(p.Y0 / 2) * a.ouv_pitch + (long)p.X0 * BPS;
  const unsigned char* lab0 = t.labels + ((long)p.f * t.H + p.Y0) * t.W + p.X0;
  flag_cells(t, p, lds.act, lds.flag);
  __syncthreads();
  // luma: 4 samples per lane where cell is a multiple of 4, as the RGB kernel's (an aligned launch, whose tw is a multiple of 4, reads
  // them as one dword -- one v_sad_u8 -- or as P010's dword pair)
  if (t.G >= 4)
    sum_flagged<4, 1, LumaSum>(t, lds, tid, p.th, p.tw, t.TW >> 2, t.m_q, t.G >> 2, [&](int r, int c) {
      LumaSum v;
      const unsigned char* q = y0 + (long)r * a.y_pitch;
      if (PX == 4) {
        uint32_t w[BPS];
        __builtin_memcpy(w, __builtin_assume_aligned(q + (long)c * BPS, 4), 4 * BPS);
        if (FMT == 0) v.v = __builtin_amdgcn_sad_u8(w[0], 0u, 0u);
        else v.v = ((w[0] & 0xFFFFu) >> 6) + (w[0] >> 22) + ((w[BPS - 1] & 0xFFFFu) >> 6) + (w[BPS - 1] >> 22);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c + k < p.tw) v.v += value_of<FMT>(row_raw<FMT>(q, c + k));
      }
      return v;
    });
  else
    sum_flagged<1, 1, LumaSum>(t, lds, tid, p.th, p.tw, t.TW, t.m_tw, t.G, [&](int r, int c) {
      return LumaSum{value_of<FMT>(row_raw<FMT>(y0 + (long)r * a.y_pitch, c))};
    });
  // chroma: the pairs under the same cells, groups of G / 2 lanes (G >= 2)
  const int chr = (p.th + 1) / 2, chc = (p.tw + 1) / 2;
  sum_flagged<1, 2, ChromaSum>(t, lds, tid, chr, chc, t.TW / 2, t.m_htw, t.G / 2, [&](int r, int c) {
    const unsigned char* q = c0p + (long)r * a.uv_pitch;
    return ChromaSum{value_of<FMT>(row_raw<FMT>(q, 2 * c)) | value_of<FMT>(row_raw<FMT>(q, 2 * c + 1)) << 16};
  });
  __syncthreads();
  cell_means<10, true>(t, p, lds, tid);
  __syncthreads();
  // paint: item j of row pair rp is the block of 2 rows x PX pixels at column PX * j of the tile
  for (int it = tid; it < chr * t.items; it += 256) {
    const int rp = mdiv(it, t.m_items), j = it - rp * t.items;
    const int cb = PX * j;                                            // column inside the tile
    if (cb >= p.tw) continue;
    const int r0 = p.Y0 + 2 * rp, c0 = p.X0 + cb;
    const int nr = r0 + 1 < t.H ? 2 : 1;
    const int cyn = mdiv(2 * rp, t.m_cell) * t.nx;
    const unsigned char* yrow = y0 + (long)(2 * rp) * a.y_pitch;
    const unsigned char* crow = c0p + (long)rp * a.uv_pitch;
    unsigned char* oyrow = oy0 + (long)(2 * rp) * a.oy_pitch;
    unsigned char* ocrow = oc0 + (long)rp * a.ouv_pitch;
    const unsigned char* lab = lab0 + (long)(2 * rp) * t.W + cb;
    if constexpr (PX == 4) {
      // every pointer, pitch, stride and W are multiples of 4 and so is the tile's width: the block lies inside the row, 4-byte aligned
      constexpr int NW = BPS;                                         // dwords of 4 samples
      uint32_t yw[2][NW], cw[NW], oyw[2][NW], ocw[NW];
      __builtin_memcpy(yw[0], __builtin_assume_aligned(yrow + (long)cb * BPS, 4), 4 * NW);
      if (nr == 2) __builtin_memcpy(yw[1], __builtin_assume_aligned(yrow + a.y_pitch + (long)cb * BPS, 4), 4 * NW);
      else { yw[1][0] = 0u; yw[1][NW - 1] = 0u; }
      __builtin_memcpy(cw, __builtin_assume_aligned(crow + (long)cb * BPS, 4), 4 * NW);
#pragma unroll
      for (int q = 0; q < 2; ++q) {                                   // the block's two chroma pairs
        uint32_t ry[2][2], o[2][2], ou, ov;
#pragma unroll
        for (int row = 0; row < 2; ++row) {
          if (FMT == 0) { ry[row][0] = (yw[row][0] >> 16 * q) & 0xFFu; ry[row][1] = (yw[row][0] >> (16 * q + 8)) & 0xFFu; }
          else { ry[row][0] = yw[row][q] & 0xFFFFu; ry[row][1] = yw[row][q] >> 16; }
        }
        const uint32_t ru = FMT == 0 ? (cw[0] >> 16 * q) & 0xFFu : cw[q] & 0xFFFFu;
        const uint32_t rv = FMT == 0 ? (cw[0] >> (16 * q + 8)) & 0xFFu : cw[q] >> 16;
        block2x2<FMT, R>(t, lds.pal, lds.act, lds.mean[cyn + mdiv(cb + 2 * q, t.m_cell)], lab + 2 * q, r0, c0 + 2 * q, nr, 2, ry, ru, rv, o, ou, ov);
        if (FMT == 0) {
#pragma unroll
          for (int row = 0; row < 2; ++row) {
            const uint32_t two = o[row][0] | o[row][1] << 8;
            oyw[row][0] = q == 0 ? two : oyw[row][0] | two << 16;
          }
          ocw[0] = q == 0 ? (ou | ov << 8) : ocw[0] | (ou | ov << 8) << 16;
        } else {
          oyw[0][q] = o[0][0] | o[0][1] << 16;
          oyw[1][q] = o[1][0] | o[1][1] << 16;
          ocw[q] = ou | ov << 16;
        }
      }
      __builtin_memcpy(__builtin_assume_aligned(oyrow + (long)cb * BPS, 4), oyw[0], 4 * NW);
      if (nr == 2) __builtin_memcpy(__builtin_assume_aligned(oyrow + a.oy_pitch + (long)cb * BPS, 4), oyw[1], 4 * NW);
      __builtin_memcpy(__builtin_assume_aligned(ocrow + (long)cb * BPS, 4), ocw, 4 * NW);
    } else {
      const int nc = c0 + 1 < t.W ? 2 : 1;
      uint32_t ry[2][2] = {{0u, 0u}, {0u, 0u}}, o[2][2], ou, ov;
#pragma unroll
      for (int row = 0; row < 2; ++row)
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (row < nr && k < nc) ry[row][k] = row_raw<FMT>(yrow + (long)row * a.y_pitch, cb + k);
      const uint32_t ru = row_raw<FMT>(crow, cb), rv = row_raw<FMT>(crow, cb + 1);
      block2x2<FMT, R>(t, lds.pal, lds.act, lds.mean[cyn + mdiv(cb, t.m_cell)], lab, r0, c0, nr, nc, ry, ru, rv, o, ou, ov);
#pragma unroll
      for (int row = 0; row < 2; ++row)
#pragma unroll
        for (int k = 0; k < 2; ++k)
          if (row < nr && k < nc) row_put<FMT>(oyrow + (long)row * a.oy_pitch, cb + k, o[row][k]);
      row_put<FMT>(ocrow, cb, ou);
      row_put<FMT>(ocrow, cb + 1, ov);
    }
  }
}

template <int FMT, int PX>
void launch_my(int contour, dim3 grid, hipStream_t stream, const MosaicYuvArgs& a) {
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_mosaic_yuv_kernel<FMT, PX, decltype(R)::value>), grid, dim3(256), 0, stream, a);
  });
}

bool cell_ok(int cell) { return cell >= 2 && cell <= 64 && (cell & 1) == 0; }

}  // namespace

extern "C" int mdqe_render_mosaic_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                                     const unsigned char* labels, int F, int Ho, int Wo,
                                     const unsigned char* palette, const unsigned char* action, int a256, int contour, int cell,
                                     unsigned char* out, int f_off, void* stream) {
  MDQE_REQUIRE(cell_ok(cell));
  MosaicArgs a;
  const int st = rgb_call(frames, frame_stride, h0, w0, labels, F, Ho, Wo, palette, action, true, a256, contour, out, f_off, a.src, a.ident, a.out);
  if (st != MDQE_OK || F == 0) return st;
  const long tiles = tile_args(a.t, labels, action, F, Ho, Wo, cell, a256);
  a.palette = palette;
  a.head = (unsigned)((uintptr_t)a.out & 3u);
  a.t.items = paint_items(a.t.TW, Wo, a.head);
  a.t.m_items = magic(a.t.items);
  mdqe_clear_error();
  const dim3 grid((unsigned)tiles);
  if (frames == nullptr) launch_mosaic<0>(contour, grid, (hipStream_t)stream, a);
  else if (is_u8) launch_mosaic<1>(contour, grid, (hipStream_t)stream, a);
  else launch_mosaic<2>(contour, grid, (hipStream_t)stream, a);
  return mdqe_launch_status();
}

extern "C" int mdqe_render_mosaic_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                           int F, int H, int W, int fmt, const unsigned char* labels,
                                           const unsigned short* palette_yuv, const unsigned char* action, int a256, int contour, int cell,
                                           void* out_y, long out_y_pitch, long out_y_stride,
                                           void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream) {
  MDQE_REQUIRE(cell_ok(cell));
  // not in place: a cell's mean reads samples that other threads write
  SurfaceOut o;
  const int st = surface_call(y, y_pitch, y_stride, uv, uv_pitch, uv_stride, F, H, W, fmt, labels, palette_yuv, action, true, false, a256,
                              contour, out_y, out_y_pitch, out_y_stride, out_uv, out_uv_pitch, out_uv_stride, f_off, o);
  if (st != MDQE_OK || F == 0) return st;
  // 4-byte accesses where every address of the launch is aligned for them
  const int px = (o.m & 3u) == 0 ? 4 : 2;
  MosaicYuvArgs a;
  const long tiles = tile_args(a.t, labels, action, F, H, W, cell, a256);
  a.t.items = a.t.TW / px;                                            // (TW is a multiple of 4)
  a.t.m_items = magic(a.t.items);
  a.y = (const unsigned char*)y;
  a.uv = (const unsigned char*)uv;
  a.palette = palette_yuv;
  a.oy = o.oy;
  a.ouv = o.ouv;
  a.y_pitch = y_pitch; a.y_stride = y_stride; a.uv_pitch = uv_pitch; a.uv_stride = uv_stride;
  a.oy_pitch = out_y_pitch; a.oy_stride = out_y_stride; a.ouv_pitch = out_uv_pitch; a.ouv_stride = out_uv_stride;
  mdqe_clear_error();
  const dim3 grid((unsigned)tiles);
  hipStream_t s = (hipStream_t)stream;
  if (fmt == 0) { if (px == 4) launch_my<0, 4>(contour, grid, s, a); else launch_my<0, 2>(contour, grid, s, a); }
  else { if (px == 4) launch_my<1, 4>(contour, grid, s, a); else launch_my<1, 2>(contour, grid, s, a); }
  return mdqe_launch_status();
}
