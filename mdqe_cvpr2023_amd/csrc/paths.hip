// Track paths: the centroid of each label's visible region per frame, and the trail of those centroids over the last frames painted onto
// a picture.  A third consumer of the label map, beside annotate.hip and crops.hip.  ONE definition, integers only (include/mdqe_hip.h
// has the rule); tests/_paths_ref.py restates it in numpy with Python integers and every comparison is exact.
//
// Centroids: three launches.  (1) zero the moment table.  (2) a block sweeps a band of 32 rows of one frame; a thread takes 16
// consecutive bytes of a row, gathers the runs of equal labels in registers and adds a run [xa, xb) of row Y to an LDS table of 64-bit
// sums in closed form (xb - xa, (xa + xb - 1) * (xb - xa) / 2, Y * (xb - xa)); a wave whose 64 pieces all hold one and the same label --
// the inside of a region, most of what is not background -- adds them up with shuffles first and makes three LDS adds instead of 192
// that would queue on one address.  The block's table goes to the global one with 64-bit atomic adds.  (3) a thread per (row, frame)
// divides.  Integer sums: the result does not depend on the order of the adds, identical from run to run.
//
// Trails: one launch, in place, annotate.hip's shape.  A block owns a tile (64 x 16 pixels of an RGB picture, 64 x 32 of a surface: a
// thread then holds the 2 x 4 pixels that decide two chroma pairs).  The block loads the trail's columns of the point table into LDS,
// all rows side by side (in passes where 255 rows x 65 columns do not fit), so the table costs one memory latency and not one per
// column.  Thread r then walks row r there, joins each present point to the next present one, and counts the segments whose box, grown
// by `width`, meets the tile; a scan over the block turns the counts into positions in label order.  A tile no segment reaches ends
// there, before any pixel is touched.  The list is walked in chunks of 512: the threads whose positions fall into the chunk walk their
// row again and store their segments, then every thread tests its pixels that nothing has hit yet against the chunk.  Passes and
// chunks ascend by label, so a pixel's first hit is the rule's.  No atomics, no data-dependent order.
#include "render_rule.h"

namespace {

// ---- centroids ------------------------------------------------------------------------------------------------------------------------
constexpr int BAND = 32, PIECE = 16;

__global__ __launch_bounds__(256) void moments_zero_kernel(unsigned long long* mom, int count) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i < count) mom[i] = 0ull;
}

__device__ __forceinline__ void run_add(unsigned long long* tab, int n, int l, int xa, int xb, int Y) {   // columns [xa, xb) of row Y hold l
  if (l == 0 || l > n) return;                                       // background; a label no row of the table stands for
  const unsigned long long len = (unsigned long long)(xb - xa);
  atomicAdd(tab + 3 * (l - 1), len);
  atomicAdd(tab + 3 * (l - 1) + 1, (unsigned long long)(xa + xb - 1) * len / 2ull);
  atomicAdd(tab + 3 * (l - 1) + 2, (unsigned long long)Y * len);
}

__global__ __launch_bounds__(256) void moments_sweep_kernel(const unsigned char* __restrict__ labels, int F, int Ho, int Wo, int n,
                                                            unsigned bands, unsigned long long* __restrict__ mom) {
  __shared__ unsigned long long tab[255 * 3];
  const int f = (int)(blockIdx.x / bands), band = (int)(blockIdx.x - (unsigned)f * bands);
  for (int i = (int)threadIdx.x; i < 3 * n; i += 256) tab[i] = 0ull;
  __syncthreads();
  const int y0 = band * BAND, rows = (Ho - y0 < BAND ? Ho - y0 : BAND), per_row = (Wo + PIECE - 1) / PIECE, total = rows * per_row;
  const unsigned char* fr = labels + (long)f * Ho * Wo;
  for (int base = 0; base < total; base += 256) {                    // (block-uniform bounds: every lane of a wave is here)
    const int c = base + (int)threadIdx.x;
    const bool active = c < total;
    int Y = 0, x0 = 0, cnt = 0;
    unsigned char b[PIECE];
    if (active) {
      const int r = c / per_row;
      x0 = (c - r * per_row) * PIECE;
      Y = y0 + r;
      cnt = Wo - x0 < PIECE ? Wo - x0 : PIECE;
      const unsigned char* p = fr + (long)Y * Wo + x0;
      if (cnt == PIECE) {
        __builtin_memcpy(b, p, PIECE);                               // (any alignment)
      } else {
#pragma unroll
        for (int q = 0; q < PIECE; ++q) b[q] = q < cnt ? p[q] : p[0];
      }
    }
    bool one = true;                                                 // the piece holds one label
    if (active) {
#pragma unroll
      for (int q = 1; q < PIECE; ++q) one = one && (q >= cnt || b[q] == b[0]);
    }
    const int lab = active ? (int)b[0] : -1;
    const unsigned long long am = __ballot(active);
    if (am == 0ull) continue;                                        // (wave-uniform)
    const int l0 = __shfl(lab, __ffsll((long long)am) - 1, 64);
    if (__all(!active || (one && lab == l0))) {
      if (l0 == 0 || l0 > n) continue;
      int m = cnt, sx = (2 * x0 + cnt - 1) * cnt / 2, sy = Y * cnt;  // (cnt <= 16, x0, Y < 2^14: 64 of them stay below 2^25)
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        m += __shfl_xor(m, d, 64);
        sx += __shfl_xor(sx, d, 64);
        sy += __shfl_xor(sy, d, 64);
      }
      if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(tab + 3 * (l0 - 1), (unsigned long long)m);
        atomicAdd(tab + 3 * (l0 - 1) + 1, (unsigned long long)sx);
        atomicAdd(tab + 3 * (l0 - 1) + 2, (unsigned long long)sy);
      }
      continue;
    }
    if (!active) continue;
    int cur = (int)b[0], xa = 0;
#pragma unroll
    for (int q = 1; q < PIECE; ++q)
      if (q < cnt && (int)b[q] != cur) {
        run_add(tab, n, cur, x0 + xa, x0 + q, Y);
        cur = (int)b[q];
        xa = q;
      }
    run_add(tab, n, cur, x0 + xa, x0 + cnt, Y);
  }
  __syncthreads();
  for (int i = (int)threadIdx.x; i < 3 * n; i += 256) {
    const unsigned long long v = tab[i];
    const int k = i / 3;
    if (v != 0ull) atomicAdd(mom + ((long)k * F + f) * 3 + (i - 3 * k), v);
  }
}

__global__ __launch_bounds__(256) void centroid_points_kernel(const unsigned long long* __restrict__ mom, int F, int count, int min_area,
                                                              int* __restrict__ pts, long pts_row_stride, int p_off) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= count) return;
  const int k = i / F, f = i - k * F;
  const unsigned long long m = mom[3L * i], need = (unsigned long long)(min_area > 1 ? min_area : 1);
  int cx = -1, cy = -1;
  if (m >= need) {
    cx = (int)((mom[3L * i + 1] + m / 2ull) / m);
    cy = (int)((mom[3L * i + 2] + m / 2ull) / m);
  }
  int* q = pts + (long)k * pts_row_stride + 2L * (p_off + f);
  q[0] = cx;
  q[1] = cy;
}

// ---- trails ---------------------------------------------------------------------------------------------------------------------------
constexpr int TILE_W = 64, TILE_H_RGB = 16, TILE_H_YUV = 32;         // 256 threads: 16 units of 4 columns x 16 rows / row pairs
constexpr int CAP = 512;                                             // segments of one chunk of the tile's list
constexpr int PTS = 1040;                                            // points of one pass: 16 rows of 65 columns at least

struct TrailArgs {
  const int* pts;                // row k: pts + k * pts_row_stride, column j: (x, y) at 2 * j
  const void* palette;           // uint8 [256, 3] (RGB) or uint16 [256, 3] (surfaces)
  long pts_row_stride;
  int F, H, W, n, p_off, trail, width;
  unsigned tiles_x, tiles_y;
};

struct SegList {
  int2 pt[PTS];                  // the pass's points, row-major by (row, column); x < 0: absent
  int4 seg[CAP];                 // ax, ay, bx, by -- ascending label
  uint32_t col[CAP];
  int wave_count[4];
};

// fn(ax, ay, bx, by) for each stroke of a row's staged points pt[0 .. cols) whose box, grown by g, meets the tile, in column order.  A
// lone present point is the stroke (P, P); with two or more, the strokes (P, P) lie inside the segments that end in P and are left out.
template <class Fn>
__device__ __forceinline__ void strokes_of(const int2* pt, int cols, int g, int tx0, int ty0, int tx1, int ty1, Fn&& fn) {
  int px = 0, py = 0, seen = 0;
  for (int c = 0; c < cols; ++c) {
    const int2 p = pt[c];
    if (p.x < 0) continue;
    if (seen > 0) {
      const int xl = p.x < px ? p.x : px, xh = p.x < px ? px : p.x, yl = p.y < py ? p.y : py, yh = p.y < py ? py : p.y;
      if (xl - g <= tx1 && xh + g >= tx0 && yl - g <= ty1 && yh + g >= ty0) fn(px, py, p.x, p.y);
    }
    px = p.x; py = p.y; ++seen;
  }
  if (seen == 1 && px - g <= tx1 && px + g >= tx0 && py - g <= ty1 && py + g >= ty0) fn(px, py, px, py);
}

// The rule's hit test of pixel (X, Y) against the stroke (A, B), w2 = width * width.  Every coordinate lies in [0, 2^14): differences
// are below 2^14 in size, a sum of two of their products below 2^29, so everything but the last comparison is exact in 32 bits.
__device__ __forceinline__ bool stroke_hit(int X, int Y, const int4& s, int w2) {
  const int dx = s.z - s.x, dy = s.w - s.y;
  int px = X - s.x, py = Y - s.y;
  const int L2 = dx * dx + dy * dy, t = px * dx + py * dy;
  if (L2 == 0 || t <= 0) return 4 * (px * px + py * py) <= w2;       // (< 2^31)
  if (t >= L2) {
    px = X - s.z; py = Y - s.w;
    return 4 * (px * px + py * py) <= w2;
  }
  const long long c = px * dy - py * dx;                             // |c| < 2^29: 4 c^2 < 2^60
  return 4 * c * c <= (long long)w2 * L2;
}

// The rule on the thread's NX x NY pixels whose top left one is (Y, X); (ty1, tx1) is the tile's last pixel inside the picture.  Every
// thread of the block calls it (it holds barriers).  The rows are taken in passes of as many as fit `pt` (all of them where n * (trail
// + 1) <= PTS: 15 tracks with a trail of 64): the block loads the pass's points side by side -- one latency, not one per column -- and
// marks the absent ones; the pass's thread r then walks row r in LDS, twice: to count, and to store.
// -> bit row * NX + k set: pixel (Y + row, X + k) is hit, its colour in col[row][k]; inside: the pixels that lie in the picture.
template <bool YUV, int NX, int NY>
__device__ __forceinline__ unsigned trail_hits(const TrailArgs& a, int f, int tx0, int ty0, int tx1, int ty1, int Y, int X, SegList& t,
                                               uint32_t (&col)[NY][NX], unsigned& inside) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int cols = a.trail + 1, j0 = a.p_off + f - a.trail, g = a.width;
  const int per_pass = PTS / cols < 256 ? PTS / cols : 256;          // >= 16 rows
  unsigned todo = 0u, hit = 0u;
#pragma unroll
  for (int row = 0; row < NY; ++row)
#pragma unroll
    for (int q = 0; q < NX; ++q)
      if (Y + row <= ty1 && X + q <= tx1) todo |= 1u << (row * NX + q);
  inside = todo;
  const int X1 = X + NX - 1 < tx1 ? X + NX - 1 : tx1, Y1 = Y + NY - 1 < ty1 ? Y + NY - 1 : ty1;
  const int w2 = a.width * a.width;
  for (int r0 = 0; r0 < a.n; r0 += per_pass) {                       // (block-uniform)
    const int rows = a.n - r0 < per_pass ? a.n - r0 : per_pass;
    for (int i = tid; i < rows * cols; i += 256) {
      const int r = i / cols, j = j0 + (i - r * cols);
      int2 p = make_int2(-1, -1);
      if (j >= 0) {
        const int* q = a.pts + (long)(r0 + r) * a.pts_row_stride + 2L * j;
        p = make_int2(q[0], q[1]);
        if (p.x < 0 || p.y < 0 || p.x >= a.W || p.y >= a.H) p.x = -1;
      }
      t.pt[i] = p;
    }
    __syncthreads();
    const int2* mine_pt = t.pt + (tid < rows ? tid : 0) * cols;
    int mine = 0;
    if (tid < rows) strokes_of(mine_pt, cols, g, tx0, ty0, tx1, ty1, [&](int, int, int, int) { ++mine; });
    int incl = mine;                                                 // inclusive scan over the wave, then over the waves
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d, 64);
      if (lane >= d) incl += v;
    }
    if (lane == 63) t.wave_count[wv] = incl;
    __syncthreads();
    int at = incl - mine, total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < wv) at += t.wave_count[i];
      total += t.wave_count[i];
    }
    const int l = r0 + tid + 1;                                      // the label of the pass's row `tid`
    const uint32_t colour = mine > 0 ? (YUV ? pack_yuv((const unsigned short*)a.palette + 3 * l) : pack_rgb((const unsigned char*)a.palette + 3 * l)) : 0u;
    for (int first = 0; first < total; first += CAP) {               // (block-uniform; a tile no stroke of the pass reaches: no turn)
      if (mine > 0 && at < first + CAP && at + mine > first) {
        int i = at;
        strokes_of(mine_pt, cols, g, tx0, ty0, tx1, ty1, [&](int ax, int ay, int bx, int by) {
          if (i >= first && i < first + CAP) {
            t.seg[i - first] = make_int4(ax, ay, bx, by);
            t.col[i - first] = colour;
          }
          ++i;
        });
      }
      __syncthreads();
      const int cnt = total - first < CAP ? total - first : CAP;
      for (int i = 0; i < cnt && todo != 0u; ++i) {
        const int4 s = t.seg[i];
        const int xl = s.x < s.z ? s.x : s.z, xh = s.x < s.z ? s.z : s.x, yl = s.y < s.w ? s.y : s.w, yh = s.y < s.w ? s.w : s.y;
        if (X1 < xl - g || X > xh + g || Y1 < yl - g || Y > yh + g) continue;
#pragma unroll
        for (int row = 0; row < NY; ++row)
#pragma unroll
          for (int q = 0; q < NX; ++q) {
            const unsigned bit = 1u << (row * NX + q);
            if ((todo & bit) != 0u && stroke_hit(X + q, Y + row, s, w2)) {
              col[row][q] = t.col[i];
              hit |= bit;
              todo &= ~bit;
            }
          }
      }
      __syncthreads();                                               // (the next chunk overwrites the list)
    }
    __syncthreads();                                                 // (the next pass overwrites the points and the waves' counts)
  }
  return hit;
}

// -> the tile's column, row and frame of block b
__device__ __forceinline__ void tile_of(const TrailArgs& a, unsigned b, int& tx, int& ty, int& f) {
  const unsigned row = b / a.tiles_x;
  tx = (int)(b - row * a.tiles_x);
  f = (int)(row / a.tiles_y);
  ty = (int)(row - (unsigned)f * a.tiles_y);
}

__global__ __launch_bounds__(256) void trails_u8_kernel(const TrailArgs a, unsigned char* pic) {
  __shared__ SegList t;
  int tx, ty, f;
  tile_of(a, blockIdx.x, tx, ty, f);
  const int tx0 = tx * TILE_W, ty0 = ty * TILE_H_RGB;
  const int tx1 = tx0 + TILE_W - 1 < a.W - 1 ? tx0 + TILE_W - 1 : a.W - 1, ty1 = ty0 + TILE_H_RGB - 1 < a.H - 1 ? ty0 + TILE_H_RGB - 1 : a.H - 1;
  const int Y = ty0 + (int)(threadIdx.x >> 4), X = tx0 + 4 * (int)(threadIdx.x & 15u);
  uint32_t col[1][4] = {{0u, 0u, 0u, 0u}};
  unsigned inside;
  const unsigned hits = trail_hits<false, 4, 1>(a, f, tx0, ty0, tx1, ty1, Y, X, t, col, inside);
  if (hits == 0u) return;
  const uint32_t* px = col[0];
  unsigned char* o = pic + (((long)f * a.H + Y) * a.W + X) * 3;
  if (hits == 15u && ((uintptr_t)o & 3u) == 0u) {                    // 12 bytes: three aligned dwords, as the painters pack them
    uint32_t* o4 = (uint32_t*)o;
    o4[0] = px[0] | px[1] << 24;
    o4[1] = px[1] >> 8 | px[2] << 16;
    o4[2] = px[2] >> 16 | px[3] << 8;
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (hits >> i & 1u) {
      o[3 * i] = (unsigned char)px[i];
      o[3 * i + 1] = (unsigned char)(px[i] >> 8);
      o[3 * i + 2] = (unsigned char)(px[i] >> 16);
    }
}

struct SurfaceArgs {
  unsigned char* y;              // at frame f_off already
  unsigned char* uv;
  long y_pitch, y_stride, uv_pitch, uv_stride;                       // bytes
};

// four stored samples of a row at p (4-byte aligned): one dword (NV12) or two (P010)
template <int FMT>
__device__ __forceinline__ void put4(unsigned char* p, const uint32_t* s) {
  uint32_t* q = (uint32_t*)p;
  if (FMT == 0) {
    q[0] = s[0] | s[1] << 8 | s[2] << 16 | s[3] << 24;
  } else {
    q[0] = s[0] | s[1] << 16;
    q[1] = s[2] | s[3] << 16;
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void trails_yuv_kernel(const TrailArgs a, const SurfaceArgs s) {
  __shared__ SegList t;
  int tx, ty, f;
  tile_of(a, blockIdx.x, tx, ty, f);
  const int tx0 = tx * TILE_W, ty0 = ty * TILE_H_YUV;
  const int tx1 = tx0 + TILE_W - 1 < a.W - 1 ? tx0 + TILE_W - 1 : a.W - 1, ty1 = ty0 + TILE_H_YUV - 1 < a.H - 1 ? ty0 + TILE_H_YUV - 1 : a.H - 1;
  const int r0 = ty0 + 2 * (int)(threadIdx.x >> 4), c0 = tx0 + 4 * (int)(threadIdx.x & 15u);    // both even
  constexpr int BPS = FMT ? 2 : 1;
  uint32_t col[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
  unsigned inside;
  const unsigned hits = trail_hits<true, 4, 2>(a, f, tx0, ty0, tx1, ty1, r0, c0, t, col, inside);
  const unsigned in[2] = {inside & 15u, inside >> 4}, hit[2] = {hits & 15u, hits >> 4};   // bit k: pixel (r0 + row, c0 + k) is in the picture / has a hit
  if (hits == 0u) return;
  // luma: the rule per sample
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    if (hit[row] == 0u) continue;
    unsigned char* yr = s.y + (long)f * s.y_stride + (long)(r0 + row) * s.y_pitch;
    if (hit[row] == 15u && ((uintptr_t)(yr + (long)c0 * BPS) & 3u) == 0u) {
      uint32_t v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = stored<FMT>(comp<FMT>(col[row][k], 0));
      put4<FMT>(yr + (long)c0 * BPS, v);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (hit[row] >> k & 1u) row_put<FMT>(yr, c0 + k, stored<FMT>(comp<FMT>(col[row][k], 0)));
    }
  }
  // chroma, mdqe_annotate_yuv420sp's rule: a pair with a hit in its block is the rounded mean over the block's in-picture pixels, a hit
  // with its colour's component and any other pixel with the stored sample's value
  unsigned char* cr = s.uv + (long)f * s.uv_stride + (long)(r0 >> 1) * s.uv_pitch;
  uint32_t c[4] = {0u, 0u, 0u, 0u};
  bool wr[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const unsigned m = 3u << 2 * p;
    wr[p] = ((hit[0] | hit[1]) & m) != 0u;
    if (!wr[p]) continue;
    const uint32_t U = value_of<FMT>(row_raw<FMT>(cr, c0 + 2 * p)), V = value_of<FMT>(row_raw<FMT>(cr, c0 + 2 * p + 1));
    uint32_t su = 0u, sv = 0u;
#pragma unroll
    for (int row = 0; row < 2; ++row)
#pragma unroll
      for (int k = 2 * p; k < 2 * p + 2; ++k)
        if (in[row] >> k & 1u) {
          const bool h = hit[row] >> k & 1u;
          su += h ? comp<FMT>(col[row][k], 1) : U;
          sv += h ? comp<FMT>(col[row][k], 2) : V;
        }
    const uint32_t n = (uint32_t)(__popc(in[0] & m) + __popc(in[1] & m)), sh = n >> 1;   // n is 1, 2 or 4: (sum + n / 2) >> log2(n)
    c[2 * p] = stored<FMT>((su + sh) >> sh);
    c[2 * p + 1] = stored<FMT>((sv + sh) >> sh);
  }
  if (wr[0] && wr[1] && ((uintptr_t)(cr + (long)c0 * BPS) & 3u) == 0u) {
    put4<FMT>(cr + (long)c0 * BPS, c);
  } else {
#pragma unroll
    for (int p = 0; p < 2; ++p)
      if (wr[p]) {
        row_put<FMT>(cr, c0 + 2 * p, c[2 * p]);
        row_put<FMT>(cr, c0 + 2 * p + 1, c[2 * p + 1]);
      }
  }
}

// The checks both trail entries share, made before any pointer is looked at.  `done`: the call is valid and launches nothing.
inline int trails_call(int F, int H, int W, int f_off, long pts_row_stride, int p_off, int n, int trail, int width, bool& done) {
  MDQE_REQUIRE(trail >= 1 && trail <= 64 && width >= 1 && width <= 5 && n >= 0 && n <= 255);
  MDQE_REQUIRE(F >= 0 && f_off >= 0 && p_off >= 0 && H > 0 && W > 0 && H <= 16384 && W <= 16384);   // (the hit test's 64-bit products)
  MDQE_REQUIRE((long)F * ((long)H * W) < 0x7FFFFFFFL);               // the block index of one call is 32-bit
  if (n > 1) MDQE_REQUIRE(pts_row_stride >= 2L * ((long)p_off + F)); // (a row's columns end before the next row)
  done = F == 0 || n == 0;
  return MDQE_OK;
}

inline unsigned set_args(TrailArgs& a, const int* pts, long pts_row_stride, int p_off, const void* palette, int F, int H, int W, int n,
                         int trail, int width, int tile_h) {
  a.pts = pts; a.palette = palette; a.pts_row_stride = pts_row_stride;
  a.F = F; a.H = H; a.W = W; a.n = n; a.p_off = p_off; a.trail = trail; a.width = width;
  a.tiles_x = (unsigned)((W + TILE_W - 1) / TILE_W);
  a.tiles_y = (unsigned)((H + tile_h - 1) / tile_h);
  return (unsigned)F * a.tiles_y * a.tiles_x;                        // <= F * H * W < 2^31
}

}  // namespace

extern "C" int mdqe_label_centroids_u8(const unsigned char* labels, int F, int Ho, int Wo, int n, int min_area, long long* mom,
                                       int* pts, long pts_row_stride, int p_off, void* stream) {
  MDQE_REQUIRE(n >= 0 && n <= 255 && min_area >= 0 && F >= 0 && Ho > 0 && Wo > 0 && Ho <= 16384 && Wo <= 16384 && p_off >= 0);
  MDQE_REQUIRE((long)F * ((long)Ho * Wo) < 0x7FFFFFFFL);
  if (n > 1) MDQE_REQUIRE(pts_row_stride >= 2L * ((long)p_off + F)); // (two writers otherwise)
  if (n == 0 || F == 0) return MDQE_OK;
  MDQE_CHECK_PTR(labels);
  MDQE_CHECK_PTR(mom);
  const int count = n * F;                                           // <= 255 * F < 2^31: F * Ho * Wo is
  const unsigned bands = (unsigned)((Ho + BAND - 1) / BAND);
  unsigned long long* m = (unsigned long long*)mom;
  mdqe_clear_error();
  hipLaunchKernelGGL(moments_zero_kernel, dim3((unsigned)((3L * count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, 3 * count);
  hipLaunchKernelGGL(moments_sweep_kernel, dim3((unsigned)F * bands), dim3(256), 0, (hipStream_t)stream, labels, F, Ho, Wo, n, bands, m);
  if (pts != nullptr)
    hipLaunchKernelGGL(centroid_points_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, F, count,
                       min_area, pts, pts_row_stride, p_off);
  return mdqe_launch_status();
}

extern "C" int mdqe_render_trails_u8(unsigned char* pic, int F, int Ho, int Wo, int f_off, const int* pts, long pts_row_stride, int p_off,
                                     int n, int trail, int width, const unsigned char* palette, void* stream) {
  bool done = false;
  const int st = trails_call(F, Ho, Wo, f_off, pts_row_stride, p_off, n, trail, width, done);
  if (st != MDQE_OK || done) return st;
  MDQE_CHECK_PTR(pic);
  MDQE_CHECK_PTR(pts);
  MDQE_CHECK_PTR(palette);
  TrailArgs a;
  const unsigned blocks = set_args(a, pts, pts_row_stride, p_off, palette, F, Ho, Wo, n, trail, width, TILE_H_RGB);
  mdqe_clear_error();
  hipLaunchKernelGGL(trails_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, pic + (long)f_off * Ho * Wo * 3);
  return mdqe_launch_status();
}

extern "C" int mdqe_render_trails_yuv420sp(void* y, long y_pitch, long y_stride, void* uv, long uv_pitch, long uv_stride,
                                           int F, int H, int W, int fmt, int f_off, const int* pts, long pts_row_stride, int p_off,
                                           int n, int trail, int width, const unsigned short* palette_yuv, void* stream) {
  bool done = false;
  const int st = trails_call(F, H, W, f_off, pts_row_stride, p_off, n, trail, width, done);
  if (st != MDQE_OK) return st;
  // the surface conditions of mdqe_annotate_yuv420sp, for planes that are both read and written
  MDQE_REQUIRE(fmt == 0 || fmt == 1);
  const long bps = fmt ? 2 : 1, yb = bps * W, cb = bps * 2 * ((W + 1L) / 2), CH = (H + 1L) / 2;
  MDQE_REQUIRE(y_pitch >= yb && uv_pitch >= cb && y_stride >= 0 && uv_stride >= 0);
  if (fmt == 1) MDQE_REQUIRE(((y_pitch | y_stride | uv_pitch | uv_stride) & 1L) == 0);
  if (F > 1) MDQE_REQUIRE(y_stride >= (H - 1) * y_pitch + yb && uv_stride >= (CH - 1) * uv_pitch + cb);
  if (done) return MDQE_OK;
  MDQE_CHECK_PTR(y);
  MDQE_CHECK_PTR(uv);
  MDQE_CHECK_PTR(pts);
  MDQE_CHECK_PTR(palette_yuv);
  MDQE_REQUIRE(((uintptr_t)palette_yuv & 1u) == 0);
  if (fmt == 1) MDQE_REQUIRE((((uintptr_t)y | (uintptr_t)uv) & 1u) == 0);
  SurfaceArgs s;
  s.y = (unsigned char*)y + (long)f_off * y_stride;
  s.uv = (unsigned char*)uv + (long)f_off * uv_stride;
  s.y_pitch = y_pitch; s.y_stride = y_stride; s.uv_pitch = uv_pitch; s.uv_stride = uv_stride;
  MDQE_REQUIRE(apart(plane_of(s.y, y_pitch, y_stride, F, H, yb), plane_of(s.uv, uv_pitch, uv_stride, F, CH, cb)));   // (two writers otherwise)
  TrailArgs a;
  const unsigned blocks = set_args(a, pts, pts_row_stride, p_off, palette_yuv, F, H, W, n, trail, width, TILE_H_YUV);
  mdqe_clear_error();
  if (fmt == 0) hipLaunchKernelGGL(trails_yuv_kernel<0>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, s);
  else hipLaunchKernelGGL(trails_yuv_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, s);
  return mdqe_launch_status();
}
