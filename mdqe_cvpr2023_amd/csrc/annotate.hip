// Track boxes and captions on a painted overlay: an annotation pass that runs behind a painter, in place, on the same stream.  ONE
// definition, integers only (include/mdqe_hip.h has the rule); tests/_annotate_ref.py restates it in numpy as a painter's algorithm
// and every comparison is exact.  What it draws comes from the geometry table mdqe_final_label_map_u8 writes in its own sweep (per label
// and frame the visible region's area and box) and from small host-made tables (captions, font, palette, ink): nothing is read back.
//
// A block owns a tile of the picture: 64 x 16 pixels of an RGB picture (a thread: 4 pixels of a row, 12 bytes), 64 x 32 of a surface (a
// thread: 2 rows x 4 columns, the rows that share a chroma row, so each chroma pair has ONE writer which holds the four hits that decide
// it -- the surface painters' ownership).  First thread k looks at label k + 1 (n <= 255 < 256 threads): is its row of the table live, do
// its plate and its box frame meet the tile (a tile that lies wholly inside a box's interior does not meet its frame).  The flagged
// rectangles are compacted into LDS in label order -- a ballot per wave, the lane's rank among the lanes below it, the waves' counts
// through LDS -- into two lists of capacity 255 each, the plates and the frames, with their colours packed beside them.  A tile whose
// lists are empty returns there, before any pixel is read or written: on real video that is most tiles.  Otherwise a thread walks the
// plates and then the frames ONCE for its 4 or 8 pixels: an entry that misses them all costs one rectangle test, one that meets them is
// tested on the pixels nothing has hit yet -- each pixel's first hit in list order, which IS the rule's priority since both lists
// ascend by label.  No pixel loops over all labels.
// Stores: a pixel without a hit is not written.  Four hit pixels of an RGB row at a 4-byte aligned address are three dword stores, four
// hit luma samples one or two dwords, two hit chroma pairs likewise; anything else goes out sample by sample.  The alignment is looked
// at per address, so every pitch, width and offset is accepted.  A chroma pair with a hit reads the stored pair, which only this thread
// writes: in place by construction.  No atomics, no data-dependent order: identical from run to run.
// render_rule.h gives the colour packings, the stored-sample helpers and the plane overlap test this file shares with the painters.
#include "render_rule.h"

namespace {

constexpr int TILE_W = 64, TILE_H_RGB = 16, TILE_H_YUV = 32;         // 256 threads: 16 units of 4 columns x 16 rows / row pairs
constexpr int CAP = 255;                                             // every label of a frame may meet one tile

struct AnnotateArgs {
  const int* geom;               // [n * F, 5]: row k * F + f = (area, xmin, ymin, xmax, ymax)
  const void* palette;           // uint8 [256, 3] (RGB) or uint16 [256, 3] (surfaces)
  const void* ink;               // the same layout
  const unsigned char* captions; // [256, cap_len] or unused
  const unsigned char* font;     // [64, 7]
  int F, H, W, n, cap_len, box, scale, min_area;
  unsigned tiles_x, tiles_y;
};

struct TileList {
  int4 plate[CAP];               // px, py, width, label -- ascending label
  uint32_t plate_col[CAP], plate_ink[CAP];
  int4 frame[CAP];               // x0, y0, x1, y1 -- ascending label
  uint32_t frame_col[CAP];
  int wave_plates[4], wave_frames[4];
  unsigned char font[64 * 7];
};

template <bool YUV>
__device__ __forceinline__ uint32_t pack_row(const void* table, int l) {
  return YUV ? pack_yuv((const unsigned short*)table + 3 * l) : pack_rgb((const unsigned char*)table + 3 * l);
}

// The lists of tile [tx0, tx1] x [ty0, ty1] of frame f.  Every thread of the block calls it; -> the counts; both 0: nothing to draw.
template <bool YUV>
__device__ __forceinline__ void build_list(const AnnotateArgs& a, int f, int tx0, int ty0, int tx1, int ty1, TileList& t, int& np, int& nf) {
  const int k = (int)threadIdx.x;                                    // label k + 1
  bool plate = false, frame = false;
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0, px = 0, py = 0, w = 0;
  if (k < a.n) {
    const int* g = a.geom + ((long)k * a.F + f) * 5;
    const int area = g[0];
    x0 = g[1]; y0 = g[2]; x1 = g[3]; y1 = g[4];
    // live: every later expression stays inside the picture's coordinates whatever the table holds
    const bool live = area >= (a.min_area > 1 ? a.min_area : 1) && 0 <= x0 && x0 <= x1 && x1 < a.W && 0 <= y0 && y0 <= y1 && y1 < a.H;
    if (live && a.box > 0) {
      const bool inside = tx0 >= x0 + a.box && tx1 <= x1 - a.box && ty0 >= y0 + a.box && ty1 <= y1 - a.box;   // the tile sees the interior only
      frame = x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0 && !inside;
    }
    if (live && a.cap_len > 0) {
      const int h = 9 * a.scale;
      py = y0 - h >= 0 ? y0 - h : y0;
      if (py <= ty1 && py + h - 1 >= ty0) {                          // (the text is looked at only by the tiles of the plate's rows)
        const unsigned char* row = a.captions + (long)(k + 1) * a.cap_len;
        int c = 0;
        for (int j = 0; j < a.cap_len && c == j; j += 8) {           // 8 bytes at a time: loads that do not wait for each other
          unsigned char b[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) b[q] = j + q < a.cap_len ? row[j + q] : (unsigned char)0;
          int z = 8;                                                 // the first 0 byte of the eight, 8: none
#pragma unroll
          for (int q = 7; q >= 0; --q) z = b[q] == 0 ? q : z;
          c = j + z;
        }
        c = c < a.cap_len ? c : a.cap_len;
        w = (6 * c + 1) * a.scale;
        px = x0 < a.W - w ? x0 : a.W - w;
        px = px > 0 ? px : 0;
        plate = c > 0 && px <= tx1 && px + w - 1 >= tx0;
      }
    }
  }
  const unsigned long long bp = __ballot(plate), bf = __ballot(frame);
  const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
  if (lane == 0) {
    t.wave_plates[wv] = __popcll(bp);
    t.wave_frames[wv] = __popcll(bf);
  }
  __syncthreads();
  int p_at = 0, f_at = 0;
  np = nf = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < wv) { p_at += t.wave_plates[i]; f_at += t.wave_frames[i]; }
    np += t.wave_plates[i];
    nf += t.wave_frames[i];
  }
  if (np + nf == 0) return;                                          // (block-uniform)
  const unsigned long long below = (1ull << lane) - 1ull;
  if (plate) {
    const int i = p_at + __popcll(bp & below);
    t.plate[i] = make_int4(px, py, w, k + 1);
    t.plate_col[i] = pack_row<YUV>(a.palette, k + 1);
    t.plate_ink[i] = pack_row<YUV>(a.ink, k + 1);
  }
  if (frame) {
    const int i = f_at + __popcll(bf & below);
    t.frame[i] = make_int4(x0, y0, x1, y1);
    t.frame_col[i] = pack_row<YUV>(a.palette, k + 1);
  }
  if (np > 0)
    for (int i = (int)threadIdx.x; i < 64 * 7; i += 256) t.font[i] = a.font[i];
  __syncthreads();
}

// The rule on the thread's NX x NY pixels whose top left one is (Y, X); (yl, xl) is the tile's last pixel inside the picture.  The lists
// are walked ONCE per thread: an entry whose rectangle (a frame: whose ring) misses the thread's pixels costs one test, and only an
// entry that meets them is tested pixel by pixel, on the pixels no earlier entry has hit -- the first hit in list order, as the rule
// says.  -> bit row * NX + k set: pixel (Y + row, X + k) is hit, its colour in col[row][k].
template <int NX, int NY>
__device__ __forceinline__ unsigned hits_of(const AnnotateArgs& a, const TileList& t, int np, int nf, int Y, int X, int yl, int xl,
                                            uint32_t (&col)[NY][NX], unsigned& inside) {
  const int X1 = X + NX - 1 < xl ? X + NX - 1 : xl, Y1 = Y + NY - 1 < yl ? Y + NY - 1 : yl, h = 9 * a.scale;
  unsigned todo = 0u, hit = 0u;
#pragma unroll
  for (int row = 0; row < NY; ++row)
#pragma unroll
    for (int k = 0; k < NX; ++k)
      if (Y + row <= yl && X + k <= xl) todo |= 1u << (row * NX + k);
  inside = todo;
  for (int i = 0; i < np && todo != 0u; ++i) {
    const int4 p = t.plate[i];
    if (X1 < p.x || X >= p.x + p.z || Y1 < p.y || Y >= p.y + h) continue;
#pragma unroll
    for (int row = 0; row < NY; ++row)
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const unsigned bit = 1u << (row * NX + k);
        const unsigned u = (unsigned)(X + k - p.x), v = (unsigned)(Y + row - p.y);
        if ((todo & bit) != 0u && u < (unsigned)p.z && v < (unsigned)h) {
          const int gx = (int)(u / (unsigned)a.scale) - 1, gy = (int)(v / (unsigned)a.scale) - 1;
          bool ink = false;
          if (gx >= 0 && gy >= 0 && gy < 7 && gx % 6 < 5) {          // (u < (6c + 1) * scale: gx / 6 < c <= cap_len)
            unsigned ch = a.captions[(long)p.w * a.cap_len + gx / 6];
            if (ch < 0x20u || ch > 0x5Fu) ch = 0x3Fu;                // '?'
            ink = (t.font[(ch - 32u) * 7u + (unsigned)gy] >> (4 - gx % 6)) & 1u;
          }
          col[row][k] = ink ? t.plate_ink[i] : t.plate_col[i];
          hit |= bit;
          todo &= ~bit;
        }
      }
  }
  for (int i = 0; i < nf && todo != 0u; ++i) {
    const int4 r = t.frame[i];
    if (X1 < r.x || X > r.z || Y1 < r.y || Y > r.w) continue;
    if (X >= r.x + a.box && X1 <= r.z - a.box && Y >= r.y + a.box && Y1 <= r.w - a.box) continue;     // the box's interior
#pragma unroll
    for (int row = 0; row < NY; ++row)
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        const unsigned bit = 1u << (row * NX + k);
        const int x = X + k, y = Y + row;
        const int dx = x - r.x < r.z - x ? x - r.x : r.z - x, dy = y - r.y < r.w - y ? y - r.y : r.w - y;   // (negative outside the box)
        if ((todo & bit) != 0u && dx >= 0 && dy >= 0 && (dx < dy ? dx : dy) < a.box) {
          col[row][k] = t.frame_col[i];
          hit |= bit;
          todo &= ~bit;
        }
      }
  }
  return hit;
}

// -> the tile's column, row and frame of block b
__device__ __forceinline__ void tile_of(const AnnotateArgs& a, unsigned b, int& tx, int& ty, int& f) {
  const unsigned row = b / a.tiles_x;
  tx = (int)(b - row * a.tiles_x);
  f = (int)(row / a.tiles_y);
  ty = (int)(row - (unsigned)f * a.tiles_y);
}

__global__ __launch_bounds__(256) void annotate_u8_kernel(const AnnotateArgs a, unsigned char* pic) {
  __shared__ TileList t;
  int tx, ty, f, np, nf;
  tile_of(a, blockIdx.x, tx, ty, f);
  const int tx0 = tx * TILE_W, ty0 = ty * TILE_H_RGB;
  const int tx1 = tx0 + TILE_W - 1 < a.W - 1 ? tx0 + TILE_W - 1 : a.W - 1, ty1 = ty0 + TILE_H_RGB - 1 < a.H - 1 ? ty0 + TILE_H_RGB - 1 : a.H - 1;
  build_list<false>(a, f, tx0, ty0, tx1, ty1, t, np, nf);
  if (np + nf == 0) return;
  const int Y = ty0 + (int)(threadIdx.x >> 4), X = tx0 + 4 * (int)(threadIdx.x & 15u);
  if (Y > ty1 || X > tx1) return;
  uint32_t col[1][4] = {{0u, 0u, 0u, 0u}};
  unsigned inside;
  const unsigned hits = hits_of<4, 1>(a, t, np, nf, Y, X, ty1, tx1, col, inside);
  const uint32_t* px = col[0];
  if (hits == 0u) return;
  unsigned char* o = pic + (((long)f * a.H + Y) * a.W + X) * 3;
  if (hits == 15u && ((uintptr_t)o & 3u) == 0u) {                    // 12 bytes: three aligned dwords, as the painter packs them
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
__global__ __launch_bounds__(256) void annotate_yuv_kernel(const AnnotateArgs a, const SurfaceArgs s) {
  __shared__ TileList t;
  int tx, ty, f, np, nf;
  tile_of(a, blockIdx.x, tx, ty, f);
  const int tx0 = tx * TILE_W, ty0 = ty * TILE_H_YUV;
  const int tx1 = tx0 + TILE_W - 1 < a.W - 1 ? tx0 + TILE_W - 1 : a.W - 1, ty1 = ty0 + TILE_H_YUV - 1 < a.H - 1 ? ty0 + TILE_H_YUV - 1 : a.H - 1;
  build_list<true>(a, f, tx0, ty0, tx1, ty1, t, np, nf);
  if (np + nf == 0) return;
  const int r0 = ty0 + 2 * (int)(threadIdx.x >> 4), c0 = tx0 + 4 * (int)(threadIdx.x & 15u);    // both even
  if (r0 > ty1 || c0 > tx1) return;
  constexpr int BPS = FMT ? 2 : 1;
  uint32_t col[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
  unsigned inside;
  const unsigned hits = hits_of<4, 2>(a, t, np, nf, r0, c0, ty1, tx1, col, inside);
  const unsigned in[2] = {inside & 15u, inside >> 4}, hit[2] = {hits & 15u, hits >> 4};   // bit k: pixel (r0 + row, c0 + k) is in the picture / has a hit
  if ((hit[0] | hit[1]) == 0u) return;
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
  // chroma: a pair with a hit in its block is the rounded mean over the block's in-picture pixels, a hit with its colour's component
  // and any other pixel with the stored sample's value
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

// The checks both entries share, made before any pointer is looked at.  `done`: the call is valid and launches nothing.
inline int annotate_call(int F, int H, int W, int f_off, int n, int cap_len, int box, int scale, int min_area, bool& done) {
  MDQE_REQUIRE(box >= 0 && box <= 4 && scale >= 1 && scale <= 4 && n >= 0 && n <= 255 && cap_len >= 0 && cap_len <= 64 && min_area >= 0);
  MDQE_REQUIRE(F >= 0 && f_off >= 0 && H > 0 && W > 0);
  MDQE_REQUIRE((long)H * W < 0x7FFFFFFFL && (long)F * ((long)H * W) < 0x7FFFFFFFL);   // the block index of one call is 32-bit
  done = F == 0 || n == 0 || (box == 0 && cap_len == 0);
  return MDQE_OK;
}

inline int annotate_tables(const int* geom, const void* palette, const void* ink, const unsigned char* captions, int cap_len,
                           const unsigned char* font) {
  MDQE_CHECK_PTR(geom);
  MDQE_CHECK_PTR(palette);
  if (cap_len > 0) {
    MDQE_CHECK_PTR(ink);
    MDQE_CHECK_PTR(captions);
    MDQE_CHECK_PTR(font);
  }
  return MDQE_OK;
}

inline unsigned set_args(AnnotateArgs& a, const int* geom, const void* palette, const void* ink, const unsigned char* captions,
                         const unsigned char* font, int F, int H, int W, int n, int cap_len, int box, int scale, int min_area, int tile_h) {
  a.geom = geom; a.palette = palette; a.ink = ink; a.captions = captions; a.font = font;
  a.F = F; a.H = H; a.W = W; a.n = n; a.cap_len = cap_len; a.box = box; a.scale = scale; a.min_area = min_area;
  a.tiles_x = (unsigned)((W + TILE_W - 1) / TILE_W);
  a.tiles_y = (unsigned)((H + tile_h - 1) / tile_h);
  return (unsigned)F * a.tiles_y * a.tiles_x;                        // <= F * H * W < 2^31
}

}  // namespace

extern "C" int mdqe_annotate_u8(unsigned char* pic, int F, int Ho, int Wo, int f_off, const int* geom, int n,
                                const unsigned char* palette, const unsigned char* ink,
                                const unsigned char* captions, int cap_len, const unsigned char* font,
                                int box, int scale, int min_area, void* stream) {
  bool done = false;
  const int st = annotate_call(F, Ho, Wo, f_off, n, cap_len, box, scale, min_area, done);
  if (st != MDQE_OK || done) return st;
  MDQE_CHECK_PTR(pic);
  const int tb = annotate_tables(geom, palette, ink, captions, cap_len, font);
  if (tb != MDQE_OK) return tb;
  AnnotateArgs a;
  const unsigned blocks = set_args(a, geom, palette, ink, captions, font, F, Ho, Wo, n, cap_len, box, scale, min_area, TILE_H_RGB);
  mdqe_clear_error();
  hipLaunchKernelGGL(annotate_u8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, pic + (long)f_off * Ho * Wo * 3);
  return mdqe_launch_status();
}

extern "C" int mdqe_annotate_yuv420sp(void* y, long y_pitch, long y_stride, void* uv, long uv_pitch, long uv_stride,
                                      int F, int H, int W, int fmt, int f_off, const int* geom, int n,
                                      const unsigned short* palette_yuv, const unsigned short* ink_yuv,
                                      const unsigned char* captions, int cap_len, const unsigned char* font,
                                      int box, int scale, int min_area, void* stream) {
  bool done = false;
  const int st = annotate_call(F, H, W, f_off, n, cap_len, box, scale, min_area, done);
  if (st != MDQE_OK) return st;
  // the surface conditions of mdqe_render_overlay_yuv420sp, for planes that are both read and written
  MDQE_REQUIRE(fmt == 0 || fmt == 1);
  const long bps = fmt ? 2 : 1, yb = bps * W, cb = bps * 2 * ((W + 1L) / 2), CH = (H + 1L) / 2;
  MDQE_REQUIRE(y_pitch >= yb && uv_pitch >= cb && y_stride >= 0 && uv_stride >= 0);
  if (fmt == 1) MDQE_REQUIRE(((y_pitch | y_stride | uv_pitch | uv_stride) & 1L) == 0);
  if (F > 1) MDQE_REQUIRE(y_stride >= (H - 1) * y_pitch + yb && uv_stride >= (CH - 1) * uv_pitch + cb);
  if (done) return MDQE_OK;
  MDQE_CHECK_PTR(y);
  MDQE_CHECK_PTR(uv);
  const int tb = annotate_tables(geom, palette_yuv, ink_yuv, captions, cap_len, font);
  if (tb != MDQE_OK) return tb;
  MDQE_REQUIRE(((uintptr_t)palette_yuv & 1u) == 0 && ((uintptr_t)ink_yuv & 1u) == 0);
  if (fmt == 1) MDQE_REQUIRE((((uintptr_t)y | (uintptr_t)uv) & 1u) == 0);
  SurfaceArgs s;
  s.y = (unsigned char*)y + (long)f_off * y_stride;
  s.uv = (unsigned char*)uv + (long)f_off * uv_stride;
  s.y_pitch = y_pitch; s.y_stride = y_stride; s.uv_pitch = uv_pitch; s.uv_stride = uv_stride;
  MDQE_REQUIRE(apart(plane_of(s.y, y_pitch, y_stride, F, H, yb), plane_of(s.uv, uv_pitch, uv_stride, F, CH, cb)));   // (two writers otherwise)
  AnnotateArgs a;
  const unsigned blocks = set_args(a, geom, palette_yuv, ink_yuv, captions, font, F, H, W, n, cap_len, box, scale, min_area, TILE_H_YUV);
  mdqe_clear_error();
  if (fmt == 0) hipLaunchKernelGGL(annotate_yuv_kernel<0>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, s);
  else hipLaunchKernelGGL(annotate_yuv_kernel<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, s);
  return mdqe_launch_status();
}
