// Per-track crops: one fixed-size chip per track and frame, cut from the frames the caller handed in and resized, on the device.  ONE
// definition, integers only (include/mdqe_hip.h has the rule); tests/_crops_ref.py restates it in numpy loops and every comparison is
// exact.  What is cut comes from the geometry table mdqe_final_label_map_u8 writes in its own sweep and, with cutout, from the label map
// itself: nothing is read back.
//
// A block of 256 threads owns 256 consecutive pixels of ONE chip (block -> (row k, taken frame t, tile)), so the chip's rect, whether it
// is live and which split sums its footprints are block-uniform.  The rect is derived by every thread from the table's row (5 cached
// dwords): no LDS, no barrier.  Footprints range from one source pixel (a box smaller than the chip: replication) to the whole picture
// (a 1 x 1 chip), so there are two splits, chosen per chip from an upper bound of its footprints, fh * fw with fh = ceil(ch / Sh) + 1:
//   <= 256 source pixels   a thread owns a chip pixel and walks its footprint row by row;
//   more                   a wave owns a chip pixel (the block's four waves take its 256 pixels in turn), its lanes stride the footprint
//                          in row-major order -- consecutive lanes on consecutive source columns -- and a butterfly of shuffles adds
//                          the four partial sums (three channels and the count).
// The sums are integers (uint32: fewer than 2^24 bytes), so either split gives the rule's bits.  Thread mode is the common case (a 640 x
// 360 picture into a 128 x 64 chip: at most 4 x 11 source pixels); below 256 its serial walk is shorter than the wave form's 64 chip
// pixels x (ceil(fp / 64) strides + the reduction).  Stores are single bytes: a chip is a few KB against the source pixels read for it.
// No atomics, no data-dependent order: identical from run to run.
#include "render_rule.h"

namespace {

constexpr int THREAD_MODE_MAX = 256;   // footprints of at most this many source pixels: one thread per chip pixel

struct CropArgs {
  const unsigned char* labels;   // [F, Ho, Wo]
  const int* geom;               // [n * F, 5]: row k * F + f = (area, xmin, ymin, xmax, ymax)
  unsigned char* out;
  int* rects;
  long out_row_stride, rect_row_stride;
  int F, Ho, Wo, n, Fc, f_first, f_step, Sh, Sw, pad256, min_area, cutout, c_off;
  uint32_t fill;                 // c0 | c1 << 8 | c2 << 16
  unsigned tiles;                // blocks per chip: ceil(Sh * Sw / 256)
};

struct YuvSource {
  const unsigned char* y;
  const unsigned char* uv;
  long y_pitch, y_stride, uv_pitch, uv_stride;   // bytes
  int h0, w0, bgr;
  int yo, co, cy, rv, gu, gv, bu;
};

// clamp(x >> 16, 0, 255) in the order csrc/yuv.hip gives its reasons for
__device__ __forceinline__ uint32_t clamp8(int x) {
  x = x < 0 ? 0 : (x > 0xFFFFFF ? 0xFFFFFF : x);
  return (uint32_t)x >> 16;
}

// The source pixel (sy, sx) of frame f as c0 | c1 << 8 | c2 << 16.  KIND 1: uint8 planes, 2: float32 planes, 3: NV12, 4: P010.
template <int KIND>
struct Source;

template <> struct Source<1> { typedef RgbSource type; };
template <> struct Source<2> { typedef RgbSource type; };
template <> struct Source<3> { typedef YuvSource type; };
template <> struct Source<4> { typedef YuvSource type; };

template <int KIND>
__device__ __forceinline__ uint32_t fetch(const RgbSource& s, int f, int sy, int sx) {
  return src_px<KIND>(s, (long)f * s.frame_stride + (long)sy * s.w0 + sx);
}

template <int KIND>
__device__ __forceinline__ uint32_t fetch(const YuvSource& s, int f, int sy, int sx) {
  constexpr int FMT = KIND - 3;
  const unsigned char* yr = s.y + (long)f * s.y_stride + (long)sy * s.y_pitch;
  const unsigned char* cr = s.uv + (long)f * s.uv_stride + (long)(sy >> 1) * s.uv_pitch;
  const int Y = (int)value_of<FMT>(row_raw<FMT>(yr, sx));
  const int cu = (int)value_of<FMT>(row_raw<FMT>(cr, 2 * (sx >> 1))) - s.co, cv = (int)value_of<FMT>(row_raw<FMT>(cr, 2 * (sx >> 1) + 1)) - s.co;
  const int yy = (Y - s.yo) * s.cy;
  const uint32_t R = clamp8(yy + s.rv * cv + 32768), G = clamp8(yy + s.gu * cu + s.gv * cv + 32768), B = clamp8(yy + s.bu * cu + 32768);
  return s.bgr ? (B | G << 8 | R << 16) : (R | G << 8 | B << 16);
}

struct Sums { uint32_t c0, c1, c2, m; };

__device__ __forceinline__ void count(Sums& a, uint32_t px) {
  a.c0 += px & 0xFFu;
  a.c1 += (px >> 8) & 0xFFu;
  a.c2 += px >> 16;
  a.m += 1u;
}

// the footprint bounds of chip index i along an axis of `len` source pixels from `lo`, chip size S (i * len may pass 2^31)
__device__ __forceinline__ void span_of(int i, int len, int S, int lo, int& a, int& b) {
  a = lo + (int)((unsigned long long)i * (unsigned)len / (unsigned)S);
  b = lo + (int)(((unsigned long long)(i + 1) * (unsigned)len + (unsigned)(S - 1)) / (unsigned)S);
}

template <int KIND>
__global__ __launch_bounds__(256) void track_crops_kernel(const CropArgs a, const typename Source<KIND>::type s) {
  const unsigned chip = blockIdx.x / a.tiles, tile = blockIdx.x - chip * a.tiles;
  const int k = (int)(chip / (unsigned)a.Fc), t = (int)(chip - (unsigned)k * (unsigned)a.Fc);
  const int f = a.f_first + t * a.f_step;                           // < F: Fc counts exactly those
  const int* g = a.geom + ((long)k * a.F + f) * 5;
  const int area = g[0], xmin = g[1], ymin = g[2], xmax = g[3], ymax = g[4];
  // live: every later expression stays inside the picture's coordinates whatever the table holds
  const bool live = area >= (a.min_area > 1 ? a.min_area : 1) && 0 <= xmin && xmin <= xmax && xmax < a.Wo && 0 <= ymin && ymin <= ymax && ymax < a.Ho;
  const int npx = a.Sh * a.Sw, first = (int)tile * 256;
  unsigned char* chip_out = a.out + (long)k * a.out_row_stride + (long)(a.c_off + t) * npx * 3;
  int X0 = 0, Y0 = 0, X1 = -1, Y1 = -1;
  if (live) {
    const int px = (int)(((unsigned)(xmax - xmin + 1) * (unsigned)a.pad256 + 128u) >> 8);   // (width < 2^24: < 2^32)
    const int py = (int)(((unsigned)(ymax - ymin + 1) * (unsigned)a.pad256 + 128u) >> 8);
    X0 = xmin - px > 0 ? xmin - px : 0;                             // (px <= width <= Wo: no overflow)
    X1 = xmax + px < a.Wo - 1 ? xmax + px : a.Wo - 1;
    Y0 = ymin - py > 0 ? ymin - py : 0;
    Y1 = ymax + py < a.Ho - 1 ? ymax + py : a.Ho - 1;
  }
  if (tile == 0u && threadIdx.x == 0u) {
    int* r = a.rects + (long)k * a.rect_row_stride + (long)(a.c_off + t) * 4;
    r[0] = X0; r[1] = Y0; r[2] = X1; r[3] = Y1;
  }
  const uint32_t fill = a.fill;
  if (!live) {                                                       // (block-uniform)
    const int p = first + (int)threadIdx.x;
    if (p < npx) {
      unsigned char* o = chip_out + (long)p * 3;
      o[0] = (unsigned char)fill; o[1] = (unsigned char)(fill >> 8); o[2] = (unsigned char)(fill >> 16);
    }
    return;
  }
  const int cw = X1 - X0 + 1, ch = Y1 - Y0 + 1;
  const unsigned char* lab = a.labels + (long)f * a.Ho * a.Wo;
  const uint32_t own = (uint32_t)(k + 1);
  const bool ident = s.h0 == a.Ho && s.w0 == a.Wo;
  const long fh = (ch + a.Sh - 1) / a.Sh + 1, fw = (cw + a.Sw - 1) / a.Sw + 1;      // bounds of Yb - Ya, Xb - Xa
  if (fh * fw <= THREAD_MODE_MAX) {
    const int p = first + (int)threadIdx.x;
    if (p >= npx) return;
    const int i = p / a.Sw, j = p - i * a.Sw;
    int Ya, Yb, Xa, Xb;
    span_of(i, ch, a.Sh, Y0, Ya, Yb);
    span_of(j, cw, a.Sw, X0, Xa, Xb);
    Sums acc = {0u, 0u, 0u, 0u};
    for (int Y = Ya; Y < Yb; ++Y) {
      const int sy = ident ? Y : (int)((unsigned)Y * (unsigned)s.h0 / (unsigned)a.Ho);
      const unsigned char* lr = lab + (long)Y * a.Wo;
      for (int X = Xa; X < Xb; ++X) {
        if (a.cutout && lr[X] != own) continue;
        const int sx = ident ? X : (int)((unsigned)X * (unsigned)s.w0 / (unsigned)a.Wo);
        count(acc, fetch<KIND>(s, f, sy, sx));
      }
    }
    uint32_t v = fill;
    if (acc.m != 0u) {
      const uint32_t h = acc.m >> 1;                                 // (sum <= 255 * m, m < 2^24: sum + m / 2 < 2^32)
      v = (acc.c0 + h) / acc.m | (acc.c1 + h) / acc.m << 8 | (acc.c2 + h) / acc.m << 16;
    }
    unsigned char* o = chip_out + (long)p * 3;
    o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16);
    return;
  }
  // a wave per chip pixel: wave w takes pixels first + w, first + w + 4, ...; every lane of a wave sees the same pixel
  const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
  for (int p = first + wv; p < first + 256 && p < npx; p += 4) {
    const int i = p / a.Sw, j = p - i * a.Sw;
    int Ya, Yb, Xa, Xb;
    span_of(i, ch, a.Sh, Y0, Ya, Yb);
    span_of(j, cw, a.Sw, X0, Xa, Xb);
    const unsigned wd = (unsigned)(Xb - Xa), total = (unsigned)(Yb - Ya) * wd;      // <= Ho * Wo < 2^24
    Sums acc = {0u, 0u, 0u, 0u};
    for (unsigned q = (unsigned)lane; q < total; q += 64u) {
      const unsigned r = q / wd;
      const int Y = Ya + (int)r, X = Xa + (int)(q - r * wd);
      if (a.cutout && lab[(long)Y * a.Wo + X] != own) continue;
      const int sy = ident ? Y : (int)((unsigned)Y * (unsigned)s.h0 / (unsigned)a.Ho);
      const int sx = ident ? X : (int)((unsigned)X * (unsigned)s.w0 / (unsigned)a.Wo);
      count(acc, fetch<KIND>(s, f, sy, sx));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {                              // (all 64 lanes are here: the loop bounds above are wave-uniform)
      acc.c0 += (uint32_t)__shfl_xor((int)acc.c0, d, 64);
      acc.c1 += (uint32_t)__shfl_xor((int)acc.c1, d, 64);
      acc.c2 += (uint32_t)__shfl_xor((int)acc.c2, d, 64);
      acc.m += (uint32_t)__shfl_xor((int)acc.m, d, 64);
    }
    if (lane < 3) {
      const uint32_t sum = lane == 0 ? acc.c0 : (lane == 1 ? acc.c1 : acc.c2);
      chip_out[(long)p * 3 + lane] = (unsigned char)(acc.m != 0u ? (sum + (acc.m >> 1)) / acc.m : (fill >> 8 * lane) & 0xFFu);
    }
  }
}

// The checks both entries share, made before any pointer is looked at.  -> the status; Fc: the frames taken.
inline int crops_call(int h0, int w0, int F, int Ho, int Wo, int n, int f_first, int f_step, int Sh, int Sw, int pad256, int min_area,
                      int cutout, int fill, long out_row_stride, int c_off, long rect_row_stride, int& Fc, unsigned& tiles) {
  MDQE_REQUIRE(Sh >= 1 && Sh <= 512 && Sw >= 1 && Sw <= 512 && pad256 >= 0 && pad256 <= 256 && min_area >= 0);
  MDQE_REQUIRE((cutout == 0 || cutout == 1) && fill >= 0 && fill <= 0xFFFFFF && n >= 0 && n <= 255);
  MDQE_REQUIRE(F >= 0 && Ho > 0 && Wo > 0 && h0 > 0 && w0 > 0 && f_first >= 0 && f_step >= 1 && c_off >= 0);
  MDQE_REQUIRE((long)Ho * Wo < (1L << 24));                          // a uint32 sum of bytes cannot overflow
  MDQE_REQUIRE((long)h0 * Ho < 0x7FFFFFFFL && (long)w0 * Wo < 0x7FFFFFFFL);          // (Y * h0, X * w0 in 32 bits)
  const long taken = f_first < F ? ((long)F - f_first + f_step - 1) / f_step : 0;
  const long chips = (long)c_off + taken, chip_bytes = 3L * Sh * Sw;
  MDQE_REQUIRE(chips * chip_bytes < 0x7FFFFFFFL);
  if (n > 1) MDQE_REQUIRE(out_row_stride >= chips * chip_bytes && rect_row_stride >= chips * 4);   // (two writers otherwise)
  tiles = (unsigned)((Sh * Sw + 255) / 256);
  MDQE_REQUIRE((long)n * taken * tiles < 0x7FFFFFFFL);               // the block index of one call is 32-bit
  Fc = (int)taken;
  return MDQE_OK;
}

inline void set_args(CropArgs& a, const unsigned char* labels, int F, int Ho, int Wo, const int* geom, int n, int Fc, int f_first, int f_step,
                     int Sh, int Sw, int pad256, int min_area, int cutout, int fill, unsigned char* out, long out_row_stride, int c_off,
                     int* rects, long rect_row_stride, unsigned tiles) {
  a.labels = labels; a.geom = geom; a.out = out; a.rects = rects;
  a.out_row_stride = out_row_stride; a.rect_row_stride = rect_row_stride;
  a.F = F; a.Ho = Ho; a.Wo = Wo; a.n = n; a.Fc = Fc; a.f_first = f_first; a.f_step = f_step; a.Sh = Sh; a.Sw = Sw;
  a.pad256 = pad256; a.min_area = min_area; a.cutout = cutout; a.c_off = c_off; a.fill = (uint32_t)fill; a.tiles = tiles;
}

}  // namespace

extern "C" int mdqe_track_crops_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                                   const unsigned char* labels, int F, int Ho, int Wo, const int* geom, int n,
                                   int f_first, int f_step, int Sh, int Sw, int pad256, int min_area, int cutout, int fill,
                                   unsigned char* out, long out_row_stride, int c_off, int* rects, long rect_row_stride, void* stream) {
  int Fc = 0;
  unsigned tiles = 0;
  const int st = crops_call(h0, w0, F, Ho, Wo, n, f_first, f_step, Sh, Sw, pad256, min_area, cutout, fill, out_row_stride, c_off,
                            rect_row_stride, Fc, tiles);
  if (st != MDQE_OK) return st;
  MDQE_REQUIRE(is_u8 == 0 || is_u8 == 1);
  MDQE_REQUIRE(frame_stride >= 3L * h0 * w0 || F <= 1);
  if (n == 0 || Fc == 0) return MDQE_OK;
  MDQE_CHECK_PTR(frames);
  MDQE_CHECK_PTR(labels);
  MDQE_CHECK_PTR(geom);
  MDQE_CHECK_PTR(out);
  MDQE_CHECK_PTR(rects);
  CropArgs a;
  set_args(a, labels, F, Ho, Wo, geom, n, Fc, f_first, f_step, Sh, Sw, pad256, min_area, cutout, fill, out, out_row_stride, c_off, rects,
           rect_row_stride, tiles);
  RgbSource s;
  s.frames = frames; s.frame_stride = frame_stride; s.h0 = h0; s.w0 = w0; s.plane = (long)h0 * w0;
  const dim3 grid((unsigned)n * (unsigned)Fc * tiles);
  mdqe_clear_error();
  if (is_u8) hipLaunchKernelGGL(track_crops_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, a, s);
  else hipLaunchKernelGGL(track_crops_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a, s);
  return mdqe_launch_status();
}

extern "C" int mdqe_track_crops_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                         int H, int W, int fmt, int matrix, int full_range, int bgr,
                                         const unsigned char* labels, int F, int Ho, int Wo, const int* geom, int n,
                                         int f_first, int f_step, int Sh, int Sw, int pad256, int min_area, int cutout, int fill,
                                         unsigned char* out, long out_row_stride, int c_off, int* rects, long rect_row_stride, void* stream) {
  static const int coeffs[8][7] = MDQE_YUV_COEFFS;
  int Fc = 0;
  unsigned tiles = 0;
  const int st = crops_call(H, W, F, Ho, Wo, n, f_first, f_step, Sh, Sw, pad256, min_area, cutout, fill, out_row_stride, c_off,
                            rect_row_stride, Fc, tiles);
  if (st != MDQE_OK) return st;
  // the surface conditions of mdqe_yuv420sp_to_rgb_u8
  MDQE_REQUIRE((fmt == 0 || fmt == 1) && (matrix == 0 || matrix == 1));
  const long bps = fmt ? 2 : 1;
  MDQE_REQUIRE(y_pitch >= bps * W && uv_pitch >= bps * 2 * ((W + 1L) / 2) && y_stride >= 0 && uv_stride >= 0);
  if (fmt == 1) MDQE_REQUIRE(((y_pitch | y_stride | uv_pitch | uv_stride) & 1L) == 0);
  if (n == 0 || Fc == 0) return MDQE_OK;
  MDQE_CHECK_PTR(y);
  MDQE_CHECK_PTR(uv);
  MDQE_CHECK_PTR(labels);
  MDQE_CHECK_PTR(geom);
  MDQE_CHECK_PTR(out);
  MDQE_CHECK_PTR(rects);
  if (fmt == 1) MDQE_REQUIRE((((uintptr_t)y | (uintptr_t)uv) & 1u) == 0);
  CropArgs a;
  set_args(a, labels, F, Ho, Wo, geom, n, Fc, f_first, f_step, Sh, Sw, pad256, min_area, cutout, fill, out, out_row_stride, c_off, rects,
           rect_row_stride, tiles);
  const int* c = coeffs[4 * fmt + 2 * matrix + (full_range ? 1 : 0)];
  YuvSource s;
  s.y = (const unsigned char*)y; s.uv = (const unsigned char*)uv;
  s.y_pitch = y_pitch; s.y_stride = y_stride; s.uv_pitch = uv_pitch; s.uv_stride = uv_stride;
  s.h0 = H; s.w0 = W; s.bgr = bgr ? 1 : 0;
  s.yo = c[0]; s.co = c[1]; s.cy = c[2]; s.rv = c[3]; s.gu = c[4]; s.gv = c[5]; s.bu = c[6];
  const dim3 grid((unsigned)n * (unsigned)Fc * tiles);
  mdqe_clear_error();
  if (fmt == 0) hipLaunchKernelGGL(track_crops_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, a, s);
  else hipLaunchKernelGGL(track_crops_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a, s);
  return mdqe_launch_status();
}
