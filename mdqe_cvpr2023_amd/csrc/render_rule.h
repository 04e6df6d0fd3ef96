// The overlay painters' rule, said once: what render.hip, render_yuv.hip and render_mosaic.hip share.  Device side: the source pixel, the
// tint (packed RGB and one component), the stored-sample helpers of the two surface formats, the palette's LDS packings, the contour
// test and the contour dispatch.  Host side: the argument checks of the two RGB entries and of the two surface entries, the surface
// entries' overlap test included.  The kernels, their launch decisions and their argument structs stay in the three .hip files.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

// ---- device: RGB --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld4(const unsigned char* p) {     // (any alignment)
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// float32 frame value -> 0..255: round half to even, clamp, NaN -> 0 (both comparisons are false for a NaN)
__device__ __forceinline__ uint32_t to_u8(float v) {
  const float r = __builtin_rintf(v);
  return r >= 0.f ? (r > 255.f ? 255u : (uint32_t)r) : 0u;
}

struct RgbSource {
  const void* frames;            // [F, 3, h0, w0] planes, frame stride `frame_stride` elements; unused for KIND 0
  long frame_stride;
  long plane;                    // h0 * w0
  int h0, w0;
};

// The source pixel at element offset `at` (frame, row and column applied) as c0 | c1 << 8 | c2 << 16.  KIND 0: no frames (black), 1: uint8, 2: float32.
template <int KIND>
__device__ __forceinline__ uint32_t src_px(const RgbSource& a, long at) {
  if (KIND == 1) {
    const unsigned char* s = (const unsigned char*)a.frames + at;
    return (uint32_t)s[0] | (uint32_t)s[a.plane] << 8 | (uint32_t)s[2 * a.plane] << 16;
  }
  if (KIND == 2) {
    const float* s = (const float*)a.frames + at;
    return to_u8(s[0]) | to_u8(s[a.plane]) << 8 | to_u8(s[2 * a.plane]) << 16;
  }
  return 0u;
}

// The source pixel of output pixel (Y, X) of an Ho x Wo picture, in the frame at element offset `frame`: the pixel itself (ident) or its
// nearest neighbour.
template <int KIND>
__device__ __forceinline__ uint32_t source_px(const RgbSource& a, int ident, long frame, int Y, int X, int Ho, int Wo) {
  if (KIND == 0) return 0u;
  const int sy = ident ? Y : (int)((unsigned)Y * (unsigned)a.h0 / (unsigned)Ho);
  const int sx = ident ? X : (int)((unsigned)X * (unsigned)a.w0 / (unsigned)Wo);
  return src_px<KIND>(a, frame + (long)sy * a.w0 + sx);
}

// out_c = (s_c * (256 - a) + pal_c * a + 128) >> 8 on a packed pixel: channels 0 and 2 share one multiply (each 16-bit lane holds at most
// 255 * 256 + 128 < 2^16: no carry between them).  A contour pixel takes the palette row.
__device__ __forceinline__ uint32_t tint(uint32_t s, uint32_t pal, bool edge, uint32_t a) {
  const uint32_t rb = ((s & 0x00FF00FFu) * (256u - a) + (pal & 0x00FF00FFu) * a + 0x00800080u) >> 8 & 0x00FF00FFu;
  const uint32_t g = (((s >> 8) & 0xFFu) * (256u - a) + ((pal >> 8) & 0xFFu) * a + 128u) & 0xFF00u;
  return edge ? pal : (rb | g);
}

__device__ __forceinline__ uint32_t pack_rgb(const unsigned char* q) {   // a palette row as one LDS dword
  return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
}

// ---- device: surfaces (FMT 0: NV12 bytes, 1: P010 little-endian words, value = word >> 6) ---------------------------------------------
// stored sample i of a plane row in memory, and its store
template <int FMT>
__device__ __forceinline__ uint32_t row_raw(const unsigned char* row, int i) {
  return FMT == 0 ? (uint32_t)row[i] : (uint32_t)((const unsigned short*)row)[i];
}

template <int FMT>
__device__ __forceinline__ void row_put(unsigned char* row, int i, uint32_t raw) {
  if (FMT == 0) row[i] = (unsigned char)raw; else ((unsigned short*)row)[i] = (unsigned short)raw;
}

// the value of a stored sample, and the stored form of a value the rule produced
template <int FMT> __device__ __forceinline__ uint32_t value_of(uint32_t raw) { return FMT == 0 ? raw : raw >> 6; }
template <int FMT> __device__ __forceinline__ uint32_t stored(uint32_t v) { return FMT == 0 ? v : v << 6; }

// a palette row (Y, U, V) as one LDS dword of 10-bit fields, and its component k
__device__ __forceinline__ uint32_t pack_yuv(const unsigned short* q) {
  return ((uint32_t)q[0] & 0x3FFu) | ((uint32_t)q[1] & 0x3FFu) << 10 | ((uint32_t)q[2] & 0x3FFu) << 20;
}
template <int FMT> __device__ __forceinline__ uint32_t comp(uint32_t c, int k) { return (c >> 10 * k) & (FMT ? 0x3FFu : 0xFFu); }

// the blend of the rule on one component.  s, p <= 1023: s * (256 - a) + p * a + 128 < 2^19.
__device__ __forceinline__ uint32_t blend1(uint32_t s, uint32_t p, uint32_t a) { return (s * (256u - a) + p * a + 128u) >> 8; }

// tinted value of the rule: the palette component on an edge, else the blend
__device__ __forceinline__ uint32_t tint1(uint32_t s, uint32_t p, bool edge, uint32_t a) { return edge ? p : blend1(s, p, a); }

// ---- the contour ----------------------------------------------------------------------------------------------------------------------
// edge of the rule: pixel (Y, X) with label l at q has, within R pixels along an axis and inside the picture, a neighbour of another label
template <int R>
__device__ __forceinline__ bool edge_at(const unsigned char* q, uint32_t l, int Y, int X, int H, int W) {
  bool edge = false;
#pragma unroll
  for (int d = 1; d <= R; ++d) {
    if (X - d >= 0) edge |= q[-d] != l;
    if (X + d < W) edge |= q[d] != l;
    if (Y - d >= 0) edge |= q[-(long)d * W] != l;
    if (Y + d < H) edge |= q[(long)d * W] != l;
  }
  return edge;
}

// fn(std::integral_constant<int, contour>): a launch picks its kernel's R with decltype(R)::value.  contour is 0..3 (the entries check).
template <class Fn>
void with_contour(int contour, Fn&& fn) {
  switch (contour) {
    case 0: fn(std::integral_constant<int, 0>()); break;
    case 1: fn(std::integral_constant<int, 1>()); break;
    case 2: fn(std::integral_constant<int, 2>()); break;
    default: fn(std::integral_constant<int, 3>()); break;
  }
}

// ---- host: the RGB entries' checks ----------------------------------------------------------------------------------------------------
// Sizes first, F == 0 next (MDQE_OK: the entry launches nothing), null pointers last; `action` is looked at only `with_action`.
// -> the status, the source, whether it is the output's size, and `out` at frame f_off.
inline int rgb_call(const void* frames, long frame_stride, int h0, int w0, const unsigned char* labels, int F, int Ho, int Wo,
                    const unsigned char* palette, const unsigned char* action, bool with_action, int a256, int contour,
                    unsigned char* out, int f_off, RgbSource& src, int& ident, unsigned char*& out_at) {
  MDQE_REQUIRE(a256 >= 0 && a256 <= 256 && contour >= 0 && contour <= 3);
  MDQE_REQUIRE(F >= 0 && Ho > 0 && Wo > 0 && f_off >= 0 && (long)Ho * Wo * 3 < 0x7FFFFFFFL);
  MDQE_REQUIRE((long)F * Ho * Wo < 0x7FFFFFFFL);                     // the flat pixel index of one call is 32-bit
  if (frames != nullptr) {
    MDQE_REQUIRE(h0 > 0 && w0 > 0 && (long)h0 * Ho < 0x7FFFFFFFL && (long)w0 * Wo < 0x7FFFFFFFL);   // (Y * h0, X * w0 in 32 bits)
    MDQE_REQUIRE(frame_stride >= 3L * h0 * w0 || F <= 1);
  }
  if (F == 0) return MDQE_OK;
  MDQE_CHECK_PTR(labels);
  MDQE_CHECK_PTR(palette);
  if (with_action) MDQE_CHECK_PTR(action);
  MDQE_CHECK_PTR(out);
  src.frames = frames;
  src.frame_stride = frame_stride;
  src.h0 = frames ? h0 : 1;
  src.w0 = frames ? w0 : 1;
  src.plane = (long)src.h0 * src.w0;
  ident = frames != nullptr && h0 == Ho && w0 == Wo;
  out_at = out + (long)f_off * Ho * Wo * 3;
  return MDQE_OK;
}

// ---- host: the surface entries' checks ------------------------------------------------------------------------------------------------
// A plane of the call: n surfaces of `extent` bytes (first byte to last byte of a surface, the rows' padding included), `stride` bytes
// apart.  Planes of one decoder allocation interleave (luma 0, chroma 0, luma 1, ...), so what must not meet are SURFACES, not spans.
struct Plane { long lo, stride, extent; int n; };
inline Plane plane_of(const void* p, long pitch, long stride, int n, long rows, long row_bytes) {
  return {(long)(uintptr_t)p, n > 1 ? stride : 0, (rows - 1) * pitch + row_bytes, n};
}
inline bool apart(const Plane& s, const Plane& t) {
  const long s_hi = s.lo + (s.n - 1) * s.stride + s.extent, t_hi = t.lo + (t.n - 1) * t.stride + t.extent;
  if (s_hi <= t.lo || t_hi <= s.lo) return true;                     // the spans do not meet
  if (s.n == t.n && s.stride == t.stride && s.stride > 0 && s.extent <= s.stride && t.extent <= s.stride) {
    // one stride: surface j of t starts d + k * stride behind some surface of s, 0 <= d < stride; they meet iff d < s.extent (k = 0) or
    // d + t.extent > stride (k = -1).  (Which k occur is not looked at: that only refuses more.)
    const long m = (t.lo - s.lo) % s.stride, d = m < 0 ? m + s.stride : m;
    return d >= s.extent && d + t.extent <= s.stride;
  }
  for (int i = 0; i < s.n; ++i)                                      // anything else: surface by surface
    for (int j = 0; j < t.n; ++j) {
      const long a = s.lo + i * s.stride, b = t.lo + j * t.stride;
      if (a < b + t.extent && b < a + s.extent) return false;
    }
  return true;
}

struct SurfaceOut {
  unsigned char* oy;             // the output planes at frame f_off
  unsigned char* ouv;
  uintptr_t m;                   // every address, pitch and (F > 1) stride of the launch, and W, or-ed: the alignment they share
};

// Sizes first, F == 0 next (MDQE_OK: the entry launches nothing), null pointers, then alignment and overlap.  No output plane may meet
// an input plane, the other output plane, the labels, the palette or (`with_action`) the action table; `allow_in_place` excepts an
// output plane that IS its input plane (same address, pitch and stride): nothing else is a function of the inputs.
inline int surface_call(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride, int F, int H, int W, int fmt,
                        const unsigned char* labels, const unsigned short* palette_yuv, const unsigned char* action, bool with_action,
                        bool allow_in_place, int a256, int contour, void* out_y, long out_y_pitch, long out_y_stride,
                        void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, SurfaceOut& s) {
  MDQE_REQUIRE(a256 >= 0 && a256 <= 256 && contour >= 0 && contour <= 3);
  MDQE_REQUIRE(F >= 0 && H > 0 && W > 0 && f_off >= 0 && (fmt == 0 || fmt == 1));
  const long bps = fmt ? 2 : 1, yb = bps * W, cb = bps * 2 * ((W + 1L) / 2), CH = (H + 1L) / 2;
  MDQE_REQUIRE(y_pitch >= yb && uv_pitch >= cb && y_stride >= 0 && uv_stride >= 0);
  MDQE_REQUIRE(out_y_pitch >= yb && out_uv_pitch >= cb && out_y_stride >= 0 && out_uv_stride >= 0);
  if (fmt == 1)
    MDQE_REQUIRE(((y_pitch | y_stride | uv_pitch | uv_stride | out_y_pitch | out_y_stride | out_uv_pitch | out_uv_stride) & 1L) == 0);
  // (two output surfaces that shared bytes would have two writers)
  if (F > 1) MDQE_REQUIRE(out_y_stride >= (H - 1) * out_y_pitch + yb && out_uv_stride >= (CH - 1) * out_uv_pitch + cb);
  MDQE_REQUIRE((long)F * H * W < 0x7FFFFFFFL);                       // the block index of one call is 32-bit
  if (F == 0) return MDQE_OK;
  MDQE_CHECK_PTR(y);
  MDQE_CHECK_PTR(uv);
  MDQE_CHECK_PTR(labels);
  MDQE_CHECK_PTR(palette_yuv);
  if (with_action) MDQE_CHECK_PTR(action);
  MDQE_CHECK_PTR(out_y);
  MDQE_CHECK_PTR(out_uv);
  MDQE_REQUIRE(((uintptr_t)palette_yuv & 1u) == 0);
  if (fmt == 1) MDQE_REQUIRE((((uintptr_t)y | (uintptr_t)uv | (uintptr_t)out_y | (uintptr_t)out_uv) & 1u) == 0);
  s.oy = (unsigned char*)out_y + (long)f_off * out_y_stride;
  s.ouv = (unsigned char*)out_uv + (long)f_off * out_uv_stride;
  const Plane sy = plane_of(y, y_pitch, y_stride, F, H, yb), sc = plane_of(uv, uv_pitch, uv_stride, F, CH, cb);
  const Plane ty = plane_of(s.oy, out_y_pitch, out_y_stride, F, H, yb), tc = plane_of(s.ouv, out_uv_pitch, out_uv_stride, F, CH, cb);
  const Plane sl = plane_of(labels, W, (long)H * W, F, H, W), sp = plane_of(palette_yuv, 6, 0, 1, 256, 6);
  const bool same_y = allow_in_place && s.oy == (const unsigned char*)y && out_y_pitch == y_pitch && (F == 1 || out_y_stride == y_stride);
  const bool same_c = allow_in_place && s.ouv == (const unsigned char*)uv && out_uv_pitch == uv_pitch && (F == 1 || out_uv_stride == uv_stride);
  MDQE_REQUIRE(same_y || apart(sy, ty));
  MDQE_REQUIRE(same_c || apart(sc, tc));
  MDQE_REQUIRE(apart(sy, tc) && apart(sc, ty) && apart(ty, tc));
  MDQE_REQUIRE(apart(sl, ty) && apart(sl, tc) && apart(sp, ty) && apart(sp, tc));
  if (with_action) {
    const Plane sa = plane_of(action, 256, 0, 1, 1, 256);
    MDQE_REQUIRE(apart(sa, ty) && apart(sa, tc));
  }
  // (strides matter only between surfaces)
  s.m = (uintptr_t)y | (uintptr_t)uv | (uintptr_t)s.oy | (uintptr_t)s.ouv | (uintptr_t)labels | (uintptr_t)W
      | (uintptr_t)y_pitch | (uintptr_t)uv_pitch | (uintptr_t)out_y_pitch | (uintptr_t)out_uv_pitch;
  if (F > 1) s.m |= (uintptr_t)y_stride | (uintptr_t)uv_stride | (uintptr_t)out_y_stride | (uintptr_t)out_uv_stride | (uintptr_t)((long)H * W);
  return MDQE_OK;
}

}  // namespace
