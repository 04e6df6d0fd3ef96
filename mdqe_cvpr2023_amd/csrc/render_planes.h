// The overlap test of the surface painters (render_yuv.hip, render_mosaic.hip): which planes of a call may meet.
#pragma once
#include <stdint.h>

namespace {

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

}  // namespace
