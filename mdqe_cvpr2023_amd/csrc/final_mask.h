// One output pixel of the final mask (mdqe/mdqe.py:357-358 + 458-462; the formula is stated above the entry points in final_mask.hip),
// shared by every form built on it -- dense, RLE, geometry, label map (final_mask.hip), the overlap counts (score_ops.hip) and the
// occlusion table (occlusion.hip): identical arithmetic, identical bits.  Three steps: where the pixel reads (the same for every map
// of a window), the up-sampled logit there, and the threshold on it.
#pragma once
#include "common.h"

struct MaskTaps { int y0, y1, x0, x1; float ly, lx; };

__device__ __forceinline__ MaskTaps final_mask_taps(int Hm, int Wm, int factor, int h, int w, float sy_scale, float sx_scale, int Y, int X) {
  const int sy = min((int)floorf(Y * sy_scale), h - 1), sx = min((int)floorf(X * sx_scale), w - 1);
  const float fy = (float)max(sy - factor / 2, 0) / (float)factor, fx = (float)max(sx - factor / 2, 0) / (float)factor;
  const int y0 = min((int)fy, Hm - 1), x0 = min((int)fx, Wm - 1);
  const int y1 = min(y0 + 1, Hm - 1), x1 = min(x0 + 1, Wm - 1);
  return MaskTaps{y0, y1, x0, x1, fy - y0, fx - x0};
}

// (m: row 0 of the rows t.y0 / t.y1 count from, Wm floats apart)
__device__ __forceinline__ float final_mask_value_at(const float* __restrict__ m, int Wm, const MaskTaps& t) {
  const float top = m[t.y0 * Wm + t.x0] * (1.f - t.lx) + m[t.y0 * Wm + t.x1] * t.lx;
  const float bot = m[t.y1 * Wm + t.x0] * (1.f - t.lx) + m[t.y1 * Wm + t.x1] * t.lx;
  return top * (1.f - t.ly) + bot * t.ly;
}

__device__ __forceinline__ float final_mask_value(const float* __restrict__ m, int Hm, int Wm, int factor, int h, int w, float sy_scale,
                                                  float sx_scale, int Y, int X) {
  return final_mask_value_at(m, Wm, final_mask_taps(Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, X));
}

__device__ __forceinline__ int final_mask_bit(float v) {
  const float p = 1.0f / (1.0f + expf(-v));
  return p > 0.5f ? 1 : 0;
}

__device__ __forceinline__ int final_mask_pixel(const float* __restrict__ m, int Hm, int Wm, int factor, int h, int w, float sy_scale,
                                                float sx_scale, int Y, int X) {
  return final_mask_bit(final_mask_value(m, Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, X));
}

// The owner of a pixel, one row at a time in the order of the selected rows: row k (bit: its final-mask bit, v: its up-sampled logit)
// takes the pixel from `best` (-1: nobody yet; best_v: its logit) iff its bit is set and it is the first such row or v is strictly
// larger.  So the owner is the first row with the largest logit among the set ones: the label map's choice and the occlusion table's.
__device__ __forceinline__ bool final_owner_takes(int bit, float v, int best, float best_v) {
  return bit && (best < 0 || v > best_v);
}

// The matte's level 0..255 from x = gain * (the largest up-sampled logit of the participating rows) and U = the OR of their final-mask
// bits: the rounded sigmoid, held at >= 128 where a bit is set and at <= 127 where none is.  So level >= 128 exactly where U is set,
// whatever gain is and whatever the last ulp of expf is.  Every form that needs a level calls this.
__device__ __forceinline__ int final_matte_level(float x, int U) {
  const float p = 1.f / (1.f + expf(-x));
  const int a = (int)rintf(255.f * p);
  return U ? max(a, 128) : min(a, 127);
}

// ---- host only: what the six entry points of the family share (final_mask.hip, score_ops.hip) ------------------------------------------
#define MDQE_TRY(e) do { const int rc_ = (e); if (rc_ != MDQE_OK) return rc_; } while (0)

// The arguments every entry point leads with; each keeps the conditions that are its own, its MDQE_OK for nothing to do, its pointers.
static inline int final_mask_args(int n_sel, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo) {
  MDQE_REQUIRE(n_sel >= 0 && Fw >= 0 && Hm > 0 && Wm > 0 && factor >= 1 && h > 0 && w > 0 && Ho > 0 && Wo > 0);
  MDQE_REQUIRE(h <= Hm * factor && w <= Wm * factor);
  return MDQE_OK;
}

// Output rows a block takes when `units` masks or frames share about `blocks` blocks of 256 threads (4096: ~16 per CU; 2048: ~8), at
// least ~1024 pixels (4 per thread) a block so that reduction and atomics stay a small part of its work.  n_bands = ceil(Ho / band).
static inline int final_mask_band(long blocks, long units, int Ho, int Wo) {
  long want = (blocks + units - 1) / units;
  const long most = ((long)Ho * Wo + 1023) / 1024;
  if (want > most) want = most;
  if (want > Ho) want = Ho;
  if (want < 1) want = 1;
  return (int)((Ho + want - 1) / want);
}
