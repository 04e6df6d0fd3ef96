// Rendered overlay frames: the picture a viewer would paint from a window's label map (mdqe_final_label_map_u8) and the frames the
// caller handed in, painted on the device.  ONE definition, integers only (include/mdqe_hip.h has the rule); tests/_overlay_ref.py
// restates it in numpy and every comparison is exact.
//
// A pure streaming pass: at equal sizes 1 label byte + 3 frame bytes in, 3 bytes out per pixel.  256-thread blocks, at most 2048 of
// them, grid-stride over GROUPS of 4 consecutive pixels of the flat [F, Ho, Wo] index: a group is one 4-byte label read, one 4-byte read
// per frame plane (equal sizes) and one 12-byte write.  Nothing is aligned by the caller -- Wo, Ho*Wo*3 and f_off*Ho*Wo*3 are arbitrary --
// so the groups are laid out from the OUTPUT address: `head` = 0..3 single pixels bring the first group to a 4-byte boundary (3 * head ==
// -address mod 4 has the solution head = address mod 4), then every group's 12 bytes are three aligned dwords, then `tail` = 0..3 single
// pixels.  Head and tail go through the per-pixel path with byte stores.  A group whose pixels and contour neighbours all lie inside one
// row takes the wide path (its neighbour reads are the same 4-byte window shifted by d pixels or d rows); a group at a row's ends, or one
// that straddles two rows or frames, paints its four pixels one by one and still stores three dwords.  The contour neighbours are read
// straight from the label map: they are the bytes the neighbouring lanes and the rows above and below read anyway, so they hit L1 (what
// profiles/label_map_ab.txt found for the map rows of the label kernel); there is no LDS tile.  The 256 palette rows sit in LDS, one
// packed dword each.  No atomics, no control flow that depends on data beyond selects on the label: the output is a function of the inputs.
#include "common.h"

namespace {

struct RenderArgs {
  const void* frames;            // [F, 3, h0, w0] planes, frame stride `frame_stride` elements; unused for KIND 0
  long frame_stride;
  long plane;                    // h0 * w0
  int h0, w0;
  const unsigned char* labels;   // [F, Ho, Wo]
  const unsigned char* palette;  // [256, 3]
  unsigned char* out;            // at frame f_off already: [F, Ho, Wo, 3]
  unsigned n_px, HoWo;           // F * Ho * Wo (< 2^31), Ho * Wo
  int Ho, Wo;
  unsigned head, n_groups, tail;
  int a256;
  int ident;                     // (Ho, Wo) == (h0, w0): the source pixel is the output pixel
};

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

// The source pixel at element offset `at` (frame, row and column applied) as c0 | c1 << 8 | c2 << 16.  KIND 0: no frames (black), 1: uint8, 2: float32.
template <int KIND>
__device__ __forceinline__ uint32_t src_px(const RenderArgs& a, long at) {
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

// out_c = (s_c * (256 - a) + pal_c * a + 128) >> 8 on a packed pixel: channels 0 and 2 share one multiply (each 16-bit lane holds at most
// 255 * 256 + 128 < 2^16: no carry between them).  Background keeps the source, a contour pixel takes the palette row.
__device__ __forceinline__ uint32_t paint(uint32_t s, uint32_t pal, uint32_t l, bool edge, uint32_t a) {
  const uint32_t rb = ((s & 0x00FF00FFu) * (256u - a) + (pal & 0x00FF00FFu) * a + 0x00800080u) >> 8 & 0x00FF00FFu;
  const uint32_t g = (((s >> 8) & 0xFFu) * (256u - a) + ((pal >> 8) & 0xFFu) * a + 128u) & 0xFF00u;
  const uint32_t o = edge ? pal : (rb | g);
  return l != 0u ? o : s;
}

// One pixel of the flat index, every bound checked: the rule as written.
template <int KIND, int R>
__device__ __forceinline__ uint32_t paint_pixel(const RenderArgs& a, const uint32_t* pal, unsigned p) {
  const unsigned f = p / a.HoWo, rem = p - f * a.HoWo;
  const int Y = (int)(rem / (unsigned)a.Wo), X = (int)(rem - (unsigned)Y * (unsigned)a.Wo);
  const unsigned char* lab = a.labels + p;
  const uint32_t l = lab[0];
  bool edge = false;
#pragma unroll
  for (int d = 1; d <= R; ++d) {
    if (X - d >= 0) edge |= lab[-d] != l;
    if (X + d < a.Wo) edge |= lab[d] != l;
    if (Y - d >= 0) edge |= lab[-(long)d * a.Wo] != l;
    if (Y + d < a.Ho) edge |= lab[(long)d * a.Wo] != l;
  }
  uint32_t s = 0u;
  if (KIND != 0) {
    const int sy = a.ident ? Y : (int)((unsigned)Y * (unsigned)a.h0 / (unsigned)a.Ho);
    const int sx = a.ident ? X : (int)((unsigned)X * (unsigned)a.w0 / (unsigned)a.Wo);
    s = src_px<KIND>(a, (long)f * a.frame_stride + (long)sy * a.w0 + sx);
  }
  return paint(s, pal[l], l, edge, (uint32_t)a.a256);
}

template <int KIND, int R>
__global__ __launch_bounds__(256) void render_overlay_kernel(const RenderArgs a) {
  __shared__ uint32_t pal[256];
  {
    const unsigned char* q = a.palette + 3 * threadIdx.x;
    pal[threadIdx.x] = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16;
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < a.head + a.tail) {            // the 0..3 + 0..3 pixels outside the groups
    const unsigned p = threadIdx.x < a.head ? threadIdx.x : a.n_px - a.tail + (threadIdx.x - a.head);
    const uint32_t v = paint_pixel<KIND, R>(a, pal, p);
    unsigned char* o = a.out + 3L * p;
    o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16);
  }
  const unsigned step = gridDim.x * 256u;
  for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < a.n_groups; g += step) {
    const unsigned p = a.head + 4u * g;
    const unsigned f = p / a.HoWo, rem = p - f * a.HoWo;
    const int Y = (int)(rem / (unsigned)a.Wo), X = (int)(rem - (unsigned)Y * (unsigned)a.Wo);
    uint32_t px[4];
    if (X >= R && X + 3 + R < a.Wo) {
      // the wide path: the four pixels and all their neighbours at distance <= R lie inside row Y
      const unsigned char* lab = a.labels + p;
      const uint32_t c4 = ld4(lab);
      uint32_t diff = 0u;                                            // byte i != 0: pixel i has a neighbour with another label
#pragma unroll
      for (int d = 1; d <= R; ++d) {
        diff |= c4 ^ ld4(lab - d);
        diff |= c4 ^ ld4(lab + d);
        if (Y - d >= 0) diff |= c4 ^ ld4(lab - (long)d * a.Wo);
        if (Y + d < a.Ho) diff |= c4 ^ ld4(lab + (long)d * a.Wo);
      }
      uint32_t s[4] = {0u, 0u, 0u, 0u};
      if (KIND != 0) {
        if (a.ident) {
          const long at = (long)f * a.frame_stride + (long)Y * a.w0 + X;
          if (KIND == 1) {
            const unsigned char* q = (const unsigned char*)a.frames + at;
            const uint32_t c0 = ld4(q), c1 = ld4(q + a.plane), c2 = ld4(q + 2 * a.plane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
              s[i] = ((c0 >> 8 * i) & 0xFFu) | ((c1 >> 8 * i) & 0xFFu) << 8 | ((c2 >> 8 * i) & 0xFFu) << 16;
          } else {
            const float* q = (const float*)a.frames + at;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              s[i] = to_u8(q[i]) | to_u8(q[a.plane + i]) << 8 | to_u8(q[2 * a.plane + i]) << 16;
          }
        } else {
          const long row = (long)f * a.frame_stride + (long)((unsigned)Y * (unsigned)a.h0 / (unsigned)a.Ho) * a.w0;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            s[i] = src_px<KIND>(a, row + (long)((unsigned)(X + i) * (unsigned)a.w0 / (unsigned)a.Wo));
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t l = (c4 >> 8 * i) & 0xFFu;
        px[i] = paint(s[i], pal[l], l, ((diff >> 8 * i) & 0xFFu) != 0u, (uint32_t)a.a256);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) px[i] = paint_pixel<KIND, R>(a, pal, p + i);
    }
    uint32_t* o = (uint32_t*)(a.out + 3L * p);                       // 4-byte aligned by the choice of `head`
    o[0] = px[0] | px[1] << 24;
    o[1] = px[1] >> 8 | px[2] << 16;
    o[2] = px[2] >> 16 | px[3] << 8;
  }
}

template <int KIND>
void launch_render(int contour, dim3 grid, hipStream_t stream, const RenderArgs& a) {
  switch (contour) {
    case 0: hipLaunchKernelGGL((render_overlay_kernel<KIND, 0>), grid, dim3(256), 0, stream, a); break;
    case 1: hipLaunchKernelGGL((render_overlay_kernel<KIND, 1>), grid, dim3(256), 0, stream, a); break;
    case 2: hipLaunchKernelGGL((render_overlay_kernel<KIND, 2>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((render_overlay_kernel<KIND, 3>), grid, dim3(256), 0, stream, a); break;
  }
}

}  // namespace

extern "C" int mdqe_render_overlay_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                                      const unsigned char* labels, int F, int Ho, int Wo,
                                      const unsigned char* palette, int a256, int contour,
                                      unsigned char* out, int f_off, void* stream) {
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
  MDQE_CHECK_PTR(out);
  RenderArgs a;
  a.frames = frames;
  a.frame_stride = frame_stride;
  a.h0 = frames ? h0 : 1;
  a.w0 = frames ? w0 : 1;
  a.plane = (long)a.h0 * a.w0;
  a.labels = labels;
  a.palette = palette;
  a.HoWo = (unsigned)Ho * (unsigned)Wo;
  a.out = out + (long)f_off * a.HoWo * 3;
  a.n_px = (unsigned)F * a.HoWo;
  a.Ho = Ho;
  a.Wo = Wo;
  a.head = (unsigned)((uintptr_t)a.out & 3u);
  if (a.head > a.n_px) a.head = a.n_px;
  a.n_groups = (a.n_px - a.head) / 4u;
  a.tail = a.n_px - a.head - 4u * a.n_groups;
  a.a256 = a256;
  a.ident = frames != nullptr && h0 == Ho && w0 == Wo;
  unsigned blocks = (a.n_groups + 255u) / 256u;
  if (blocks > 2048u) blocks = 2048u;
  if (blocks < 1u) blocks = 1u;
  mdqe_clear_error();
  const dim3 grid(blocks);
  if (frames == nullptr) launch_render<0>(contour, grid, (hipStream_t)stream, a);
  else if (is_u8) launch_render<1>(contour, grid, (hipStream_t)stream, a);
  else launch_render<2>(contour, grid, (hipStream_t)stream, a);
  return mdqe_launch_status();
}
