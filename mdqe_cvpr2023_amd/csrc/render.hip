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
// The rule's pieces (source pixel, tint, contour test and dispatch) and the entry's checks are render_rule.h's, shared with the other painters.
#include "render_rule.h"

namespace {

struct RenderArgs {
  RgbSource src;
  const unsigned char* labels;   // [F, Ho, Wo]
  const unsigned char* palette;  // [256, 3]
  unsigned char* out;            // at frame f_off already: [F, Ho, Wo, 3]
  unsigned n_px, HoWo;           // F * Ho * Wo (< 2^31), Ho * Wo
  int Ho, Wo;
  unsigned head, n_groups, tail;
  int a256;
  int ident;                     // (Ho, Wo) == (h0, w0): the source pixel is the output pixel
};

// One pixel of the flat index, every bound checked: the rule as written.
template <int KIND, int R>
__device__ __forceinline__ uint32_t paint_pixel(const RenderArgs& a, const uint32_t* pal, unsigned p) {
  const unsigned f = p / a.HoWo, rem = p - f * a.HoWo;
  const int Y = (int)(rem / (unsigned)a.Wo), X = (int)(rem - (unsigned)Y * (unsigned)a.Wo);
  const unsigned char* lab = a.labels + p;
  const uint32_t l = lab[0];
  const bool edge = edge_at<R>(lab, l, Y, X, a.Ho, a.Wo);
  const uint32_t s = source_px<KIND>(a.src, a.ident, (long)f * a.src.frame_stride, Y, X, a.Ho, a.Wo);
  const uint32_t t = tint(s, pal[l], edge, (uint32_t)a.a256);
  return l != 0u ? t : s;                                            // background keeps the source
}

template <int KIND, int R>
__global__ __launch_bounds__(256) void render_overlay_kernel(const RenderArgs a) {
  __shared__ uint32_t pal[256];
  pal[threadIdx.x] = pack_rgb(a.palette + 3 * threadIdx.x);
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
          const long at = (long)f * a.src.frame_stride + (long)Y * a.src.w0 + X;
          if (KIND == 1) {
            const unsigned char* q = (const unsigned char*)a.src.frames + at;
            const uint32_t c0 = ld4(q), c1 = ld4(q + a.src.plane), c2 = ld4(q + 2 * a.src.plane);
#pragma unroll
            for (int i = 0; i < 4; ++i)
              s[i] = ((c0 >> 8 * i) & 0xFFu) | ((c1 >> 8 * i) & 0xFFu) << 8 | ((c2 >> 8 * i) & 0xFFu) << 16;
          } else {
            const float* q = (const float*)a.src.frames + at;
#pragma unroll
            for (int i = 0; i < 4; ++i)
              s[i] = to_u8(q[i]) | to_u8(q[a.src.plane + i]) << 8 | to_u8(q[2 * a.src.plane + i]) << 16;
          }
        } else {
          const long row = (long)f * a.src.frame_stride + (long)((unsigned)Y * (unsigned)a.src.h0 / (unsigned)a.Ho) * a.src.w0;
#pragma unroll
          for (int i = 0; i < 4; ++i)
            s[i] = src_px<KIND>(a.src, row + (long)((unsigned)(X + i) * (unsigned)a.src.w0 / (unsigned)a.Wo));
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t l = (c4 >> 8 * i) & 0xFFu;
        const uint32_t t = tint(s[i], pal[l], ((diff >> 8 * i) & 0xFFu) != 0u, (uint32_t)a.a256);
        px[i] = l != 0u ? t : s[i];
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
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_overlay_kernel<KIND, decltype(R)::value>), grid, dim3(256), 0, stream, a);
  });
}

}  // namespace

extern "C" int mdqe_render_overlay_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                                      const unsigned char* labels, int F, int Ho, int Wo,
                                      const unsigned char* palette, int a256, int contour,
                                      unsigned char* out, int f_off, void* stream) {
  RenderArgs a;
  const int st = rgb_call(frames, frame_stride, h0, w0, labels, F, Ho, Wo, palette, nullptr, false, a256, contour, out, f_off, a.src, a.ident, a.out);
  if (st != MDQE_OK || F == 0) return st;
  a.labels = labels;
  a.palette = palette;
  a.HoWo = (unsigned)Ho * (unsigned)Wo;
  a.n_px = (unsigned)F * a.HoWo;
  a.Ho = Ho;
  a.Wo = Wo;
  a.head = (unsigned)((uintptr_t)a.out & 3u);
  if (a.head > a.n_px) a.head = a.n_px;
  a.n_groups = (a.n_px - a.head) / 4u;
  a.tail = a.n_px - a.head - 4u * a.n_groups;
  a.a256 = a256;
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
