// The compositing painter: the overlay's picture mixed with a backdrop -- one colour or a picture of the output's size -- by a soft
// matte (mdqe_final_matte_u8), so that tracks or the background are REPLACED with an anti-aliased edge.  ONE definition, integers only
// (include/mdqe_hip.h has the rule); tests/_matte_ref.py restates it in numpy and every comparison is exact.
//
// A pure streaming pass shaped like render.hip: 1 label byte + 1 matte byte + 3 frame bytes (+ 3 backdrop bytes) in, 3 bytes out per
// pixel; 256-thread blocks, at most 2048 of them, grid-stride over GROUPS of 4 consecutive pixels of the flat [F, Ho, Wo] index, laid out
// from the OUTPUT address (`head` single pixels bring the first group to a 4-byte boundary, every group's 12 bytes are three aligned
// dwords, `tail` single pixels; head and tail go through the per-pixel path with byte stores).  A group inside one row reads its labels,
// its matte, its uint8 source planes (equal sizes) and its backdrop pixels 4 (12) bytes at a time; one that straddles rows or frames
// paints its pixels one by one and still stores three dwords.  Contour neighbours are looked at for tinted pixels only, straight from
// the label map (L1).  The palette rows and the action table sit in LDS.  No atomics: the output is a function of the inputs.
// The rule's pieces (source pixel, tint, contour test and dispatch) and the entry's checks are render_rule.h's.
#include "render_rule.h"

namespace {

struct ReplaceArgs {
  RgbSource src;
  const unsigned char* labels;   // [F, Ho, Wo]
  const unsigned char* matte;    // [F, Ho, Wo]
  const unsigned char* palette;  // [256, 3]
  const unsigned char* action;   // [256]
  const unsigned char* backdrop; // [3], or [Ho, Wo, 3] (picture)
  unsigned char* out;            // at frame f_off already: [F, Ho, Wo, 3]
  unsigned n_px, HoWo;           // F * Ho * Wo (< 2^31), Ho * Wo
  int Ho, Wo;
  unsigned head, n_groups, tail;
  uint32_t a256;
  int ident;
  int picture;                   // the backdrop is a picture
  int mode;                      // 0: the matte is what is kept, 1: the matte is what is replaced
};

// mix of the rule on a packed pixel: (s * w + b * (255 - w) + 127) / 255 per channel (at most 255 * 255 + 127 < 2^16)
__device__ __forceinline__ uint32_t mix1(uint32_t s, uint32_t b, uint32_t w) { return (s * w + b * (255u - w) + 127u) / 255u; }
__device__ __forceinline__ uint32_t mix3(uint32_t s, uint32_t b, uint32_t w) {
  return mix1(s & 0xFFu, b & 0xFFu, w) | mix1((s >> 8) & 0xFFu, (b >> 8) & 0xFFu, w) << 8 | mix1((s >> 16) & 0xFFu, (b >> 16) & 0xFFu, w) << 16;
}

// One pixel from its label l (at q), source s, matte level m and backdrop pixel b: base = the overlay rule's pixel (action 1 tints, every
// other action keeps the source), then the mix.
template <int R>
__device__ __forceinline__ uint32_t replace_px(const ReplaceArgs& a, const uint32_t* pal, const unsigned char* act, const unsigned char* q,
                                               uint32_t l, int Y, int X, uint32_t s, uint32_t m, uint32_t b) {
  const uint32_t base = act[l] == 1u ? tint(s, pal[l], edge_at<R>(q, l, Y, X, a.Ho, a.Wo), a.a256) : s;
  return mix3(base, b, a.mode ? 255u - m : m);
}

// One pixel of the flat index, every bound checked: the rule as written.
template <int KIND, int R>
__device__ __forceinline__ uint32_t paint_pixel(const ReplaceArgs& a, const uint32_t* pal, const unsigned char* act, uint32_t colour, unsigned p) {
  const unsigned f = p / a.HoWo, rem = p - f * a.HoWo;
  const int Y = (int)(rem / (unsigned)a.Wo), X = (int)(rem - (unsigned)Y * (unsigned)a.Wo);
  const uint32_t s = source_px<KIND>(a.src, a.ident, (long)f * a.src.frame_stride, Y, X, a.Ho, a.Wo);
  const uint32_t b = a.picture ? pack_rgb(a.backdrop + 3L * rem) : colour;
  return replace_px<R>(a, pal, act, a.labels + p, a.labels[p], Y, X, s, a.matte[p], b);
}

template <int KIND, int R>
__global__ __launch_bounds__(256) void render_replace_kernel(const ReplaceArgs a) {
  __shared__ uint32_t pal[256];
  __shared__ unsigned char act[256];
  pal[threadIdx.x] = pack_rgb(a.palette + 3 * threadIdx.x);
  act[threadIdx.x] = a.action[threadIdx.x];
  __syncthreads();
  const uint32_t colour = a.picture ? 0u : pack_rgb(a.backdrop);
  if (blockIdx.x == 0 && threadIdx.x < a.head + a.tail) {            // the 0..3 + 0..3 pixels outside the groups
    const unsigned p = threadIdx.x < a.head ? threadIdx.x : a.n_px - a.tail + (threadIdx.x - a.head);
    const uint32_t v = paint_pixel<KIND, R>(a, pal, act, colour, p);
    unsigned char* o = a.out + 3L * p;
    o[0] = (unsigned char)v; o[1] = (unsigned char)(v >> 8); o[2] = (unsigned char)(v >> 16);
  }
  const unsigned step = gridDim.x * 256u;
  for (unsigned g = blockIdx.x * 256u + threadIdx.x; g < a.n_groups; g += step) {
    const unsigned p = a.head + 4u * g;
    const unsigned f = p / a.HoWo, rem = p - f * a.HoWo;
    const int Y = (int)(rem / (unsigned)a.Wo), X = (int)(rem - (unsigned)Y * (unsigned)a.Wo);
    uint32_t px[4];
    if (X + 3 < a.Wo) {
      // the wide path: the four pixels lie inside row Y
      const unsigned char* lab = a.labels + p;
      const uint32_t l4 = ld4(lab), m4 = ld4(a.matte + p);
      uint32_t s[4] = {0u, 0u, 0u, 0u}, b[4] = {colour, colour, colour, colour};
      if (KIND != 0) {
        if (KIND == 1 && a.ident) {
          const unsigned char* q = (const unsigned char*)a.src.frames + (long)f * a.src.frame_stride + (long)Y * a.src.w0 + X;
          const uint32_t c0 = ld4(q), c1 = ld4(q + a.src.plane), c2 = ld4(q + 2 * a.src.plane);
#pragma unroll
          for (int i = 0; i < 4; ++i)
            s[i] = ((c0 >> 8 * i) & 0xFFu) | ((c1 >> 8 * i) & 0xFFu) << 8 | ((c2 >> 8 * i) & 0xFFu) << 16;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) s[i] = source_px<KIND>(a.src, a.ident, (long)f * a.src.frame_stride, Y, X + i, a.Ho, a.Wo);
        }
      }
      if (a.picture) {
        const unsigned char* q = a.backdrop + 3L * rem;               // 12 bytes inside the picture's row Y
        const uint32_t w0 = ld4(q), w1 = ld4(q + 4), w2 = ld4(q + 8);
        b[0] = w0 & 0xFFFFFFu;
        b[1] = w0 >> 24 | (w1 & 0xFFFFu) << 8;
        b[2] = w1 >> 16 | (w2 & 0xFFu) << 16;
        b[3] = w2 >> 8;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
        px[i] = replace_px<R>(a, pal, act, lab + i, (l4 >> 8 * i) & 0xFFu, Y, X + i, s[i], (m4 >> 8 * i) & 0xFFu, b[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) px[i] = paint_pixel<KIND, R>(a, pal, act, colour, p + i);
    }
    uint32_t* o = (uint32_t*)(a.out + 3L * p);                       // 4-byte aligned by the choice of `head`
    o[0] = px[0] | px[1] << 24;
    o[1] = px[1] >> 8 | px[2] << 16;
    o[2] = px[2] >> 16 | px[3] << 8;
  }
}

// ---- surfaces -----------------------------------------------------------------------------------------------------------------------
// The same compositing on decoder surfaces (NV12, P010).  A thread owns one 2 x 2 block -- the two luma rows that share a chroma row, so
// every chroma pair has ONE writer, which holds the four labels and the four weights that decide it -- and reads only the samples it
// writes: painting in place is allowed as in render_yuv.hip.  Single samples at any alignment (the 4- and 16-byte forms of render_yuv.hip
// are not built here).  The backdrop is one colour in sample units or one surface of the same size and format.
struct ReplaceYuvArgs {
  const unsigned char* y;
  const unsigned char* uv;
  const unsigned char* labels;                   // [F, H, W]
  const unsigned char* matte;                    // [F, H, W]
  const unsigned short* palette;                 // [256, 3]: Y, U, V in sample units
  const unsigned char* action;                   // [256]
  const unsigned short* colour;                  // [3], or NULL: the backdrop surface below
  const unsigned char* by;
  const unsigned char* buv;
  unsigned char* oy;                             // at frame f_off already
  unsigned char* ouv;
  long y_pitch, y_stride, uv_pitch, uv_stride;   // bytes
  long oy_pitch, oy_stride, ouv_pitch, ouv_stride;
  long by_pitch, buv_pitch;
  int H, W;
  unsigned XU, RP, n_units;                      // blocks per row pair, row pairs per surface, F * RP * XU
  uint32_t a256;
  int mode;
};

template <int FMT, int R>
__global__ __launch_bounds__(256) void render_replace_yuv_kernel(const ReplaceYuvArgs a) {
  __shared__ uint32_t pal[256];
  __shared__ unsigned char act[256];
  pal[threadIdx.x] = pack_yuv(a.palette + 3 * threadIdx.x);
  act[threadIdx.x] = a.action[threadIdx.x];
  __syncthreads();
  const unsigned u = blockIdx.x * 256u + threadIdx.x;
  if (u >= a.n_units) return;
  const unsigned rpn = u / a.XU, xu = u - rpn * a.XU;
  const unsigned n = rpn / a.RP, rp = rpn - n * a.RP;
  const int r0 = 2 * (int)rp, c = 2 * (int)xu;
  const unsigned char* yrow = a.y + n * a.y_stride + (long)r0 * a.y_pitch;
  const unsigned char* crow = a.uv + n * a.uv_stride + (long)rp * a.uv_pitch;
  unsigned char* oyrow = a.oy + n * a.oy_stride + (long)r0 * a.oy_pitch;
  unsigned char* ocrow = a.ouv + n * a.ouv_stride + (long)rp * a.ouv_pitch;
  const long at = ((long)n * a.H + r0) * a.W + c;                    // label and matte of (r0, c)
  const uint32_t ru = row_raw<FMT>(crow, c), rv = row_raw<FMT>(crow, c + 1);
  const uint32_t U = value_of<FMT>(ru), V = value_of<FMT>(rv);
  uint32_t BY = 0u, BU, BV;
  if (a.colour != nullptr) {
    BY = a.colour[0] & (FMT ? 0x3FFu : 0xFFu); BU = a.colour[1] & (FMT ? 0x3FFu : 0xFFu); BV = a.colour[2] & (FMT ? 0x3FFu : 0xFFu);
  } else {
    const unsigned char* bc = a.buv + (long)rp * a.buv_pitch;
    BU = value_of<FMT>(row_raw<FMT>(bc, c)); BV = value_of<FMT>(row_raw<FMT>(bc, c + 1));
  }
  uint32_t su = 0u, sv = 0u, np = 0u;
  bool same = true;                                                  // every pixel of the block kept at full weight
  for (int row = 0; row < 2 && r0 + row < a.H; ++row) {
    for (int k = 0; k < 2 && c + k < a.W; ++k) {
      const int Y = r0 + row, X = c + k;
      const unsigned char* q = a.labels + at + (long)row * a.W + k;
      const uint32_t l = q[0], m = a.matte[at + (long)row * a.W + k];
      const uint32_t wt = a.mode ? 255u - m : m;
      const bool tinted = act[l] == 1u;
      const bool edge = tinted && edge_at<R>(q, l, Y, X, a.H, a.W);
      const uint32_t col = pal[l];
      const uint32_t ry = row_raw<FMT>(yrow + (long)row * a.y_pitch, X);
      const uint32_t sy = value_of<FMT>(ry);
      if (a.colour == nullptr) BY = value_of<FMT>(row_raw<FMT>(a.by + (long)Y * a.by_pitch, X));
      const uint32_t base = tinted ? tint1(sy, comp<FMT>(col, 0), edge, a.a256) : sy;
      const bool kept = !tinted && wt == 255u;
      row_put<FMT>(oyrow + (long)row * a.oy_pitch, X, kept ? ry : stored<FMT>(mix1(base, BY, wt)));
      su += mix1(tinted ? tint1(U, comp<FMT>(col, 1), edge, a.a256) : U, BU, wt);
      sv += mix1(tinted ? tint1(V, comp<FMT>(col, 2), edge, a.a256) : V, BV, wt);
      same = same && kept;
      ++np;
    }
  }
  const uint32_t sh = np >> 1;                                       // n = 1, 2, 4: n / 2 = log2(n) = 0, 1, 2
  row_put<FMT>(ocrow, c, same ? ru : stored<FMT>((su + sh) >> sh));
  row_put<FMT>(ocrow, c + 1, same ? rv : stored<FMT>((sv + sh) >> sh));
}

template <int FMT>
void launch_replace_yuv(int contour, dim3 grid, hipStream_t stream, const ReplaceYuvArgs& a) {
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_replace_yuv_kernel<FMT, decltype(R)::value>), grid, dim3(256), 0, stream, a);
  });
}

template <int KIND>
void launch_replace(int contour, dim3 grid, hipStream_t stream, const ReplaceArgs& a) {
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_replace_kernel<KIND, decltype(R)::value>), grid, dim3(256), 0, stream, a);
  });
}

}  // namespace

extern "C" int mdqe_render_replace_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                                      const unsigned char* labels, int F, int Ho, int Wo,
                                      const unsigned char* palette, const unsigned char* action, int a256, int contour,
                                      const unsigned char* matte, const unsigned char* backdrop, int backdrop_picture, int mode,
                                      unsigned char* out, int f_off, void* stream) {
  MDQE_REQUIRE((mode == 0 || mode == 1) && (backdrop_picture == 0 || backdrop_picture == 1));
  ReplaceArgs a;
  const int st = rgb_call(frames, frame_stride, h0, w0, labels, F, Ho, Wo, palette, action, true, a256, contour, out, f_off, a.src, a.ident, a.out);
  if (st != MDQE_OK || F == 0) return st;
  MDQE_CHECK_PTR(matte);
  MDQE_CHECK_PTR(backdrop);
  a.labels = labels;
  a.matte = matte;
  a.palette = palette;
  a.action = action;
  a.backdrop = backdrop;
  a.HoWo = (unsigned)Ho * (unsigned)Wo;
  a.n_px = (unsigned)F * a.HoWo;
  a.Ho = Ho;
  a.Wo = Wo;
  a.head = (unsigned)((uintptr_t)a.out & 3u);
  if (a.head > a.n_px) a.head = a.n_px;
  a.n_groups = (a.n_px - a.head) / 4u;
  a.tail = a.n_px - a.head - 4u * a.n_groups;
  a.a256 = (uint32_t)a256;
  a.picture = backdrop_picture;
  a.mode = mode;
  unsigned blocks = (a.n_groups + 255u) / 256u;
  if (blocks > 2048u) blocks = 2048u;
  if (blocks < 1u) blocks = 1u;
  mdqe_clear_error();
  const dim3 grid(blocks);
  if (frames == nullptr) launch_replace<0>(contour, grid, (hipStream_t)stream, a);
  else if (is_u8) launch_replace<1>(contour, grid, (hipStream_t)stream, a);
  else launch_replace<2>(contour, grid, (hipStream_t)stream, a);
  return mdqe_launch_status();
}

extern "C" int mdqe_render_replace_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                            int F, int H, int W, int fmt, const unsigned char* labels,
                                            const unsigned short* palette_yuv, const unsigned char* action, int a256, int contour,
                                            const unsigned char* matte, const unsigned short* backdrop_yuv,
                                            const void* by, long by_pitch, const void* buv, long buv_pitch, int mode,
                                            void* out_y, long out_y_pitch, long out_y_stride,
                                            void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream) {
  MDQE_REQUIRE(mode == 0 || mode == 1);
  SurfaceOut o;                                                      // in place is accepted: a thread reads only the samples it writes
  const int st = surface_call(y, y_pitch, y_stride, uv, uv_pitch, uv_stride, F, H, W, fmt, labels, palette_yuv, action, true, true, a256,
                              contour, out_y, out_y_pitch, out_y_stride, out_uv, out_uv_pitch, out_uv_stride, f_off, o);
  if (st != MDQE_OK || F == 0) return st;
  MDQE_CHECK_PTR(matte);
  const long bps = fmt ? 2 : 1, yb = bps * W, cb = bps * 2 * ((W + 1L) / 2), CH = (H + 1L) / 2;
  const Plane ty = plane_of(o.oy, out_y_pitch, out_y_stride, F, H, yb), tc = plane_of(o.ouv, out_uv_pitch, out_uv_stride, F, CH, cb);
  const Plane sm = plane_of(matte, W, (long)H * W, F, H, W);
  MDQE_REQUIRE(apart(sm, ty) && apart(sm, tc));
  if (backdrop_yuv != nullptr) {
    MDQE_REQUIRE(((uintptr_t)backdrop_yuv & 1u) == 0);
    const Plane sb = plane_of(backdrop_yuv, 6, 0, 1, 1, 6);
    MDQE_REQUIRE(apart(sb, ty) && apart(sb, tc));
  } else {
    MDQE_CHECK_PTR(by);
    MDQE_CHECK_PTR(buv);
    MDQE_REQUIRE(by_pitch >= yb && buv_pitch >= cb);
    if (fmt == 1) MDQE_REQUIRE((((uintptr_t)by | (uintptr_t)buv | (uintptr_t)by_pitch | (uintptr_t)buv_pitch) & 1u) == 0);
    const Plane s1 = plane_of(by, by_pitch, 0, 1, H, yb), s2 = plane_of(buv, buv_pitch, 0, 1, CH, cb);
    MDQE_REQUIRE(apart(s1, ty) && apart(s1, tc) && apart(s2, ty) && apart(s2, tc));
  }
  ReplaceYuvArgs a;
  a.y = (const unsigned char*)y;
  a.uv = (const unsigned char*)uv;
  a.labels = labels;
  a.matte = matte;
  a.palette = palette_yuv;
  a.action = action;
  a.colour = backdrop_yuv;
  a.by = (const unsigned char*)by;
  a.buv = (const unsigned char*)buv;
  a.oy = o.oy;
  a.ouv = o.ouv;
  a.y_pitch = y_pitch; a.y_stride = y_stride; a.uv_pitch = uv_pitch; a.uv_stride = uv_stride;
  a.oy_pitch = out_y_pitch; a.oy_stride = out_y_stride; a.ouv_pitch = out_uv_pitch; a.ouv_stride = out_uv_stride;
  a.by_pitch = by_pitch; a.buv_pitch = buv_pitch;
  a.H = H; a.W = W;
  a.XU = (unsigned)((W + 1) / 2);
  a.RP = (unsigned)((H + 1) / 2);
  a.n_units = (unsigned)F * a.RP * a.XU;                             // <= F * H * W < 2^31
  a.a256 = (uint32_t)a256;
  a.mode = mode;
  mdqe_clear_error();
  const dim3 grid((a.n_units + 255u) / 256u);
  if (fmt == 0) launch_replace_yuv<0>(contour, grid, (hipStream_t)stream, a);
  else launch_replace_yuv<1>(contour, grid, (hipStream_t)stream, a);
  return mdqe_launch_status();
}
