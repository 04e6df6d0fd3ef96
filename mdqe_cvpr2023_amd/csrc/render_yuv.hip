// Overlays painted straight onto decoder surfaces: semi-planar YUV 4:2:0 (NV12, P010) in, painted surfaces of the same format out, for
// an encoder.  ONE definition, integers only (include/mdqe_hip.h has the rule); tests/_overlay_yuv_ref.py restates it in numpy and every
// comparison is exact.  A background pixel keeps the decoder's bits (P010: all 16 of a word).
//
// A pure streaming pass: 1 label byte + 1.5 surface bytes in and 1.5 out per pixel for NV12 (P010: 1 + 3 in, 3 out).  A thread owns a
// block of 2 rows by PX pixels -- the two rows that share a chroma row, as in yuv.hip: every chroma pair has ONE writer, which holds the
// four labels that decide it -- and the whole batch is one launch of one thread per block.  PX is a per-launch decision of the entry:
//   PX = 16  every plane pointer (in, out, labels), pitch, stride and W are multiples of 16 bytes AND contour == 0: 16-byte accesses;
//   PX = 4   the same with multiples of 4, any contour: 4-byte accesses;
//   PX = 2   anything else: single samples, one 2 x 2 block per thread.
// Why a contour launch stays at PX = 4 (profiles/overlay_surface_ab.txt): with the neighbour rows in registers a PX = 16 thread is a
// long chain over 32 pixels and a window is only some 3 waves per SIMD of them; measured on 30 NV12 surfaces, contour 1, the 4-byte
// form takes 21.5 us against 38.0 (360 x 640) and 102 against 151 (1080 x 1920), contour 3 half the time at both sizes.  Without a
// contour the 16-byte form is the faster one at 1080p (46.9 us against 63.0) and no slower at 360p.
// In a wide launch a block whose contour neighbours lie inside its row (c0 >= R and c0 + PX + R <= W) and whose second row exists takes
// the wide path: the label rows r0 - R .. r0 + 1 + R of its columns are 2 + 2R aligned chunk reads (the rows outside the picture are not
// read and never count), the horizontal neighbours are the chunk shifted by d bytes against the dwords to its left and right, all read
// straight from the map -- they are the bytes the neighbouring lanes and row pairs read anyway, so they hit L1 (what render.hip found);
// there is no LDS tile.  Everything else -- the blocks at a row's ends, the odd last row, every block of a PX = 2 launch -- goes through the
// per-sample path, the rule as written with every bound checked.  The 256 palette rows sit in LDS, one packed dword each.  No atomics;
// a thread reads the surface samples it owns and nothing else of the surfaces, then writes the same samples of the output: the output
// is a function of the inputs, also when the output planes ARE the input planes (the only overlap the entry accepts).
//
// No clamp is needed anywhere: a blend lies between its two operands and a rounded mean between its smallest and largest term.  The
// shifts are plain shifts of non-negative 32-bit values, each followed by a mask or a select, never a shift-then-clamp pair (see the
// note above clamp8 in yuv.hip); the exact comparisons of tests/test_overlay_yuv_gpu.py are the guard.
// The rule's pieces (sample helpers, tint, contour test and dispatch) and the entry's checks, the overlap test among them, are
// render_rule.h's, shared with the other painters; the chunk helpers of the wide path are this file's own.
#include "render_rule.h"

namespace {

struct RenderYuvArgs {
  const unsigned char* y;
  const unsigned char* uv;
  const unsigned char* labels;                   // [F, H, W]
  const unsigned short* palette;                 // [256, 3]: Y, U, V in sample units
  unsigned char* oy;                             // at frame f_off already
  unsigned char* ouv;
  long y_pitch, y_stride, uv_pitch, uv_stride;   // bytes
  long oy_pitch, oy_stride, ouv_pitch, ouv_stride;
  int H, W;
  unsigned XU, RP, n_units;                      // blocks per row pair, row pairs per surface, F * RP * XU
  uint32_t a256;
};

template <int BYTES, int ALIGN>
__device__ __forceinline__ void ld_chunk(uint32_t* dst, const unsigned char* p) {
  __builtin_memcpy(dst, __builtin_assume_aligned(p, ALIGN), BYTES);
}

template <int BYTES, int ALIGN>
__device__ __forceinline__ void st_chunk(unsigned char* p, const uint32_t* src) {
  __builtin_memcpy(__builtin_assume_aligned(p, ALIGN), src, BYTES);
}

// stored sample i of a row chunk held in dwords, as it lies in memory: a byte (NV12) or a little-endian 16-bit word (P010)
template <int FMT>
__device__ __forceinline__ uint32_t chunk_raw(const uint32_t* w, int i) {
  return FMT == 0 ? (w[i >> 2] >> (8 * (i & 3))) & 0xFFu : (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
}

template <int FMT>
__device__ __forceinline__ void chunk_put(uint32_t* w, int i, uint32_t raw) {
  if (FMT == 0) {
    if ((i & 3) == 0) w[i >> 2] = raw; else w[i >> 2] |= raw << (8 * (i & 3));
  } else {
    if ((i & 1) == 0) w[i >> 1] = raw; else w[i >> 1] |= raw << 16;
  }
}

// px(s, p) of the rule: background keeps the sample, a contour pixel takes the palette component, the rest blends.  (tint1 with the
// blend taken first and both selects after it: written this way the compiler emits the kernels profiles/overlay_surface_ab.txt measured.)
__device__ __forceinline__ uint32_t px(uint32_t s, uint32_t p, uint32_t l, bool edge, uint32_t a) {
  const uint32_t b = blend1(s, p, a);
  const uint32_t o = edge ? p : b;
  return l != 0u ? o : s;
}

// One 2 x 2 block (columns c, c + 1 of rows r0, r0 + 1; c even, c < W, r0 < H) with every bound checked: the rule as written.  `lab` is
// the label of (r0, c), yrow / oyrow row r0 of the luma planes, crow / ocrow the chroma row of the pair.
template <int FMT, int R>
__device__ __forceinline__ void paint_block(const RenderYuvArgs& a, const uint32_t* pal, const unsigned char* lab, int r0, int c,
                                            const unsigned char* yrow, const unsigned char* crow, unsigned char* oyrow, unsigned char* ocrow) {
  const uint32_t ru = row_raw<FMT>(crow, c), rv = row_raw<FMT>(crow, c + 1);
  const uint32_t U = value_of<FMT>(ru), V = value_of<FMT>(rv);
  uint32_t su = 0u, sv = 0u, any = 0u, n = 0u;
  for (int row = 0; row < 2 && r0 + row < a.H; ++row) {
    for (int k = 0; k < 2 && c + k < a.W; ++k) {
      const int Y = r0 + row, X = c + k;
      const unsigned char* q = lab + (long)row * a.W + k;
      const uint32_t l = q[0];
      const bool edge = edge_at<R>(q, l, Y, X, a.H, a.W);
      const uint32_t col = pal[l];
      const uint32_t ry = row_raw<FMT>(yrow + (long)row * a.y_pitch, X);
      const uint32_t yo = px(value_of<FMT>(ry), comp<FMT>(col, 0), l, edge, a.a256);
      row_put<FMT>(oyrow + (long)row * a.oy_pitch, X, l != 0u ? stored<FMT>(yo) : ry);
      su += px(U, comp<FMT>(col, 1), l, edge, a.a256);
      sv += px(V, comp<FMT>(col, 2), l, edge, a.a256);
      any |= l;
      ++n;
    }
  }
  // n is 1, 2 or 4: (sum + n / 2) >> log2(n)
  const uint32_t sh = n >> 1;                                        // 0, 1, 2
  const uint32_t uo = (su + sh) >> sh, vo = (sv + sh) >> sh;
  row_put<FMT>(ocrow, c, any != 0u ? stored<FMT>(uo) : ru);
  row_put<FMT>(ocrow, c + 1, any != 0u ? stored<FMT>(vo) : rv);
}

template <int FMT, int PX, int R>
__global__ __launch_bounds__(256) void render_overlay_yuv_kernel(const RenderYuvArgs a) {
  __shared__ uint32_t pal[256];
  pal[threadIdx.x] = pack_yuv(a.palette + 3 * threadIdx.x);
  __syncthreads();
  const unsigned u = blockIdx.x * 256u + threadIdx.x;
  if (u >= a.n_units) return;
  const unsigned rpn = u / a.XU, xu = u - rpn * a.XU;              // row pair over the batch, block of the row pair
  const unsigned n = rpn / a.RP, rp = rpn - n * a.RP;
  const int r0 = 2 * (int)rp, c0 = PX * (int)xu;
  constexpr int BPS = FMT ? 2 : 1;                                   // bytes per sample
  const unsigned char* yrow = a.y + n * a.y_stride + (long)r0 * a.y_pitch;
  const unsigned char* crow = a.uv + n * a.uv_stride + (long)rp * a.uv_pitch;
  unsigned char* oyrow = a.oy + n * a.oy_stride + (long)r0 * a.oy_pitch;
  unsigned char* ocrow = a.ouv + n * a.ouv_stride + (long)rp * a.ouv_pitch;
  const unsigned char* lab = a.labels + ((long)n * a.H + r0) * a.W + c0;
  if constexpr (PX > 2) if (r0 + 1 < a.H && c0 >= R && c0 + PX + R <= a.W) {
    // the wide path: rows r0 and r0 + 1, pixels c0 .. c0 + PX - 1, every horizontal neighbour inside the row
    constexpr int NL = PX / 4, NW = PX * BPS / 4;
    uint32_t lr[2 * R + 2][NL];                                      // label rows r0 - R .. r0 + 1 + R (those inside the picture)
#pragma unroll
    for (int k = 0; k < 2 * R + 2; ++k) {
      const int rr = r0 - R + k;
      if (rr >= 0 && rr < a.H) {
        ld_chunk<PX, PX>(lr[k], lab + (long)(k - R) * a.W);
      } else {
#pragma unroll
        for (int j = 0; j < NL; ++j) lr[k][j] = 0u;
      }
    }
    uint32_t diff[2][NL];                                            // byte i != 0: pixel i has a neighbour with another label
#pragma unroll
    for (int row = 0; row < 2; ++row) {
      const uint32_t* c4 = lr[R + row];
#pragma unroll
      for (int j = 0; j < NL; ++j) diff[row][j] = 0u;
      if (R > 0) {
        uint32_t e[NL + 2];                                          // the dword to the left, the chunk, the dword to the right
        ld_chunk<4, 4>(&e[0], lab + (long)row * a.W - 4);            // (c0 >= R > 0 and c0 a multiple of PX: c0 >= 4)
        ld_chunk<4, 4>(&e[NL + 1], lab + (long)row * a.W + PX);      // (c0 + PX + R <= W, W a multiple of PX: c0 + PX + 4 <= W)
#pragma unroll
        for (int j = 0; j < NL; ++j) e[j + 1] = c4[j];
#pragma unroll
        for (int d = 1; d <= R; ++d) {
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const uint64_t lo = (uint64_t)e[j + 1] << 32 | e[j], hi = (uint64_t)e[j + 2] << 32 | e[j + 1];
            diff[row][j] |= c4[j] ^ (uint32_t)(lo >> (32 - 8 * d));  // the bytes d pixels to the left
            diff[row][j] |= c4[j] ^ (uint32_t)(hi >> (8 * d));       // d pixels to the right
          }
          const int up = r0 + row - d, dn = r0 + row + d;
          if (up >= 0) {
#pragma unroll
            for (int j = 0; j < NL; ++j) diff[row][j] |= c4[j] ^ lr[R + row - d][j];
          }
          if (dn < a.H) {
#pragma unroll
            for (int j = 0; j < NL; ++j) diff[row][j] |= c4[j] ^ lr[R + row + d][j];
          }
        }
      }
    }
    uint32_t yw[2][NW], cw[NW], oyw[2][NW], ocw[NW];
    ld_chunk<4 * NW, PX>(yw[0], yrow + (long)c0 * BPS);
    ld_chunk<4 * NW, PX>(yw[1], yrow + a.y_pitch + (long)c0 * BPS);
    ld_chunk<4 * NW, PX>(cw, crow + (long)c0 * BPS);               // c0 is even: pair c0 / 2 starts at sample c0
#pragma unroll
    for (int p = 0; p < PX / 2; ++p) {
      const uint32_t ru = chunk_raw<FMT>(cw, 2 * p), rv = chunk_raw<FMT>(cw, 2 * p + 1);
      const uint32_t U = value_of<FMT>(ru), V = value_of<FMT>(rv);
      uint32_t su = 0u, sv = 0u, any = 0u;
#pragma unroll
      for (int row = 0; row < 2; ++row) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int i = 2 * p + k;
          const uint32_t l = (lr[R + row][i >> 2] >> (8 * (i & 3))) & 0xFFu;
          const bool edge = ((diff[row][i >> 2] >> (8 * (i & 3))) & 0xFFu) != 0u;
          const uint32_t col = pal[l];
          const uint32_t ry = chunk_raw<FMT>(yw[row], i);
          const uint32_t yo = px(value_of<FMT>(ry), comp<FMT>(col, 0), l, edge, a.a256);
          chunk_put<FMT>(oyw[row], i, l != 0u ? stored<FMT>(yo) : ry);
          su += px(U, comp<FMT>(col, 1), l, edge, a.a256);
          sv += px(V, comp<FMT>(col, 2), l, edge, a.a256);
          any |= l;
        }
      }
      const uint32_t uo = (su + 2u) >> 2, vo = (sv + 2u) >> 2;
      chunk_put<FMT>(ocw, 2 * p, any != 0u ? stored<FMT>(uo) : ru);
      chunk_put<FMT>(ocw, 2 * p + 1, any != 0u ? stored<FMT>(vo) : rv);
    }
    st_chunk<4 * NW, PX>(oyrow + (long)c0 * BPS, oyw[0]);
    st_chunk<4 * NW, PX>(oyrow + a.oy_pitch + (long)c0 * BPS, oyw[1]);
    st_chunk<4 * NW, PX>(ocrow + (long)c0 * BPS, ocw);
    return;
  }
  // the per-sample path
  for (int p = 0; p < PX / 2; ++p) {
    const int c = c0 + 2 * p;
    if (c >= a.W) break;
    paint_block<FMT, R>(a, pal, lab + 2 * p, r0, c, yrow, crow, oyrow, ocrow);
  }
}

template <int FMT, int PX>
void launch_r(int contour, dim3 grid, hipStream_t stream, const RenderYuvArgs& a) {
  with_contour(contour, [&](auto R) {
    hipLaunchKernelGGL((render_overlay_yuv_kernel<FMT, PX, decltype(R)::value>), grid, dim3(256), 0, stream, a);
  });
}

template <int FMT>
void launch_render_yuv(int px, int contour, dim3 grid, hipStream_t stream, const RenderYuvArgs& a) {
  switch (px) {
    case 16: hipLaunchKernelGGL((render_overlay_yuv_kernel<FMT, 16, 0>), grid, dim3(256), 0, stream, a); break;   // (contour == 0 only)
    case 4: launch_r<FMT, 4>(contour, grid, stream, a); break;
    default: launch_r<FMT, 2>(contour, grid, stream, a); break;
  }
}

}  // namespace

extern "C" int mdqe_render_overlay_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                            int F, int H, int W, int fmt, const unsigned char* labels,
                                            const unsigned short* palette_yuv, int a256, int contour,
                                            void* out_y, long out_y_pitch, long out_y_stride,
                                            void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream) {
  SurfaceOut o;                                                      // in place is accepted: a thread reads only the samples it writes
  const int st = surface_call(y, y_pitch, y_stride, uv, uv_pitch, uv_stride, F, H, W, fmt, labels, palette_yuv, nullptr, false, true, a256,
                              contour, out_y, out_y_pitch, out_y_stride, out_uv, out_uv_pitch, out_uv_stride, f_off, o);
  if (st != MDQE_OK || F == 0) return st;
  // the widest form every address of the launch is aligned for
  const int px = (o.m & 15u) == 0 && contour == 0 ? 16 : ((o.m & 3u) == 0 ? 4 : 2);
  RenderYuvArgs a;
  a.y = (const unsigned char*)y;
  a.uv = (const unsigned char*)uv;
  a.labels = labels;
  a.palette = palette_yuv;
  a.oy = o.oy;
  a.ouv = o.ouv;
  a.y_pitch = y_pitch; a.y_stride = y_stride; a.uv_pitch = uv_pitch; a.uv_stride = uv_stride;
  a.oy_pitch = out_y_pitch; a.oy_stride = out_y_stride; a.ouv_pitch = out_uv_pitch; a.ouv_stride = out_uv_stride;
  a.H = H; a.W = W;
  a.XU = (unsigned)((W + px - 1) / px);
  a.RP = (unsigned)((H + 1) / 2);
  a.n_units = (unsigned)F * a.RP * a.XU;                             // <= F * H * W < 2^31
  a.a256 = (uint32_t)a256;
  mdqe_clear_error();
  const dim3 grid((a.n_units + 255u) / 256u);
  if (fmt == 0) launch_render_yuv<0>(px, contour, grid, (hipStream_t)stream, a);
  else launch_render_yuv<1>(px, contour, grid, (hipStream_t)stream, a);
  return mdqe_launch_status();
}
