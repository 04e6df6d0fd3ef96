// Decoder surfaces as video input: semi-planar YUV 4:2:0 (NV12, P010) -> planar uint8 RGB [NI, 3, H, W], the tensor the resize and the
// stem take.  ONE definition, integers only (include/mdqe_hip.h has the rule and the constants); tests/_yuv_ref.py restates it in numpy
// and every comparison is exact.
//
// A pure streaming pass: 1.5 bytes in and 3 out per pixel for NV12, 3 in and 3 out for P010.  A thread owns a block of 2 rows by PX
// pixels -- the two rows that share a chroma row -- and the whole batch is one launch of one thread per block, the blocks of a row pair
// consecutive: a wave covers 64 * PX consecutive pixels of a row pair.  PX is a per-launch decision of the entry point:
//   PX = 16  every plane pointer, pitch, stride and W are multiples of 16 bytes: two 16-byte luma loads, one 16-byte chroma load that
//            serves both rows (P010: twice as many), six 16-byte plane stores;
//   PX = 4   the same with multiples of 4: 4-byte accesses;
//   PX = 1   anything else: single samples, consecutive lanes on consecutive pixels.
// W is a multiple of PX in the wide forms (the stores of row r start at r * W), so a wide launch has no row tails; the odd last row of a
// wide launch, and everything of a PX = 1 launch, goes through the per-sample path, which reads luma[r][c] and chroma[r >> 1][2 * (c >> 1)
// + {0, 1}] for r < H, c < W only: no padding is touched, no row past the planes' last.  No LDS, no atomics, registers only.
#include "common.h"

namespace {

struct YuvArgs {
  const unsigned char* y;
  const unsigned char* uv;
  unsigned char* out;
  long y_pitch, y_stride, uv_pitch, uv_stride;   // bytes
  long plane;                                    // H * W
  long o_r, o_b;                                 // byte offsets of the R and B planes inside an output frame (G is plane 1)
  int H, W;
  unsigned XU, RP, n_units;                      // blocks per row pair, row pairs per surface, NI * RP * XU
  int yo, co, cy, rv, gu, gv, bu;
};

// clamp(x >> 16, 0, 255), written as the clamp of x to 0 .. 2^24 - 1 in front of the shift: the same function (floor is monotonic, and
// x >> 16 <= 255 exactly when x < 2^24).  Why: with the shift first the compiler paired two of them into v_ashr_pk_u8_i32, and the wide
// form built that way returned wrong bytes on the device while the same source, run on the host, gave the rule.  The cause is NOT
// established (the compiler's use of the instruction, the instruction itself, or something else in that build); this order compiles to
// v_med3_i32 and a shift.  Nothing stops a later toolchain from forming the pattern again: the exact comparisons of
// tests/test_yuv_gpu.py are the guard.
__device__ __forceinline__ uint32_t clamp8(int x) {
  x = x < 0 ? 0 : (x > 0xFFFFFF ? 0xFFFFFF : x);
  return (uint32_t)x >> 16;
}

// sample i of a row chunk held in dwords: a byte (NV12), or the top 10 bits of a little-endian 16-bit word (P010)
template <int FMT>
__device__ __forceinline__ int chunk_sample(const uint32_t* w, int i) {
  return FMT == 0 ? (int)((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) : (int)(((w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu) >> 6);
}

// sample i of a plane row in memory
template <int FMT>
__device__ __forceinline__ int row_sample(const unsigned char* row, int i) {
  return FMT == 0 ? (int)row[i] : (int)(((const unsigned short*)row)[i] >> 6);
}

template <int BYTES, int ALIGN>
__device__ __forceinline__ void ld_chunk(uint32_t* dst, const unsigned char* p) {
  __builtin_memcpy(dst, __builtin_assume_aligned(p, ALIGN), BYTES);
}

template <int FMT, int PX>
__global__ __launch_bounds__(256) void yuv420sp_to_rgb_kernel(const YuvArgs a) {
  const unsigned u = blockIdx.x * 256u + threadIdx.x;
  if (u >= a.n_units) return;
  const unsigned rpn = u / a.XU, xu = u - rpn * a.XU;              // row pair over the batch, block of the row pair
  const unsigned n = rpn / a.RP, rp = rpn - n * a.RP;
  const int r0 = 2 * (int)rp, c0 = PX * (int)xu;
  constexpr int BPS = FMT ? 2 : 1;                                   // bytes per sample
  const unsigned char* yrow = a.y + n * a.y_stride + (long)r0 * a.y_pitch;
  const unsigned char* crow = a.uv + n * a.uv_stride + (long)rp * a.uv_pitch;
  unsigned char* o = a.out + 3L * n * a.plane + (long)r0 * a.W + c0;
  if constexpr (PX > 1) if (r0 + 1 < a.H) {
    // the wide path: rows r0 and r0 + 1, pixels c0 .. c0 + PX - 1 (c0 + PX <= W: W is a multiple of PX in a wide launch)
    constexpr int NW = PX * BPS / 4;
    uint32_t yw[2][NW], cw[NW], ow[2][3][PX / 4];
    ld_chunk<4 * NW, PX>(yw[0], yrow + (long)c0 * BPS);
    ld_chunk<4 * NW, PX>(yw[1], yrow + a.y_pitch + (long)c0 * BPS);
    ld_chunk<4 * NW, PX>(cw, crow + (long)c0 * BPS);               // c0 is even: pair c0 / 2 starts at sample c0
#pragma unroll
    for (int p = 0; p < PX / 2; ++p) {
      const int cu = chunk_sample<FMT>(cw, 2 * p) - a.co, cv = chunk_sample<FMT>(cw, 2 * p + 1) - a.co;
      const int tr = a.rv * cv + 32768, tg = a.gu * cu + a.gv * cv + 32768, tb = a.bu * cu + 32768;
#pragma unroll
      for (int row = 0; row < 2; ++row) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int i = 2 * p + k;
          const int yy = (chunk_sample<FMT>(yw[row], i) - a.yo) * a.cy;
          const uint32_t R = clamp8(yy + tr), G = clamp8(yy + tg), B = clamp8(yy + tb);
          if ((i & 3) == 0) {
            ow[row][0][i >> 2] = R; ow[row][1][i >> 2] = G; ow[row][2][i >> 2] = B;
          } else {
            ow[row][0][i >> 2] |= R << (8 * (i & 3)); ow[row][1][i >> 2] |= G << (8 * (i & 3)); ow[row][2][i >> 2] |= B << (8 * (i & 3));
          }
        }
      }
    }
#pragma unroll
    for (int row = 0; row < 2; ++row) {
      unsigned char* q = o + (long)row * a.W;
      __builtin_memcpy(__builtin_assume_aligned(q + a.o_r, PX), ow[row][0], PX);
      __builtin_memcpy(__builtin_assume_aligned(q + a.plane, PX), ow[row][1], PX);
      __builtin_memcpy(__builtin_assume_aligned(q + a.o_b, PX), ow[row][2], PX);
    }
    return;
  }
  {
    // the per-sample path: the rule as written, every bound checked
    for (int i = 0; i < PX; ++i) {
      const int c = c0 + i;
      if (c >= a.W) break;
      const int cu = row_sample<FMT>(crow, 2 * (c >> 1)) - a.co, cv = row_sample<FMT>(crow, 2 * (c >> 1) + 1) - a.co;
      const int tr = a.rv * cv + 32768, tg = a.gu * cu + a.gv * cv + 32768, tb = a.bu * cu + 32768;
      for (int row = 0; row < 2 && r0 + row < a.H; ++row) {
        const int yy = (row_sample<FMT>(yrow + (long)row * a.y_pitch, c) - a.yo) * a.cy;
        unsigned char* q = o + (long)row * a.W + i;
        q[a.o_r] = (unsigned char)clamp8(yy + tr);
        q[a.plane] = (unsigned char)clamp8(yy + tg);
        q[a.o_b] = (unsigned char)clamp8(yy + tb);
      }
    }
  }
}

template <int FMT>
void launch_yuv(int px, dim3 grid, hipStream_t stream, const YuvArgs& a) {
  switch (px) {
    case 16: hipLaunchKernelGGL((yuv420sp_to_rgb_kernel<FMT, 16>), grid, dim3(256), 0, stream, a); break;
    case 4: hipLaunchKernelGGL((yuv420sp_to_rgb_kernel<FMT, 4>), grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((yuv420sp_to_rgb_kernel<FMT, 1>), grid, dim3(256), 0, stream, a); break;
  }
}

}  // namespace

extern "C" int mdqe_yuv420sp_to_rgb_u8(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                       int NI, int H, int W, int fmt, int matrix, int full_range, int bgr, unsigned char* out,
                                       void* stream) {
  static const int coeffs[8][7] = MDQE_YUV_COEFFS;
  MDQE_REQUIRE(NI >= 0 && H > 0 && W > 0 && (fmt == 0 || fmt == 1) && (matrix == 0 || matrix == 1));
  const long bps = fmt ? 2 : 1;
  MDQE_REQUIRE(y_pitch >= bps * W && uv_pitch >= bps * 2 * ((W + 1L) / 2) && y_stride >= 0 && uv_stride >= 0);
  if (fmt == 1) MDQE_REQUIRE(((y_pitch | y_stride | uv_pitch | uv_stride) & 1L) == 0);
  MDQE_REQUIRE((long)NI * 3 * H * W < 0x80000000L);                  // the block index of one call is 32-bit
  if (NI == 0) return MDQE_OK;
  MDQE_CHECK_PTR(y);
  MDQE_CHECK_PTR(uv);
  MDQE_CHECK_PTR(out);
  if (fmt == 1) MDQE_REQUIRE((((uintptr_t)y | (uintptr_t)uv) & 1u) == 0);
  // the widest form every address of the launch is aligned for (strides matter only between surfaces)
  uintptr_t m = (uintptr_t)y | (uintptr_t)uv | (uintptr_t)out | (uintptr_t)y_pitch | (uintptr_t)uv_pitch | (uintptr_t)W;
  if (NI > 1) m |= (uintptr_t)y_stride | (uintptr_t)uv_stride;
  const int px = (m & 15u) == 0 ? 16 : ((m & 3u) == 0 ? 4 : 1);
  const int* k = coeffs[4 * fmt + 2 * matrix + (full_range ? 1 : 0)];
  YuvArgs a;
  a.y = (const unsigned char*)y;
  a.uv = (const unsigned char*)uv;
  a.out = out;
  a.y_pitch = y_pitch; a.y_stride = y_stride; a.uv_pitch = uv_pitch; a.uv_stride = uv_stride;
  a.plane = (long)H * W;
  a.o_r = bgr ? 2 * a.plane : 0;
  a.o_b = bgr ? 0 : 2 * a.plane;
  a.H = H; a.W = W;
  a.XU = (unsigned)((W + px - 1) / px);
  a.RP = (unsigned)((H + 1) / 2);
  a.n_units = (unsigned)NI * a.RP * a.XU;                            // <= NI * H * W < 2^31
  a.yo = k[0]; a.co = k[1]; a.cy = k[2]; a.rv = k[3]; a.gu = k[4]; a.gv = k[5]; a.bu = k[6];
  mdqe_clear_error();
  const dim3 grid((a.n_units + 255u) / 256u);
  if (fmt == 0) launch_yuv<0>(px, grid, (hipStream_t)stream, a);
  else launch_yuv<1>(px, grid, (hipStream_t)stream, a);
  return mdqe_launch_status();
}
