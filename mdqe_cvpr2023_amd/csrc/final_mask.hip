// The final-mask family: a tracker window's mean logits to dense masks, their geometry, their COCO run boundaries and the label map.
// The pixel is in final_mask.h, shared with the overlap counts of score_ops.hip; so are the entry points' argument check and band plan.
#include "common.h"
#include "final_mask.h"
#include <cstdlib>

// ------------------------------------------------------------------------------------------------
// Final masks (mdqe/mdqe.py:357-358 + 458-462): out[i,f,Y,X] = sigmoid(aligned_bilinear_x4(logits)[sy,sx]) > 0.5 with
// (sy,sx) = nearest source pixel of the crop [:h,:w] for an output of (Ho,Wo):  sy = min(floor(Y*h/Ho), h-1).
// aligned_bilinear (util/misc.py:485-507) in closed form: pixel p reads source (max(p - f/2, 0))/f, clamped to the map.
// logits [n, F, Hm, Wm] (mean logits of one tracker window); out uint8 [n, F_total, Ho, Wo] written at frame f_off.
// ------------------------------------------------------------------------------------------------
// (the pixel itself -- final_mask_taps / _value_at / _value / _bit / _pixel -- is in final_mask.h, shared with score_ops.hip)

__global__ void __launch_bounds__(256)
final_mask_kernel(const float* __restrict__ lg, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo,
                  unsigned char* __restrict__ out, long out_inst_stride, int f_off, const int* __restrict__ inst_idx, long total) {
  const float sy_scale = (float)h / (float)Ho, sx_scale = (float)w / (float)Wo;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int X = (int)(i % Wo); long t = i / Wo;
    const int Y = (int)(t % Ho); t /= Ho;
    const int f = (int)(t % Fw); const int k = (int)(t / Fw);
    const float* m = lg + ((long)inst_idx[k] * Fw + f) * Hm * Wm;
    out[(long)k * out_inst_stride + ((long)(f_off + f) * Ho + Y) * Wo + X] = (unsigned char)final_mask_pixel(m, Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, X);
  }
}

// Band form of the same planes, shaped like final_label_map_kernel: a block owns a band of output rows of ONE frame for ALL selected
// rows (blockIdx.x = frame * n_bands + band index) and a thread takes 4 consecutive pixels of an output row.  Where a pixel reads does
// not depend on the track, so final_mask_taps runs once per pixel (32-bit index arithmetic, no 64-bit division) and the loop over k only
// reads, blends (final_mask_value_at) and thresholds (final_mask_bit): the bits of final_mask_kernel by construction.  A track's four
// bytes leave as one dword where the group is whole and its address 4-byte aligned -- decided per address, so an odd Wo, an odd base or
// an odd stride only costs byte stores -- and byte by byte otherwise.
__global__ void __launch_bounds__(256)
final_mask_band_kernel(const float* __restrict__ lg, int n_sel, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo,
                       unsigned char* __restrict__ out, long out_inst_stride, int f_off, const int* __restrict__ inst_idx, int band,
                       int n_bands) {
  const int f = blockIdx.x / n_bands, b = blockIdx.x - f * n_bands;
  const float sy_scale = (float)h / (float)Ho, sx_scale = (float)w / (float)Wo;
  const int Y0 = b * band, rows = min(band, Ho - Y0);
  const long map_stride = (long)Hm * Wm;
  const int Wg = (Wo + 3) >> 2;                        // groups of 4 pixels per output row
  const int ngrp = rows * Wg;
  unsigned char* o = out + ((long)(f_off + f) * Ho + Y0) * Wo;
  for (int i = threadIdx.x; i < ngrp; i += 256) {
    const int y = i / Wg, X0 = (i - y * Wg) << 2, Y = Y0 + y;
    const int nx = min(4, Wo - X0);                    // pixels of the group inside the row
    MaskTaps t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = final_mask_taps(Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, min(X0 + j, Wo - 1));
    unsigned char* og = o + (long)y * Wo + X0;
    for (int k = 0; k < n_sel; ++k) {
      const float* m = lg + ((long)inst_idx[k] * Fw + f) * map_stride;
      unsigned int bits = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) bits |= (unsigned int)final_mask_bit(final_mask_value_at(m, Wm, t[j])) << (8 * j);
      unsigned char* p = og + (long)k * out_inst_stride;
      if (nx == 4 && (reinterpret_cast<unsigned long>(p) & 3) == 0) {
        *reinterpret_cast<unsigned int*>(p) = bits;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nx) p[j] = (unsigned char)((bits >> (8 * j)) & 1u);
      }
    }
  }
}

// Routes to the band kernel.  The flat kernel keeps the outputs only it accepts (Ho * Wo >= 2^31: its pixel index is a long) and stays
// selectable with MDQE_FINAL_MASK_FLAT=1 as the yardstick of tools/mask_path_ab.py and tests/test_final_mask_band_gpu.py.
extern "C" int mdqe_final_masks_u8(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                                   int h, int w, int Ho, int Wo, unsigned char* out, long out_inst_stride, int f_off,
                                   void* stream) {
  MDQE_TRY(final_mask_args(n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo));
  if (n_sel == 0 || Fw == 0) return MDQE_OK;
  MDQE_CHECK_PTR(logits); MDQE_CHECK_PTR(inst_idx_dev); MDQE_CHECK_PTR(out);
  mdqe_clear_error();
  const char* env = getenv("MDQE_FINAL_MASK_FLAT");
  const bool flat = (env != nullptr && env[0] == '1') || (long)Ho * Wo >= 0x7FFFFFFFL || (long)Hm * Wm >= 0x7FFFFFFFL;
  if (!flat) {
    // bands per frame: about 8 blocks of 256 threads per CU over the window, at least ~1024 pixels (one group of 4 per thread) a block
    const int band = final_mask_band(2048, Fw, Ho, Wo);
    const int n_bands = (Ho + band - 1) / band;
    if ((long)Fw * n_bands < 0x7FFFFFFFL && (long)band * ((Wo + 3) / 4) < 0x7FFFFFFFL) {
      hipLaunchKernelGGL(final_mask_band_kernel, dim3((unsigned)(Fw * n_bands)), dim3(256), 0, (hipStream_t)stream, logits, n_sel, Fw, Hm,
                         Wm, factor, h, w, Ho, Wo, out, out_inst_stride, f_off, inst_idx_dev, band, n_bands);
      return mdqe_launch_status();
    }
  }
  const long total = (long)n_sel * Fw * Ho * Wo;
  long nb = (total + 255) / 256; if (nb > 256 * 64) nb = 256 * 64;
  hipLaunchKernelGGL(final_mask_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, logits, Fw, Hm, Wm, factor, h, w, Ho,
                     Wo, out, out_inst_stride, f_off, inst_idx_dev, total);
  return mdqe_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Geometry of the final masks in the sweep that decides them: per (selected row k, window frame f) the number of set
// pixels and their tight box, geom[k*Fw+f] = (area, xmin, ymin, xmax, ymax) in output pixels, inclusive; an empty mask
// is (0, Wo, Ho, -1, -1) (xmin > xmax, ymin > ymax: the convention of image_mask_stats).  What pycocotools' area /
// toBbox (mdqe/data/pycocotools/mask.py:93-101) and d2's BitMasks.get_bounding_boxes (mdqe/mdqe.py:554) compute on the
// host from the masks.  Every bit comes from final_mask_pixel, so masks and geometry cannot disagree.  All integer:
// the result does not depend on the order in which blocks finish.
// ------------------------------------------------------------------------------------------------
struct MaskGeom { int cnt, x0, y0, x1, y1; };

__device__ __forceinline__ void geom_add(MaskGeom& g, int v, int Y, int X) {
  g.cnt += v;
  g.x0 = v ? min(g.x0, X) : g.x0; g.x1 = v ? max(g.x1, X) : g.x1;
  g.y0 = v ? min(g.y0, Y) : g.y0; g.y1 = v ? max(g.y1, Y) : g.y1;
}

// 256 threads: registers -> wave (__shfl_xor over 64 lanes) -> the 4 waves through red[20]; the total is valid in thread 0
__device__ __forceinline__ MaskGeom geom_block_reduce(MaskGeom g, int* red) {
  for (int o = 32; o > 0; o >>= 1) {
    g.cnt += __shfl_xor(g.cnt, o);
    g.x0 = min(g.x0, __shfl_xor(g.x0, o)); g.x1 = max(g.x1, __shfl_xor(g.x1, o));
    g.y0 = min(g.y0, __shfl_xor(g.y0, o)); g.y1 = max(g.y1, __shfl_xor(g.y1, o));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave * 5 + 0] = g.cnt; red[wave * 5 + 1] = g.x0; red[wave * 5 + 2] = g.y0; red[wave * 5 + 3] = g.x1; red[wave * 5 + 4] = g.y1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int wv = 1; wv < 4; ++wv) {
      g.cnt += red[wv * 5 + 0];
      g.x0 = min(g.x0, red[wv * 5 + 1]); g.y0 = min(g.y0, red[wv * 5 + 2]);
      g.x1 = max(g.x1, red[wv * 5 + 3]); g.y1 = max(g.y1, red[wv * 5 + 4]);
    }
  }
  return g;
}

__global__ void __launch_bounds__(256)
geom_init_kernel(int* __restrict__ geom, int rows, int Ho, int Wo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows * 5) { const int c = i % 5; geom[i] = c == 0 ? 0 : c == 1 ? Wo : c == 2 ? Ho : -1; }
}

// Dense form.  final_mask_kernel spreads one mask over many blocks of a flat grid-stride loop; here a block owns a band of
// `band` rows of ONE mask (blockIdx.x = mask * n_bands + band index), so all its pixels share one row of geom: one set of
// integer atomics per block that saw a set pixel, into the row geom_init_kernel prepared.  A band is contiguous in `out`,
// so a wave's byte stores stay contiguous as in final_mask_kernel.
__global__ void __launch_bounds__(256)
final_mask_geom_kernel(const float* __restrict__ lg, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo,
                       unsigned char* __restrict__ out, long out_inst_stride, int f_off, const int* __restrict__ inst_idx,
                       int band, int n_bands, int* __restrict__ geom) {
  const int mask = blockIdx.x / n_bands, b = blockIdx.x - mask * n_bands;
  const int k = mask / Fw, f = mask - k * Fw;
  const float* m = lg + ((long)inst_idx[k] * Fw + f) * Hm * Wm;
  const float sy_scale = (float)h / (float)Ho, sx_scale = (float)w / (float)Wo;
  const int Y0 = b * band, rows = min(band, Ho - Y0);
  unsigned char* o = out + (long)k * out_inst_stride + ((long)(f_off + f) * Ho + Y0) * Wo;
  const int npix = rows * Wo;
  MaskGeom g = {0, Wo, Ho, -1, -1};
#pragma unroll 4                       // (bounded: left alone the compiler unrolls this loop into ~250 VGPRs)
  for (int i = threadIdx.x; i < npix; i += 256) {
    const int y = i / Wo, X = i - y * Wo, Y = Y0 + y;
    const int v = final_mask_pixel(m, Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, X);
    o[i] = (unsigned char)v;
    geom_add(g, v, Y, X);
  }
  __shared__ int red[20];
  g = geom_block_reduce(g, red);
  if (threadIdx.x == 0 && g.cnt > 0) {
    int* r = geom + (long)mask * 5;
    atomicAdd(r + 0, g.cnt);
    atomicMin(r + 1, g.x0); atomicMin(r + 2, g.y0);
    atomicMax(r + 3, g.x1); atomicMax(r + 4, g.y1);
  }
}

// ------------------------------------------------------------------------------------------------
// Final masks straight to COCO run-length form (the result writer's
// mask_util.encode(np.array(mask[:, :, None], order="F")), mdqe/data/ytvis_eval.py:307-312, i.e. cocoapi rleEncode): the
// mask of (instance k, frame f) is never materialised -- one block walks its pixels in COLUMN-major order, every thread a
// contiguous segment, evaluating final_mask_pixel on the fly, and emits the positions p where the value differs from
// p-1 (value before the first pixel = 0).  Runs are the differences of consecutive positions (host).  Two sweeps: count
// per thread -> block scan -> write.  pos [n_sel*Fw, cap], n_pos [n_sel*Fw] (may exceed cap: the host then falls back).
// GEOM: the geometry is gathered in the first sweep and written by one thread -- no atomics, no initialisation.
// ------------------------------------------------------------------------------------------------
template <bool GEOM>
__global__ void __launch_bounds__(256)
final_mask_rle_kernel(const float* __restrict__ lg, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo,
                      const int* __restrict__ inst_idx, int cap, int* __restrict__ pos, int* __restrict__ n_pos,
                      int* __restrict__ geom) {
  const int k = blockIdx.x / Fw, f = blockIdx.x - k * Fw;
  const float* m = lg + ((long)inst_idx[k] * Fw + f) * Hm * Wm;
  const float sy_scale = (float)h / (float)Ho, sx_scale = (float)w / (float)Wo;
  const int total = Ho * Wo;
  const int seg = (total + 255) / 256;
  const int p0 = min((int)threadIdx.x * seg, total), p1 = min(p0 + seg, total);
  int prev0 = 0;
  if (p0 > 0 && p0 < total) prev0 = final_mask_pixel(m, Hm, Wm, factor, h, w, sy_scale, sx_scale, (p0 - 1) % Ho, (p0 - 1) / Ho);
  int cnt = 0, prev = prev0;
  MaskGeom g = {0, Wo, Ho, -1, -1};
  auto count = [&](int p) {
    const int X = p / Ho, Y = p - X * Ho;
    const int v = final_mask_pixel(m, Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, X);
    cnt += (v != prev);
    prev = v;
    if constexpr (GEOM) geom_add(g, v, Y, X);
  };
  // (the unroll bound belongs to the GEOM instance alone: the plain one is left to the compiler's own choice)
  if constexpr (GEOM) {
#pragma unroll 8
    for (int p = p0; p < p1; ++p) count(p);
  } else {
    for (int p = p0; p < p1; ++p) count(p);
  }
  __shared__ int sc[256];
  sc[threadIdx.x] = cnt;
  if constexpr (GEOM) {
    __shared__ int red[20];
    g = geom_block_reduce(g, red);                     // (its barrier also publishes sc[])
    if (threadIdx.x == 0) {
      int* r = geom + (long)blockIdx.x * 5;
      r[0] = g.cnt; r[1] = g.x0; r[2] = g.y0; r[3] = g.x1; r[4] = g.y1;
    }
  } else {
    __syncthreads();
  }
  for (int o = 1; o < 256; o <<= 1) {                  // inclusive scan
    const int add = (int)threadIdx.x >= o ? sc[threadIdx.x - o] : 0;
    __syncthreads();
    sc[threadIdx.x] += add;
    __syncthreads();
  }
  int off = sc[threadIdx.x] - cnt;
  if (threadIdx.x == 255) n_pos[blockIdx.x] = sc[255];
  int* out = pos + (long)blockIdx.x * cap;
  prev = prev0;
  auto emit = [&](int p) {
    const int v = final_mask_pixel(m, Hm, Wm, factor, h, w, sy_scale, sx_scale, p % Ho, p / Ho);
    if (v != prev) { if (off < cap) out[off] = p; ++off; }
    prev = v;
  };
  if constexpr (GEOM) {
#pragma unroll 8
    for (int p = p0; p < p1; ++p) emit(p);
  } else {
    for (int p = p0; p < p1; ++p) emit(p);
  }
}

extern "C" int mdqe_final_masks_rle(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                                    int h, int w, int Ho, int Wo, int cap, int* pos, int* n_pos, void* stream) {
  MDQE_TRY(final_mask_args(n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo));
  MDQE_REQUIRE(cap > 0 && (long)Ho * Wo < 0x7FFFFFFFL);
  if (n_sel == 0 || Fw == 0) return MDQE_OK;
  MDQE_CHECK_PTR(logits); MDQE_CHECK_PTR(inst_idx_dev); MDQE_CHECK_PTR(pos); MDQE_CHECK_PTR(n_pos);
  mdqe_clear_error();
  hipLaunchKernelGGL(final_mask_rle_kernel<false>, dim3((unsigned)(n_sel * Fw)), dim3(256), 0, (hipStream_t)stream, logits, Fw, Hm, Wm, factor,
                     h, w, Ho, Wo, inst_idx_dev, cap, pos, n_pos, nullptr);
  return mdqe_launch_status();
}

extern "C" int mdqe_final_masks_rle_geom(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                                         int h, int w, int Ho, int Wo, int cap, int* pos, int* n_pos, int* geom, void* stream) {
  MDQE_TRY(final_mask_args(n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo));
  MDQE_REQUIRE(cap > 0 && (long)Ho * Wo < 0x7FFFFFFFL);
  if (n_sel == 0 || Fw == 0) return MDQE_OK;
  MDQE_CHECK_PTR(logits); MDQE_CHECK_PTR(inst_idx_dev); MDQE_CHECK_PTR(pos); MDQE_CHECK_PTR(n_pos); MDQE_CHECK_PTR(geom);
  mdqe_clear_error();
  hipLaunchKernelGGL(final_mask_rle_kernel<true>, dim3((unsigned)(n_sel * Fw)), dim3(256), 0, (hipStream_t)stream, logits, Fw, Hm, Wm,
                     factor, h, w, Ho, Wo, inst_idx_dev, cap, pos, n_pos, geom);
  return mdqe_launch_status();
}

extern "C" int mdqe_final_masks_u8_geom(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                                        int h, int w, int Ho, int Wo, unsigned char* out, long out_inst_stride, int f_off,
                                        int* geom, void* stream) {
  MDQE_TRY(final_mask_args(n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo));
  MDQE_REQUIRE((long)Ho * Wo < 0x7FFFFFFFL);
  if (n_sel == 0 || Fw == 0) return MDQE_OK;
  MDQE_CHECK_PTR(logits); MDQE_CHECK_PTR(inst_idx_dev); MDQE_CHECK_PTR(out); MDQE_CHECK_PTR(geom);
  // bands per mask: enough blocks to fill the device when the window holds few masks (about 16 blocks of 256 threads per CU), but
  // at least ~1024 pixels (4 per thread) per block so that the reduction and the atomics stay a small part of a block's work
  const long n_masks = (long)n_sel * Fw;
  MDQE_REQUIRE(n_masks * 5 < 0x7FFFFFFFL);
  const int band = final_mask_band(4096, n_masks, Ho, Wo);
  const int n_bands = (Ho + band - 1) / band;
  MDQE_REQUIRE(n_masks * n_bands < 0x7FFFFFFFL);
  mdqe_clear_error();
  const int rows = (int)n_masks;
  hipLaunchKernelGGL(geom_init_kernel, dim3((unsigned)((rows * 5 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, geom, rows, Ho, Wo);
  hipLaunchKernelGGL(final_mask_geom_kernel, dim3((unsigned)(n_masks * n_bands)), dim3(256), 0, (hipStream_t)stream, logits, Fw, Hm, Wm,
                     factor, h, w, Ho, Wo, out, out_inst_stride, f_off, inst_idx_dev, band, n_bands, geom);
  return mdqe_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Label map: ONE uint8 plane per frame instead of one per track -- which track owns each pixel.  Among the selected rows whose
// final-mask bit is set at the pixel (final_mask_bit of final_mask_value: the dense masks' own bit), the one with the largest
// up-sampled logit wins, the first such row on an exact tie; out = inst_idx[k*] + 1, 0 where no bit is set.  So out != 0 exactly
// on the union of the dense masks, and a label always names a track whose dense mask holds the pixel.
// A block owns a band of output rows of one frame for ALL rows (blockIdx.x = frame * n_bands + band index): the taps of a pixel are
// computed once and the loop over k only reads and blends.  STAGED (opt-in, see the entry point): the source rows the band reads, of
// every selected map, are copied to LDS first (n_sel * src_cap * Wm floats; a band whose rows exceed src_cap reads global memory instead, so the bound is only a
// size, never an assumption).  GEOM: geometry of each label's visible region as mdqe_final_masks_u8_geom lays it out; a thread
// gathers the run of equal labels it meets in registers and adds it to the block's LDS table [n_sel, 5] with LDS integer atomics
// when the label changes; after the band, thread k adds row k -- if the block saw label k -- to geom with global integer atomics.
// LDS: ids[n_sel] | GEOM: tab[n_sel * 5] | STAGED: rows.
// ------------------------------------------------------------------------------------------------
template <bool STAGED, bool GEOM>
__global__ void __launch_bounds__(256)
final_label_map_kernel(const float* __restrict__ lg, int n_sel, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo,
                       unsigned char* __restrict__ out, int f_off, const int* __restrict__ inst_idx, int band, int n_bands, int src_cap,
                       int* __restrict__ geom) {
  extern __shared__ int label_lds[];
  int* ids = label_lds;
  int* tab = label_lds + n_sel;
  float* rows_lds = reinterpret_cast<float*>(label_lds + n_sel + (GEOM ? n_sel * 5 : 0));
  const int f = blockIdx.x / n_bands, b = blockIdx.x - f * n_bands;
  const float sy_scale = (float)h / (float)Ho, sx_scale = (float)w / (float)Wo;
  const int Y0 = b * band, rows = min(band, Ho - Y0);
  const long map_stride = (long)Hm * Wm;
  for (int k = threadIdx.x; k < n_sel; k += 256) ids[k] = inst_idx[k];
  if constexpr (GEOM)
    for (int i = threadIdx.x; i < n_sel * 5; i += 256) { const int c = i % 5; tab[i] = c == 0 ? 0 : c == 1 ? Wo : c == 2 ? Ho : -1; }
  int ylo = 0;
  bool staged = false;
  if constexpr (STAGED) {
    // y0 and y1 do not decrease with Y: the band reads source rows [y0 of its first row, y1 of its last]
    ylo = final_mask_taps(Hm, Wm, factor, h, w, sy_scale, sx_scale, Y0, 0).y0;
    const int nr = final_mask_taps(Hm, Wm, factor, h, w, sy_scale, sx_scale, Y0 + rows - 1, 0).y1 - ylo + 1;
    staged = nr <= src_cap;
    if (staged) {
      const int per = nr * Wm, slot = src_cap * Wm;
      for (int i = threadIdx.x; i < n_sel * per; i += 256) {
        const int k = i / per, j = i - k * per;
        rows_lds[k * slot + j] = lg[((long)inst_idx[k] * Fw + f) * map_stride + (long)ylo * Wm + j];
      }
    }
  }
  __syncthreads();
  unsigned char* o = out + ((long)(f_off + f) * Ho + Y0) * Wo;
  const int npix = rows * Wo;
  int cur = -1;
  MaskGeom g = {0, Wo, Ho, -1, -1};
  auto flush = [&]() {
    if (cur >= 0) {
      int* r = tab + cur * 5;
      atomicAdd(r + 0, g.cnt);
      atomicMin(r + 1, g.x0); atomicMin(r + 2, g.y0);
      atomicMax(r + 3, g.x1); atomicMax(r + 4, g.y1);
    }
  };
  for (int i = threadIdx.x; i < npix; i += 256) {
    const int y = i / Wo, X = i - y * Wo, Y = Y0 + y;
    MaskTaps t = final_mask_taps(Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, X);
    int best = -1;
    float best_v = 0.f;
    if (STAGED && staged) {
      t.y0 -= ylo; t.y1 -= ylo;
      const int slot = src_cap * Wm;
      for (int k = 0; k < n_sel; ++k) {
        const float v = final_mask_value_at(rows_lds + k * slot, Wm, t);
        if (final_owner_takes(final_mask_bit(v), v, best, best_v)) { best = k; best_v = v; }
      }
    } else {
      for (int k = 0; k < n_sel; ++k) {
        const float v = final_mask_value_at(lg + ((long)ids[k] * Fw + f) * map_stride, Wm, t);
        if (final_owner_takes(final_mask_bit(v), v, best, best_v)) { best = k; best_v = v; }
      }
    }
    o[i] = best < 0 ? (unsigned char)0 : (unsigned char)(ids[best] + 1);
    if constexpr (GEOM) {
      if (best != cur) { flush(); cur = best; g = MaskGeom{0, Wo, Ho, -1, -1}; }
      geom_add(g, 1, Y, X);
    }
  }
  if constexpr (GEOM) {
    flush();
    __syncthreads();
    for (int k = threadIdx.x; k < n_sel; k += 256) {
      const int* s = tab + k * 5;
      if (s[0] > 0) {
        int* r = geom + ((long)k * Fw + f) * 5;
        atomicAdd(r + 0, s[0]);
        atomicMin(r + 1, s[1]); atomicMin(r + 2, s[2]);
        atomicMax(r + 3, s[3]); atomicMax(r + 4, s[4]);
      }
    }
  }
}

extern "C" int mdqe_final_label_map_u8(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                                       int h, int w, int Ho, int Wo, unsigned char* out, int f_off, int* geom, void* stream) {
  MDQE_TRY(final_mask_args(n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo));
  MDQE_REQUIRE(n_sel <= 255 && f_off >= 0 && (long)Ho * Wo < 0x7FFFFFFFL && (long)Hm * Wm < 0x7FFFFFFFL);
  if (Fw == 0) return MDQE_OK;
  MDQE_CHECK_PTR(out);
  if (n_sel > 0) { MDQE_CHECK_PTR(logits); MDQE_CHECK_PTR(inst_idx_dev); }
  // bands per frame: about 8 blocks of 256 threads per CU over the window, at least ~1024 pixels (4 per thread, each for all rows) a block
  int band = final_mask_band(2048, Fw, Ho, Wo);
  // The rows are read through the caches by default.  MDQE_LABEL_MAP_STAGE=1 stages them in LDS first where they fit: measured on one
  // MI355X (profiles/label_map_ab.txt, 15 tracks x 30 frames) the staged form is level without geometry (158.7 against 158.3 us at
  // 360p, 484.5 against 480.0 at 640 x 1138) and 12-22 % slower with it (202.8 / 181.4, 636.7 / 523.5): neighbouring output pixels read
  // the same few map rows, so they hit L1 anyway, and the staged form adds the copy, a barrier and 38-52 KB of LDS per block.  Kept for
  // tools/label_map_ab.py and the tests.  A band of `band` output rows spans at most s = ceil((band-1) * h / Ho) + 1 source pixels, hence floor((factor - 1 + s)
  // / factor) + 2 rows of the map; the band is halved until all selected maps' rows fit 64 KB (what a block gets without a function
  // attribute), else the rows are read through the caches after all.
  const bool with_geom = geom != nullptr && n_sel > 0;
  const long head = (long)n_sel * (with_geom ? 6 : 1) * 4;
  const char* env = getenv("MDQE_LABEL_MAP_STAGE");
  bool stage = n_sel > 0 && env != nullptr && env[0] == '1';
  int src_cap = 0;
  int sband = band;
  while (stage) {
    const long s = ((long)(sband - 1) * h + Ho - 1) / Ho + 1;
    long cap = (factor - 1 + s) / factor + 2;
    if (cap > Hm) cap = Hm;
    if (head + (long)n_sel * cap * Wm * 4 <= 64 * 1024) { src_cap = (int)cap; band = sband; break; }
    if (sband <= 2) stage = false;
    sband = (sband + 1) / 2;
  }
  const int n_bands = (Ho + band - 1) / band;
  MDQE_REQUIRE((long)Fw * n_bands < 0x7FFFFFFFL && (long)n_sel * Fw * 5 < 0x7FFFFFFFL);
  const size_t lds = (size_t)(head + (stage ? (long)n_sel * src_cap * Wm * 4 : 0));
  mdqe_clear_error();
  if (with_geom)
    hipLaunchKernelGGL(geom_init_kernel, dim3((unsigned)((n_sel * Fw * 5 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, geom, n_sel * Fw, Ho, Wo);
  const dim3 grid((unsigned)(Fw * n_bands));
#define MDQE_LABEL_LAUNCH(S, G)                                                                                                     \
  hipLaunchKernelGGL((final_label_map_kernel<S, G>), grid, dim3(256), lds, (hipStream_t)stream, logits, n_sel, Fw, Hm, Wm, factor, h, w, \
                     Ho, Wo, out, f_off, inst_idx_dev, band, n_bands, src_cap, geom)
  if (stage) { if (with_geom) MDQE_LABEL_LAUNCH(true, true); else MDQE_LABEL_LAUNCH(true, false); }
  else { if (with_geom) MDQE_LABEL_LAUNCH(false, true); else MDQE_LABEL_LAUNCH(false, false); }
#undef MDQE_LABEL_LAUNCH
  return mdqe_launch_status();
}

// ------------------------------------------------------------------------------------------------
// Soft matte: ONE uint8 plane per frame again, but a weight instead of a name -- the rounded sigmoid of gain * (the largest up-sampled
// logit among the participating rows), final_matte_level: >= 128 exactly where one of their final-mask bits is set, so thresholding the
// matte at 128 gives the union of those rows' dense masks bit for bit.  Row k takes part iff take == NULL or take[inst_idx[k] + 1] != 0
// (the row's label, as in the label map).  Shaped like final_mask_band_kernel: a block owns a band of output rows of one frame for all
// rows, a thread takes 4 consecutive pixels of an output row, final_mask_taps runs once per pixel and the loop over k only reads, blends
// (final_mask_value_at) and thresholds (final_mask_bit); one expf more per PIXEL for the level.  The participating rows' indices are
// packed into LDS first (order kept; 256 threads >= n_sel), so a row `take` drops costs nothing in the sweep.  The four levels leave as
// one dword where the group is whole and its address 4-byte aligned, byte by byte otherwise.  No atomics: identical from run to run.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
final_matte_kernel(const float* __restrict__ lg, int n_sel, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo,
                   unsigned char* __restrict__ out, int f_off, const int* __restrict__ inst_idx, const unsigned char* __restrict__ take,
                   float gain, int band, int n_bands) {
  __shared__ int ids[256];
  __shared__ int wave_rows[4];
  const int tid = (int)threadIdx.x;
  bool on = false;
  int id = 0;
  if (tid < n_sel) {
    id = inst_idx[tid];
    on = take == nullptr || take[(id + 1) & 255] != 0;                // (the table has 256 entries: the index never leaves it)
  }
  const unsigned long long votes = __ballot(on);
  if ((tid & 63) == 0) wave_rows[tid >> 6] = __popcll(votes);
  __syncthreads();
  int first = 0, n_part = 0;
#pragma unroll
  for (int wv = 0; wv < 4; ++wv) { first += wv < (tid >> 6) ? wave_rows[wv] : 0; n_part += wave_rows[wv]; }
  if (on) ids[first + __popcll(votes & ((1ull << (tid & 63)) - 1ull))] = id;
  __syncthreads();
  const int f = blockIdx.x / n_bands, b = blockIdx.x - f * n_bands;
  const float sy_scale = (float)h / (float)Ho, sx_scale = (float)w / (float)Wo;
  const int Y0 = b * band, rows = min(band, Ho - Y0);
  const long map_stride = (long)Hm * Wm;
  const int Wg = (Wo + 3) >> 2;                        // groups of 4 pixels per output row
  const int ngrp = rows * Wg;
  unsigned char* o = out + ((long)(f_off + f) * Ho + Y0) * Wo;
  for (int i = tid; i < ngrp; i += 256) {
    const int y = i / Wg, X0 = (i - y * Wg) << 2, Y = Y0 + y;
    const int nx = min(4, Wo - X0);                    // pixels of the group inside the row
    MaskTaps t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = final_mask_taps(Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, min(X0 + j, Wo - 1));
    float vmax[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int U[4] = {0, 0, 0, 0};
    for (int k = 0; k < n_part; ++k) {
      const float* m = lg + ((long)ids[k] * Fw + f) * map_stride;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = final_mask_value_at(m, Wm, t[j]);
        U[j] |= final_mask_bit(v);
        vmax[j] = v > vmax[j] ? v : vmax[j];
      }
    }
    unsigned int lv = 0;
    if (n_part > 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) lv |= (unsigned int)final_matte_level(gain * vmax[j], U[j]) << (8 * j);
    }
    unsigned char* p = o + (long)y * Wo + X0;
    if (nx == 4 && (reinterpret_cast<unsigned long>(p) & 3) == 0) {
      *reinterpret_cast<unsigned int*>(p) = lv;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nx) p[j] = (unsigned char)(lv >> (8 * j));
    }
  }
}

extern "C" int mdqe_final_matte_u8(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                                   int h, int w, int Ho, int Wo, const unsigned char* take, float gain, unsigned char* out, int f_off,
                                   void* stream) {
  MDQE_TRY(final_mask_args(n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo));
  MDQE_REQUIRE(n_sel <= 255 && f_off >= 0 && (long)Ho * Wo < 0x7FFFFFFFL && (long)Hm * Wm < 0x7FFFFFFFL);
  MDQE_REQUIRE(gain > 0.f && gain <= 64.f);                           // (false for a NaN)
  if (Fw == 0) return MDQE_OK;
  MDQE_CHECK_PTR(out);
  if (n_sel > 0) { MDQE_CHECK_PTR(logits); MDQE_CHECK_PTR(inst_idx_dev); }
  // bands per frame as the label map's: about 8 blocks of 256 threads per CU over the window, at least ~1024 pixels a block
  const int band = final_mask_band(2048, Fw, Ho, Wo);
  const int n_bands = (Ho + band - 1) / band;
  MDQE_REQUIRE((long)Fw * n_bands < 0x7FFFFFFFL && (long)band * ((Wo + 3) / 4) < 0x7FFFFFFFL);
  mdqe_clear_error();
  hipLaunchKernelGGL(final_matte_kernel, dim3((unsigned)(Fw * n_bands)), dim3(256), 0, (hipStream_t)stream, logits, n_sel, Fw, Hm, Wm,
                     factor, h, w, Ho, Wo, out, f_off, inst_idx_dev, take, gain, band, n_bands);
  return mdqe_launch_status();
}
