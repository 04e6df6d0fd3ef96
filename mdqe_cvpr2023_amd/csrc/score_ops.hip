// Scoring a window's final masks against ground truth on the device: the overlap counts behind the video IoU of the YTVIS evaluator
// (mdqe/data/pycocotools/ytvoseval.py:173-219, iou_seq :200-214), from the sweep that decides the masks.  No mask leaves the device.
#include "common.h"
#include "final_mask.h"

// ------------------------------------------------------------------------------------------------
// With b_k(f, Y, X) the final-mask bit of selected row k (final_mask_bit of final_mask_value: the dense masks' own bit) and gt the
// packed ground truth (bit g of gt[f_off + f, Y, X]: ground-truth track g holds the pixel; tracks may overlap),
//   inter[k, g] += #{(f, Y, X) of the window : b_k and bit g},     area[k, f] = #{(Y, X) : b_k}.
// A block owns a band of output rows of one frame for a chunk of up to OVERLAP_ROWS selected rows (blockIdx.x = frame * n_bands + band
// index, blockIdx.y = chunk): the taps of a pixel are computed once and the ground-truth word is read once, 4 bytes a lane, contiguous
// over the band.  Counting is per WAVE, not per lane: of the 64 pixels a wave holds, lane g (g < G) keeps ballot(bit g) -- built only
// when some lane of the wave holds a ground-truth bit at all -- and lane G an all-ones mask; for each row, one ballot of b_k, nothing
// more when it is zero (most rows, most waves), else lanes 0..G each take popcount(ballot(b_k) & theirs) and add what is non-zero to
// the block's LDS table [rows, G + 1] (column G: the area) with an LDS integer atomic.  After the band, every non-zero entry of the
// table goes out with ONE global integer atomic (64-bit for inter).  Integers only: the result does not depend on any order.
// LDS: ids[rows] | tab[rows * (G + 1)], at most 256 * 34 * 4 = 34 KB.
// ------------------------------------------------------------------------------------------------
#define OVERLAP_ROWS 256

__global__ void __launch_bounds__(256)
final_mask_overlap_kernel(const float* __restrict__ lg, int n_sel, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo,
                          const uint32_t* __restrict__ gt, int G, int f_off, const int* __restrict__ inst_idx, int band, int n_bands,
                          unsigned long long* __restrict__ inter, long inter_row_stride, int* __restrict__ area) {
  extern __shared__ int overlap_lds[];
  const int k0 = blockIdx.y * OVERLAP_ROWS, kc = min(OVERLAP_ROWS, n_sel - k0), cols = G + 1;
  int* ids = overlap_lds;
  int* tab = overlap_lds + kc;
  const int f = blockIdx.x / n_bands, b = blockIdx.x - f * n_bands;
  const float sy_scale = (float)h / (float)Ho, sx_scale = (float)w / (float)Wo;
  const int Y0 = b * band, rows = min(band, Ho - Y0);
  const long map_stride = (long)Hm * Wm;
  for (int k = threadIdx.x; k < kc; k += 256) ids[k] = inst_idx[k0 + k];
  for (int i = threadIdx.x; i < kc * cols; i += 256) tab[i] = 0;
  __syncthreads();
  const uint32_t* gp = gt + ((long)(f_off + f) * Ho + Y0) * Wo;
  const int npix = rows * Wo, lane = threadIdx.x & 63;
  // (every lane runs every trip, a lane past the band with valid = false: the ballots and the masks lanes 0..G keep need whole waves)
  for (int i0 = 0; i0 < npix; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool valid = i < npix;
    const int ic = valid ? i : npix - 1;
    const int y = ic / Wo, X = ic - y * Wo, Y = Y0 + y;
    const MaskTaps t = final_mask_taps(Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, X);
    const uint32_t word = valid ? gp[i] : 0u;
    unsigned long long mine = lane == G ? ~0ull : 0ull;
    if (__ballot(word != 0u) != 0ull) {
      for (int g = 0; g < G; ++g) {
        const unsigned long long bg = __ballot((word >> g) & 1u);
        if (lane == g) mine = bg;
      }
    }
    for (int k = 0; k < kc; ++k) {
      const float v = final_mask_value_at(lg + ((long)ids[k] * Fw + f) * map_stride, Wm, t);
      const unsigned long long bk = __ballot(valid && final_mask_bit(v));
      if (bk == 0ull) continue;
      if (lane <= G) {
        const int c = __popcll(bk & mine);
        if (c) atomicAdd(tab + k * cols + lane, c);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kc * cols; i += 256) {
    const int c = tab[i];
    if (c) {
      const int k = i / cols, g = i - k * cols;
      if (g < G) atomicAdd(inter + (long)(k0 + k) * inter_row_stride + g, (unsigned long long)c);
      else atomicAdd(area + (long)(k0 + k) * Fw + f, c);
    }
  }
}

extern "C" int mdqe_final_masks_overlap(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                                        int h, int w, int Ho, int Wo, const uint32_t* gt_bits, int G, int f_off,
                                        unsigned long long* inter, long inter_row_stride, int* area, void* stream) {
  MDQE_TRY(final_mask_args(n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo));
  MDQE_REQUIRE(f_off >= 0 && (long)Ho * Wo < 0x7FFFFFFFL && (long)Hm * Wm < 0x7FFFFFFFL);
  MDQE_REQUIRE(G >= 1 && G <= 32 && inter_row_stride >= G && (long)n_sel * Fw < 0x7FFFFFFFL);
  if (n_sel == 0 || Fw == 0) return MDQE_OK;
  MDQE_CHECK_PTR(logits); MDQE_CHECK_PTR(inst_idx_dev); MDQE_CHECK_PTR(gt_bits); MDQE_CHECK_PTR(inter); MDQE_CHECK_PTR(area);
  // bands per frame as in mdqe_final_label_map_u8
  const int chunks = (n_sel + OVERLAP_ROWS - 1) / OVERLAP_ROWS;
  const int band = final_mask_band(2048, (long)Fw * chunks, Ho, Wo);
  const int n_bands = (Ho + band - 1) / band;
  MDQE_REQUIRE((long)Fw * n_bands < 0x7FFFFFFFL && chunks <= 65535);
  const int kc = n_sel < OVERLAP_ROWS ? n_sel : OVERLAP_ROWS;
  const size_t lds = (size_t)kc * (G + 2) * sizeof(int);
  mdqe_clear_error();
  if (hipMemsetAsync(area, 0, (size_t)n_sel * Fw * sizeof(int), (hipStream_t)stream) != hipSuccess) return MDQE_ELAUNCH;
  hipLaunchKernelGGL(final_mask_overlap_kernel, dim3((unsigned)(Fw * n_bands), (unsigned)chunks), dim3(256), lds, (hipStream_t)stream, logits,
                     n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo, gt_bits, G, f_off, inst_idx_dev, band, n_bands, inter, inter_row_stride, area);
  return mdqe_launch_status();
}
