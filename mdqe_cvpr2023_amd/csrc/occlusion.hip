// The occlusion table of a window: how much of each track's final mask every track owns -- the masks counted against each other, from
// the sweep that decides them (the shape of score_ops.hip's counts against ground truth).  No mask and no label map leaves the device.
#include "common.h"
#include "final_mask.h"

// ------------------------------------------------------------------------------------------------
// With b_k(f, Y, X) the final-mask bit of selected row k (final_mask_bit of final_mask_value_at: the dense masks' own bit) and o(f, Y, X)
// the pixel's owner (final_owner_takes over ALL selected rows: the label map's own choice, -1 where no bit is set),
//   occ[k, f, j] = #{(Y, X) : b_k set and o == j}                      int32 [n_sel, Fw, n_sel].
// A block owns a band of output rows of one frame for a CHUNK of the k axis (blockIdx.x = frame * n_bands + band index, blockIdx.y =
// chunk; rows [k0, k0 + kc)): the taps of a pixel are computed once, the loop over all n_sel rows reads, blends and thresholds, keeps
// the owner and, for the chunk's rows ONLY (occlusion_slot: a row of another chunk leaves no bit, so no count ever aims past the
// block's table), the bits in two 64-bit words a lane (kc <= 128).  Counting, into the block's LDS table [kc, n_sel]:
//   the diagonal per WAVE -- most pixels carry no bit or one, and then k == o: for each distinct owner among the wave's 64 pixels (of
//   this chunk) one ballot, one popcount and ONE LDS integer atomic by one lane;
//   the rest per LANE -- only a lane whose pixel carries a chunk bit that is not its owner's (a pixel inside an overlap) walks those
//   bits, one LDS integer atomic each.
// After the band every non-zero entry of the table goes out with one global integer atomic.  Integers only: the result does not depend
// on any order.  LDS: ids[n_sel] | tab[kc * n_sel], at most 64 KB: kc <= 16384 / n_sel - 1 (occlusion_chunk).
// ------------------------------------------------------------------------------------------------
// Rows of the k axis a block takes: the fewest chunks whose table [kc, n_sel] fits, beside ids[n_sel], the 64 KB a block gets without a
// function attribute, shared out evenly.  n_sel <= 127: one chunk; 255: five of 51.
static inline int occlusion_chunk(int n_sel) {
  const int most = 16384 / n_sel - 1;
  const int chunks = (n_sel + most - 1) / most;
  return (n_sel + chunks - 1) / chunks;
}

// (dynamic LDS of a block: ids[n_sel] | tab[chunk, n_sel])
static inline long occlusion_lds_bytes(int n_sel, int chunk) { return (long)n_sel * (chunk + 1) * (long)sizeof(int); }

// The row of a block's table that selected row k counts into, for the block whose chunk is rows [k0, k0 + kc): k - k0, or -1 for a row
// of another chunk.  The kernel's only way from a row to a table row, and what mdqe_final_masks_occlusion_plan reports.
__host__ __device__ __forceinline__ int occlusion_slot(int k, int k0, int kc) {
  const int r = k - k0;
  return r >= 0 && r < kc ? r : -1;
}

__global__ void __launch_bounds__(256)
final_mask_occlusion_kernel(const float* __restrict__ lg, int n_sel, int Fw, int Hm, int Wm, int factor, int h, int w, int Ho, int Wo,
                            const int* __restrict__ inst_idx, int band, int n_bands, int chunk, int* __restrict__ occ) {
  extern __shared__ int occlusion_lds[];
  int* ids = occlusion_lds;
  int* tab = occlusion_lds + n_sel;
  const int k0 = blockIdx.y * chunk, kc = min(chunk, n_sel - k0);
  const int f = blockIdx.x / n_bands, b = blockIdx.x - f * n_bands;
  const float sy_scale = (float)h / (float)Ho, sx_scale = (float)w / (float)Wo;
  const int Y0 = b * band, rows = min(band, Ho - Y0);
  const long map_stride = (long)Hm * Wm;
  for (int k = threadIdx.x; k < n_sel; k += 256) ids[k] = inst_idx[k];
  for (int i = threadIdx.x; i < kc * n_sel; i += 256) tab[i] = 0;
  __syncthreads();
  const int npix = rows * Wo, lane = threadIdx.x & 63;
  // (every lane runs every trip, a lane past the band with valid = false: the ballots need whole waves)
  for (int i0 = 0; i0 < npix; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const bool valid = i < npix;
    const int ic = valid ? i : npix - 1;
    const int y = ic / Wo, X = ic - y * Wo, Y = Y0 + y;
    const MaskTaps t = final_mask_taps(Hm, Wm, factor, h, w, sy_scale, sx_scale, Y, X);
    int best = -1;
    float best_v = 0.f;
    unsigned long long m0 = 0ull, m1 = 0ull;                         // the bits of rows k0 .. k0 + 63 | k0 + 64 .. k0 + 127
    for (int k = 0; k < n_sel; ++k) {
      const float v = final_mask_value_at(lg + ((long)ids[k] * Fw + f) * map_stride, Wm, t);
      const int bit = valid ? final_mask_bit(v) : 0;
      if (final_owner_takes(bit, v, best, best_v)) { best = k; best_v = v; }
      const int r = occlusion_slot(k, k0, kc);                       // (the same for every lane: a scalar branch)
      if (r >= 0 && r < 64) m0 |= (unsigned long long)bit << r;
      else if (r >= 64) m1 |= (unsigned long long)bit << (r - 64);
    }
    // the diagonal: the pixels whose owner is a row of this chunk, one atomic per distinct owner of the wave
    const int own = best - k0;
    const bool mine = best >= 0 && own >= 0 && own < kc;
    unsigned long long left = __ballot(mine);
    while (left != 0ull) {
      const int src = __ffsll((long long)left) - 1;
      const int o = __shfl(own, src);
      const unsigned long long same = __ballot(mine && own == o);
      if (lane == src) atomicAdd(tab + o * n_sel + (k0 + o), __popcll(same));
      left &= ~same;
    }
    // the rest: the chunk's bits of this pixel that are not its owner's -- the part of row k that row `best` hides
    if (mine) {
      if (own < 64) m0 &= ~(1ull << own);
      else m1 &= ~(1ull << (own - 64));
    }
    while (m0 != 0ull) {
      atomicAdd(tab + (__ffsll((long long)m0) - 1) * n_sel + best, 1);
      m0 &= m0 - 1ull;
    }
    while (m1 != 0ull) {
      atomicAdd(tab + (63 + __ffsll((long long)m1)) * n_sel + best, 1);
      m1 &= m1 - 1ull;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kc * n_sel; i += 256) {
    const int c = tab[i];
    if (c) {
      const int k = i / n_sel, j = i - k * n_sel;
      atomicAdd(occ + ((long)(k0 + k) * Fw + f) * n_sel + j, c);
    }
  }
}

// The launch plan on its own, for a host that wants to see it (and for the tests, which hold it to its bounds for every n_sel).
extern "C" int mdqe_final_masks_occlusion_plan(int n_sel, int* chunk, int* chunks, long* lds_bytes, int* slots) {
  MDQE_REQUIRE(n_sel >= 1 && n_sel <= 255);
  MDQE_CHECK_PTR(chunk); MDQE_CHECK_PTR(chunks); MDQE_CHECK_PTR(lds_bytes);
  const int c = occlusion_chunk(n_sel), n = (n_sel + c - 1) / c;
  *chunk = c; *chunks = n; *lds_bytes = occlusion_lds_bytes(n_sel, c);
  if (slots != nullptr)
    for (int b = 0; b < n; ++b)
      for (int k = 0; k < n_sel; ++k) slots[b * n_sel + k] = occlusion_slot(k, b * c, c < n_sel - b * c ? c : n_sel - b * c);
  return MDQE_OK;
}

extern "C" int mdqe_final_masks_occlusion(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                                          int h, int w, int Ho, int Wo, int* occ, void* stream) {
  MDQE_TRY(final_mask_args(n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo));
  MDQE_REQUIRE(n_sel <= 255 && (long)Ho * Wo < 0x7FFFFFFFL && (long)Hm * Wm < 0x7FFFFFFFL && (long)n_sel * n_sel * Fw < 0x7FFFFFFFL);
  if (n_sel == 0 || Fw == 0) return MDQE_OK;
  MDQE_CHECK_PTR(logits); MDQE_CHECK_PTR(inst_idx_dev); MDQE_CHECK_PTR(occ);
  const int chunk = occlusion_chunk(n_sel);
  const int chunks = (n_sel + chunk - 1) / chunk;
  // bands per frame as in mdqe_final_label_map_u8, the chunks of a frame sharing them out
  const int band = final_mask_band(2048, (long)Fw * chunks, Ho, Wo);
  const int n_bands = (Ho + band - 1) / band;
  MDQE_REQUIRE((long)Fw * n_bands < 0x7FFFFFFFL);
  const size_t lds = (size_t)occlusion_lds_bytes(n_sel, chunk);
  mdqe_clear_error();
  if (hipMemsetAsync(occ, 0, (size_t)n_sel * Fw * n_sel * sizeof(int), (hipStream_t)stream) != hipSuccess) return MDQE_ELAUNCH;
  hipLaunchKernelGGL(final_mask_occlusion_kernel, dim3((unsigned)(Fw * n_bands), (unsigned)chunks), dim3(256), lds, (hipStream_t)stream, logits,
                     n_sel, Fw, Hm, Wm, factor, h, w, Ho, Wo, inst_idx_dev, band, n_bands, chunk, occ);
  return mdqe_launch_status();
}
