// fp32 NT GEMM / NHWC implicit-GEMM convolution on the gfx950 matrix cores.
//
//   C[m, n] = epilogue( sum_k A(m, k) * W[n, k] )          A, W, C fp32; exact fp32 arithmetic
//
// v_mfma_f32_32x32x2_f32 (f32 in / f32 accumulate; bit-for-bit an fmaf chain, 157 TFLOP/s peak)
// is used because the path's parity bar is fp32 (north star: 1e-3 against the fp32 CPU path).
//
// Serves every Linear / 1x1 conv / KxK conv on the hot path:
//   * plain mode:  A(m,k) = A[m*lda + k]
//   * conv mode:   m = (img, oh, ow), k = (kh, kw, cin) over an NHWC input; zero padding comes
//                  from the buffer-descriptor bounds check (out-of-range lanes return 0).
// W is [N][K] row-major (nn.Linear layout; convs are pre-packed [Cout][KH][KW][Cin]).
//
// Structure (CDNA4): block tile BM x BN, K-step 32 floats (one 128-B line per row).  Tiles go
// HBM/L2 -> LDS with buffer_load ... lds (16 B per lane, 1 KiB per wave-instruction, no VGPR round
// trip), double buffered; the load of step k+1 is issued before the MFMAs of step k.  LDS rows are
// 128 B; the 16-B chunk index is XOR-swizzled with (row>>1)&7 on the *source* side (the LDS write
// of an LDS-DMA is lane-linear) and on the ds_read_b128 side, which makes every 16-lane read group
// hit 16 distinct 16-B slots (conflict-free).  One ds_read_b128 per operand feeds four MFMAs:
// lanes 0-31 carry k = 4c..4c+3 of their row, lanes 32-63 carry the next four.
#include "gemm_device.h"

template <int BM, int BN, int WM, int WN, bool CONV>
__global__ void __launch_bounds__(64 * WM * WN)
gemm_nt_f32_kernel(const GemmParams p) {
  constexpr int NW = WM * WN;
  constexpr int BK = 32;
  constexpr int MT = BM / WM / 32, NT = BN / WN / 32;
  constexpr int ROWS = BM + BN;              // A rows then W rows in one LDS image
  constexpr int NINST = ROWS / 8;            // 1-KiB LDS-DMA instructions per stage
  constexpr int IPW = NINST / NW;            // per wave
  static_assert(NINST % NW == 0, "tile rows must split evenly over waves");
  extern __shared__ __attribute__((aligned(16))) float lds[];   // 2 * ROWS * 32 floats

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  // XCD-aware tile order: blocks that share an A row-panel run on the same XCD (same L2).
  const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  const int nblk = nbm * nbn;
  const int bid = gemm_xcd_tile(blockIdx.x, nblk);
  const int bm = bid / nbn, bn = bid % nbn;
  const int m0 = bm * BM, n0 = bn * BN;

  const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, p.a_bytes, 0x00020000);
  const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)p.W, 0, p.w_bytes, 0x00020000);

  // Per-lane source bookkeeping for this lane's IPW rows (fixed over the K loop).
  // instruction j of this wave covers image rows (wave*IPW + j)*8 .. +7; lane -> row += lane>>3, chunk' = lane&7,
  // source chunk = (lane&7) ^ ((row>>1)&7).  voff[j] = byte offset of (row, k = 4*chunk); the K-step rides on the
  // instruction's scalar offset (plain rows, W rows) or on the filter-tap offset (conv A rows; kept in the VGPR offset
  // because a padded pixel's base may be "negative" and the scalar offset is not part of the bounds check).
  unsigned voff[IPW];
  int ih0[IPW], iw0[IPW], kch[IPW];
#pragma unroll
  for (int j = 0; j < IPW; ++j) {
    const int irow = (wave * IPW + j) * 8 + (lane >> 3);
    kch[j] = ((lane & 7) ^ ((irow >> 1) & 7)) * 4;
    ih0[j] = 0; iw0[j] = 0;
    if (irow < BM) {
      int m = m0 + irow; if (m > p.M - 1) m = p.M - 1;
      if (CONV) {
        voff[j] = gemm_conv_row(p, m, ih0[j], iw0[j]) + (unsigned)(kch[j] * 4);
      } else {
        voff[j] = (unsigned)((long)m * p.lda * 4) + (unsigned)(kch[j] * 4);
      }
    } else {
      int n = n0 + irow - BM; if (n > p.N - 1) n = p.N - 1;
      voff[j] = (unsigned)((long)n * p.K * 4) + (unsigned)(kch[j] * 4);
    }
  }

  const int kbeg = p.ksplit > 1 ? blockIdx.y * p.kchunk : 0;
  const int kend = p.ksplit > 1 ? min(p.K, kbeg + p.kchunk) : p.K;
  const int kt0 = kbeg / BK;
  const int nk = (kend - kbeg + BK - 1) / BK;
  // conv: filter tap of the K-step about to be issued (the 32-float K-step lies inside one tap: Cin % 32 == 0, host-checked)
  int t_kh = 0, t_kw = 0, t_c = 0;
  if (CONV) gemm_tap_seek(p, kbeg, t_kh, t_kw, t_c);

  auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
    const int k0 = kt * BK;
    const bool ktail = k0 + BK > p.K;              // only the last K-step of a ragged K (plain mode) checks lanes against K
    float* base = lds + buf * (ROWS * BK);
    int tap_off = 0;
    if (CONV) tap_off = gemm_tap_bytes(p, t_kh, t_kw, t_c);
#pragma unroll
    for (int j = 0; j < IPW; ++j) {
      const int irow0 = (wave * IPW + j) * 8;        // wave-uniform
      unsigned off = voff[j];
      if (irow0 < BM) {
        if (CONV) {
          off = gemm_tap_addr(p, ih0[j] + t_kh, iw0[j] + t_kw, off, tap_off);
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(base + irow0 * BK), 16, off, 0, 0, 0);
        } else {
          if (ktail && k0 + kch[j] >= p.K) off = OOB_OFF;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(base + irow0 * BK), 16, off, k0 * 4, 0, 0);
        }
      } else {
        if (ktail && k0 + kch[j] >= p.K) off = OOB_OFF;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)(base + irow0 * BK), 16, off, k0 * 4, 0, 0);
      }
    }
    if (CONV) gemm_tap_advance(p, BK, t_kh, t_kw, t_c);
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int lr = lane & 31, lh = lane >> 5;
  issue(kt0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's LDS-DMA for step kt has landed
    __syncthreads();                                   // ... and everybody else's; all reads of the other buffer are done
    if (kt + 1 < nk) issue(kt0 + kt + 1, (kt + 1) & 1);
    const float* sA = lds + (kt & 1) * (ROWS * BK);
    const float* sW = sA + BM * BK;
    // fragments of sub-step kk+1 are fetched before the MFMAs of kk are issued (LDS latency behind 16 MFMAs)
    f32x4 fa_[2][MT], fb_[2][NT];
    auto frag = [&](int kk, int slot) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int row = wm * (BM / WM) + i * 32 + lr;
        const int ch = (kk * 2 + lh) ^ ((row >> 1) & 7);
        fa_[slot][i] = *reinterpret_cast<const f32x4*>(sA + row * BK + ch * 4);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int row = wn * (BN / WN) + j * 32 + lr;
        const int ch = (kk * 2 + lh) ^ ((row >> 1) & 7);
        fb_[slot][j] = *reinterpret_cast<const f32x4*>(sW + row * BK + ch * 4);
      }
    };
    frag(0, 0);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      if (kk < 3) frag(kk + 1, (kk + 1) & 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa_[kk & 1][i][s], fb_[kk & 1][j][s], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue ---------------------------------------------------------------------------------
  // acc[i][j][r] is C(row = gemm_acc_row(r, lh), col = lr) of a 32x32 sub-tile.  The tile is restaged through LDS (free
  // after the K loop) for gemm_tile_out, which applies the epilogue (rolled: see gemm_k16.hip's) or writes the split-K partial.
  __syncthreads();                                   // every wave is done reading the last K-step
  float* sC = lds;                                   // [BM][BN] floats (== 2 stage buffers when BM == BN)
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * (BM / WM) + i * 32 + gemm_acc_row(r, lh);
        const int col = wn * (BN / WN) + j * 32 + lr;
        sC[row * BN + col] = acc[i][j][r];
      }
  __syncthreads();
  gemm_tile_out<BM, BN, 64 * NW, 1>(p, sC, m0, n0, tid);
}

template <int BM, int BN, int WM, int WN, bool CONV>
static int launch_gemm_(const GemmParams& p, hipStream_t st) {
  const int nbm = (p.M + BM - 1) / BM, nbn = (p.N + BN - 1) / BN;
  size_t smem = 2 * (BM + BN) * 32 * sizeof(float);
  if (smem < (size_t)BM * BN * sizeof(float)) smem = (size_t)BM * BN * sizeof(float);   // epilogue restage
  auto kern = gemm_nt_f32_kernel<BM, BN, WM, WN, CONV>;
  if (smem > 64 * 1024 && mdqe_allow_lds(reinterpret_cast<const void*>(kern), (int)smem) != hipSuccess) return MDQE_ELAUNCH;
  hipLaunchKernelGGL(kern, dim3(nbm * nbn, p.ksplit > 1 ? p.ksplit : 1), dim3(64 * WM * WN), smem, st, p);
  return mdqe_launch_status();
}

// tile: 1 128x128, 2 128x64, 3 / 7 / 8 / 9 64x64; the split-K reduce pass is launched by the caller
int mdqe_launch_gemm_k32(const GemmParams& p, int tile, hipStream_t st) {
  switch (tile) {
    case 1: return p.conv ? launch_gemm_<128, 128, 2, 2, true>(p, st) : launch_gemm_<128, 128, 2, 2, false>(p, st);
    case 2: return p.conv ? launch_gemm_<128, 64, 2, 2, true>(p, st) : launch_gemm_<128, 64, 2, 2, false>(p, st);
    case 3: case 7: case 8: case 9: return p.conv ? launch_gemm_<64, 64, 2, 2, true>(p, st) : launch_gemm_<64, 64, 2, 2, false>(p, st);
    default: return MDQE_EINVAL;
  }
}
