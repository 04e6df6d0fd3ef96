/* mdqe_hip.h -- C ABI of libmdqe_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the MDQE eval-only hot path.  Plain pointers and sizes
 * only; every pointer is a DEVICE pointer unless marked host; `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  All entry points are asynchronous on `stream`, never allocate,
 * never synchronise, borrow their inputs and fully overwrite their outputs (graph-capturable).
 * Return value: 0 on success, otherwise one of the MDQE_E* codes; kernel-launch failures are
 * reported through the return value (the reference only printf-s them,
 * mdqe/models/ops/src/cuda/ms_deform_im2col_cuda.cuh:948-952).
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   mdqe_msda_forward_f32      <- ms_deform_attn_forward  (mdqe/models/ops/src/vision.cpp:13-16,
 *                                 src/ms_deform_attn.h:20-39, src/cuda/ms_deform_attn_cuda.cu:20-80),
 *                                 kernel ms_deformable_im2col_gpu_kernel (ms_deform_im2col_cuda.cuh:237-299)
 *   everything else            <- ATen/cuDNN/cuBLAS kernels the reference reaches through PyTorch on
 *                                 the same path (SURVEY.md §2a "Fused ops / ATen kernels"); each
 *                                 prototype names the reference call site it serves.
 *   mdqe_render_overlay_u8     <- the demo's host-side painting (demo/clip/visualizer.py:83-170, overlay_instances: matplotlib
 *                                 polygons blended at alpha 0.5 per frame); here one streaming kernel behind the label map, its
 *                                 own integer rule (below), not the demo's anti-aliased picture.
 */
#ifndef MDQE_HIP_H
#define MDQE_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDQE_OK 0
#define MDQE_EINVAL 1   /* bad size / unsupported shape */
#define MDQE_ELAUNCH 2  /* hipGetLastError() != hipSuccess after launch */
#define MDQE_ENULL 3    /* null pointer */
#define MDQE_ESTATE 4   /* the object was left inconsistent by an earlier failed call (tracker: a device error in the middle of an update) and refuses further use */

/* activation codes for fused epilogues */
#define MDQE_ACT_NONE 0
#define MDQE_ACT_RELU 1
#define MDQE_ACT_GELU 2 /* exact erf GELU (nn.GELU default) */
#define MDQE_ACT_SIGMOID 3
#define MDQE_ACT_TANH 4

/* ABI version of this header: bumped whenever an existing entry point changes what it reads or WRITES under an unchanged signature.
 *   6: mdqe_f16x3_split_f32 writes THREE planes (6*n bytes; versions < 6 wrote two, 4*n bytes) -- a caller that sized its buffer for an
 *      older header must not call a newer library.  mdqe_abi_version() returns the library's value; a binding compares it with the
 *      MDQE_ABI_VERSION it was written against before the first call (mdqe_cvpr2023_amd/_lib.py does, and refuses a mismatch). */
#define MDQE_ABI_VERSION 6
int mdqe_abi_version(void);
int mdqe_version(void);
const char* mdqe_strerror(int code);

/* ---- a9: multi-scale deformable attention sampling -------------------------------------------
 * out[b,q,m,:] = sum_l sum_p attn[b,q,m,l,p] * bilinear_zero_pad(value_l[b,:,m,:], loc[b,q,m,l,p])
 * value [B,S,M,D] f32; shapes [L,2] int64 (H,W); level_start [L] int64; loc [B,Q,M,L,P,2] (x,y in
 * [0,1] image-normalised, pixel = loc*size - 0.5); attn [B,Q,M,L,P]; out [B,Q,M*D].
 * Same argument meaning as ms_deform_attn_cuda_forward (ms_deform_attn_cuda.cu:20-80); im2col_step
 * is a batching artefact of the reference launcher and has no equivalent here. */
int mdqe_msda_forward_f32(const float* value, const int64_t* shapes, const int64_t* level_start,
                          const float* loc, const float* attn,
                          int B, int S, int M, int D, int L, int Q, int P,
                          float* out, void* stream);

/* Backward of the same op (ms_deform_attn_cuda_backward, src/cuda/ms_deform_attn_cuda.cu:83-153; kernels
 * ms_deform_im2col_cuda.cuh:87-234,301-920): grad_out [B,Q,M*D] -> grad_value [B,S,M,D] (zeroed here, then float
 * atomics), grad_loc [B,Q,M,L,P,2], grad_attn [B,Q,M,L,P].  Not on the eval path; completes the extension's two exports. */
int mdqe_msda_backward_f32(const float* value, const int64_t* shapes, const int64_t* level_start, const float* loc,
                           const float* attn, const float* grad_out, int B, int S, int M, int D, int L, int Q, int P,
                           float* grad_value, float* grad_loc, float* grad_attn, void* stream);

/* The same two exports in float64 -- the reference dispatches float and double (AT_DISPATCH_FLOATING_TYPES,
 * src/cuda/ms_deform_attn_cuda.cu:64 forward, :134 backward) and its own test script checks the double forward against the
 * PyTorch core and the backward by gradcheck in double (mdqe/models/ops/test.py:32-44, :63-86).  csrc/msda_f64.hip. */
int mdqe_msda_forward_f64(const double* value, const int64_t* shapes, const int64_t* level_start, const double* loc,
                          const double* attn, int B, int S, int M, int D, int L, int Q, int P, double* out, void* stream);
int mdqe_msda_backward_f64(const double* value, const int64_t* shapes, const int64_t* level_start, const double* loc,
                           const double* attn, const double* grad_out, int B, int S, int M, int D, int L, int Q, int P,
                           double* grad_value, double* grad_loc, double* grad_attn, void* stream);

/* Grouped form used for temporal_clip_forward (mdqe/models/ops/modules/ms_deform_attn.py:219-236):
 * the reference issues G (= #spatial levels) separate native calls that share loc/attn and averages
 * them.  Here: shapes/level_start are [G*L] tables into ONE value buffer, out = scale * sum_g (...). */
int mdqe_msda_forward_grouped_f32(const float* value, const int64_t* shapes, const int64_t* level_start,
                                  const float* loc, const float* attn,
                                  int B, int S, int M, int D, int G, int L, int Q, int P,
                                  float scale, float* out, void* stream);

/* Fused module core (ops/modules/ms_deform_attn.py:141-170 / 198-235): consumes the projection GEMM's raw
 * outputs.  value rows are ldv floats apart, batch b starts at row (vidx ? vidx[b] : b)*v_brows (vidx: device
 * int32[B], lets a batch of overlapping clips address one per-frame value cache); offs row t=(b*Q+q) holds
 * M*L*P*2 floats, logits row t holds M*L*P.  mode 0 (encoder): loc = ref_xy + off/8.  mode 1 (decoder):
 * loc = ref_xy + (grid*0.5*wh + clamp(off, +-8*wh))/8 with ref = (cx,cy,w,h) and grid [M,L,P,2] (device).
 * ref row = b*ref_bstride + q*ref_dim (ref_bstride 0 broadcasts one table over the batch).
 * Level tables (HOST int[G*L]): H, W, start row -- any rows of the element's block, in any order, with gaps; the
 * forms that stage coarse levels in LDS are taken only where those levels lie back to back in ascending order.
 * out row t, ldout floats apart; out = scale * sum_g(...).
 * value_rows = number of rows of the value buffer (> 0 enables the bounds-checked buffer-load kernel; 0 = unknown). */
int mdqe_msda_fused_f32(const float* value, long ldv, long v_brows, const int* vidx, const float* offs, long ldo,
                        const float* logits, long ldl, const float* ref, long ref_bstride, int ref_dim,
                        int mode, const float* grid, const int* lvH_host, const int* lvW_host,
                        const int* lvStart_host, int B, int M, int D, int G, int L, int Q, int P, float scale,
                        float* out, long ldout, long value_rows, void* stream);

/* ---- fp32 NT GEMM with fused epilogue (v_mfma_f32_32x32x2_f32, exact fp32) ----------------------
 * C[m,n] = mask( act(sum_k A[m*lda+k] * W[n*K+k] + bias[n]) + residual[(res_mod? m%res_mod : m)*ldr + n] )
 * (res_first != 0: the residual is added before the activation instead, as in a ResNet bottleneck)
 * Serves nn.Linear / 1x1 conv call sites of the path: value_proj/output_proj/sampling_offsets/
 * attention_weights (ops/modules/ms_deform_attn.py:136-171), FFNs (transformer_enc.py:106,
 * transformer_dec.py:356,406), MLP heads (models/misc.py:6-18), MHA projections
 * (transformer_dec.py:350,399), input_proj 1x1 (models/mdqe.py:34-37), dynamic mask product
 * (mdqe/mdqe.py:384).  K % 4 == 0, lda % 4 == 0, A/W 16-B aligned.  act applies to columns
 * < act_cols (<=0: all); rowmask (u8, 1 = zero the row) applies to columns < mask_cols
 * (the masked_fill of ms_deform_attn.py:137-138).  tile: 0 auto, 1 128x128, 2 128x64, 3 64x64
 * (4 64x256 and 5 128x256 -- whole 256-wide rows per block -- are measured alternatives, not picked by auto).
 * ksplit > 1: K is cut into ksplit chunks over blockIdx.y, partial tiles go to splitk_ws (>= ksplit*M*N floats)
 * and a second pass sums them in fixed order and applies the epilogue (deterministic; for skinny large-K products). */
int mdqe_gemm_nt_f32(const float* A, long lda, const float* W, const float* bias, float* C, long ldc,
                     int M, int N, int K, int act, int act_cols, const float* residual, long ldr, int res_mod,
                     int res_first, const unsigned char* rowmask, int mask_cols, int tile, int ksplit,
                     float* splitk_ws, const void* w_split, void* stream);

/* The last 1x1 conv of a ResNet bottleneck and its projection shortcut as ONE product (detectron2 BottleneckBlock.forward:
 * out = relu(conv3(y) + shortcut(x)), both with folded FrozenBN; the reference reaches them through cuDNN):
 * C = act([A1 | A2'] W^T + bias) with W = [W3 | Ws] along K and bias = b3 + bs, so the shortcut's output is never written and read
 * back.  A1 [M = NI*OH*OW, K1] rows of pitch lda1; A2 the block's input, NHWC [NI, H2, W2, lda2 >= K2], read at pixel
 * (oh*stride, ow*stride) for output row (img, oh, ow).  K1, K2 multiples of 16.  Exact fp32 MFMA. */
int mdqe_gemm_nt_cat2_f32(const float* A1, long lda1, int K1, const float* A2, long lda2, int K2, int NI, int OH, int OW,
                          int H2, int W2, int stride, const float* W, const float* bias, float* C, long ldc, int N, int act,
                          void* stream);

/* The strided 1x1 conv1 of an MSRA bottleneck (detectron2 BottleneckBlock with STRIDE_IN_1X1 True, the downsampling block of
 * res3..res5, folded FrozenBN; configs/R101_coco.yaml, R101_ytvis19.yaml; the reference reaches it through cuDNN):
 * C[(img, oh, ow), :] = act(A[img, oh*stride, ow*stride, :] W^T + bias).  A NHWC [NI, H, W, lda >= K]; C [M = NI*OH*OW, ldc];
 * W [N, K].  (OH - 1)*stride < H and (OW - 1)*stride < W (a 1x1 conv without padding: OH = (H - 1)/stride + 1).  K a multiple
 * of 16, any H, W.  Exact fp32 MFMA; the row addressing of mdqe_gemm_nt_cat2_f32's second operand. */
int mdqe_gemm_nt_pix_f32(const float* A, long lda, int K, int NI, int H, int W, int OH, int OW, int stride, const float* Wt,
                         const float* bias, float* C, long ldc, int N, int act, void* stream);

/* Linear + residual + LayerNorm in one kernel, for the encoder / decoder pattern  x = norm(x + dropout(linear(..)))
 * (transformer_enc.py:100-110, transformer_dec.py:352-358,404-409; nn.LayerNorm over d_model = 256):
 * C = LN(A W^T + bias + residual) * gamma + beta, N must be 256; C may alias the residual.  Exact fp32 MFMA. */
int mdqe_gemm_ln_f32(const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N, int K,
                     const float* residual, long ldr, const float* gamma, const float* beta, float eps, void* stream);
/* ... followed by a second LayerNorm of the result in the same epilogue: C2 = LN(C) * gamma2 + beta2 (the decoder's shared
 * `decoder_norm` behind `norm3`, transformer_dec.py:492-495); C2 equals mdqe_layernorm_f32(C) bit for bit. */
int mdqe_gemm_ln2_f32(const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N, int K,
                      const float* residual, long ldr, const float* gamma, const float* beta, const float* gamma2, const float* beta2,
                      float* C2, long ldc2, float eps, void* stream);

/* A projection of `x + pos` whose pos is a linear function of four numbers per row -- the decoder's query position embedding
 * point2pos_proj(box centre) (mdqe/models/transformer_dec.py:42,469,480,495,503), consumed as `x + pos` by the self-attention q/k
 * projections (:348-353, :397-402) and by the sampling-offset / attention-weight projections of cross_attn / temp_attn_inst
 * (ops/modules/ms_deform_attn.py:141-147,198-203):  C = A W^T + bias;  C[:, n < side_cols] += side [M,4] . side_w[n, 0:4]
 * with side_w = W P and the bias carrying W b_P (folded once on the host).  The [M, C] position tensor is never materialised and
 * the q, k (with position) and v (without) projections of one x are ONE product.  side_cols % 4 == 0. */
int mdqe_gemm_nt_side_f32(const float* A, long lda, const float* W, const float* bias, float* C, long ldc, int M, int N, int K,
                          const float* side, const float* side_w, int side_cols, const void* w_split, void* stream);

/* GEMM arithmetic of the 128x128 tile (process-wide): 0 = exact fp32 MFMA (default), 1 = "f16x3": operands split
 * in-kernel into f16 hi + scaled f16 lo, three f16 MFMAs with fp32 accumulation (~1e-6 relative to fp32; |x| < 32752);
 * 2 = "f16" (round 5): ONE f16 MFMA pass -- both operands rounded to nearest f16, fp32 accumulation, fp32 result -- on the
 * products whose constant weight has planes (mdqe_f16x3_split_f32) and that fill the 128-row tile, exact fp32 everywhere
 * else: the arithmetic of the reference's fp16-autocast regions on a GPU (train_net.py:207) with an fp32 instead of an fp16
 * result (operand error 2^-11 relative; |x| < 65504).  Never the default and never the headline mode. */
int mdqe_set_gemm_precision(int mode);
int mdqe_get_gemm_precision(void);   /* the mode the CALLING thread's launches use (its override if set, else the process-wide one) */
/* The calling host thread's override of the mode: 0 / 1 / 2, or -1 = none (follow the process-wide mode).  Lets one region of the model --
 * the regions the reference's harness runs under fp16 autocast (train_net.py:207) -- take the split-precision kernels
 * while another host thread's launches (the sharded schedule's tracker replay) keep theirs. */
int mdqe_set_gemm_precision_thread(int mode);

/* One-time split of a CONSTANT weight tensor W (n = N*K fp32 values, row-major [N][K]) into the two f16 planes the
 * f16x3 mode consumes + the one mode 2 consumes: planes = { hi[n], lo[n], rn[n] } (6*n bytes), hi = f16_rtz(w),
 * lo = f16_rtz((w - hi) * 2048), rn = f16_rne(w).
 * Passing the planes as `w_split` to mdqe_gemm_nt_f32 / mdqe_conv2d_nhwc_f32 (NULL = none) lets mode 1 stream them
 * straight into LDS (gemm_f16x3w.hip: 128 x 256 tiles, no in-kernel weight conversion); requires K % 32 == 0 and
 * max|w| < 32752 (f16 range, caller-checked).  Ignored in mode 0.  Weights are constants of the eval path (nn.Linear / conv
 * parameters, FrozenBatchNorm folded), so this replaces no reference call. */
int mdqe_f16x3_split_f32(const float* w, long n, void* planes, void* stream);

/* tools/ only: while buf != NULL the f16x3w GEMM kernel writes 4 s_memtime stamps per block (start, prologue done, K loop done,
 * end) to buf[block*4 ..]; NULL (default) disables. */
int mdqe_debug_gemm_stamps(void* buf);
/* tools/ only: fp32 GEMM kernel form, 0 = K-step 32 (gemm.hip), 1 = K-step 16 (gemm_k16.hip), 2 = chosen by shape (default). */
int mdqe_debug_gemm_variant(int v);
int mdqe_debug_gemm_tile_rule(int v); /* auto tile rule variants (tools/ A/B); 0 = default */
int mdqe_debug_gemm_rows_dot(int v); /* products with N <= 8 columns: 1 (default) = rows_dot_kernel, 0 = MFMA tiles */
int mdqe_debug_gemm_fast_epilogue(int v); /* K-step-16 kernel (tools/ A/B): 1 (default) = interior tiles of plain products take the few-instruction epilogue, 0 = the general one */
int mdqe_debug_gemm_stagger(int v);  /* K-step-16 kernel: start offset between the blocks of a CU's first round, 10-ns ticks; 0 = off */
int mdqe_debug_gemm_stages(int v);   /* K-step-16 kernel, 64x64 and smaller tiles: LDS stages 2 / 4; 0 = by grid size (default) */
int mdqe_debug_msda_dec_stage_kb(int kb);   /* tools/ only: LDS staging budget of the decoder's box-level deformable launch (default 72: two blocks per CU) */
int mdqe_debug_trk_fast(int on);            /* tests / tools: 1 (default; env MDQE_TRK_FAST) = a tracker update takes its counts through mdqe_trk_siou_host_f32, 0 = memset + kernel + copy + synchronize */
int mdqe_debug_trk_spin_us(int us);         /* how long the tracker polls the counts' flag before falling back to a stream synchronize (default 2000; env MDQE_TRK_SPIN_US) */
int mdqe_debug_trk_times(double* out5, int on);   /* tools: host seconds of the tracker updates since the last call -- counts launch, counts wait, decision, accumulate launch, updates -- then reset; on != 0 keeps timing */
int mdqe_debug_trk_siou_blocks(int blocks);   /* tools/ only: blocks the tracker's sign-intersection launch aims at (0 = default 512) */
int mdqe_debug_gemm_lds_pad(int bytes);   /* tools/ only: extra dynamic LDS per block of the K-step-16 GEMM launches (caps the blocks per CU) */
/* tools/ only: window attention kernel form, 1 = MFMA where it applies (default), 0 = scalar everywhere. */
int mdqe_debug_window_attn_variant(int v);
int mdqe_debug_msda_xcd_order(int v); /* fused MSDA: 1 = XCD-aware block order (default), 0 = plain */
int mdqe_debug_msda_dec_staged(int v); /* fused MSDA, decoder box-level launch: 1 (default) = LDS-staged kernel, 0 = v2 */
int mdqe_debug_msda_dec_wpe8(int v);   /* fused MSDA, the decoder's 832-thread launches: 1 = the 8-waves-per-SIMD build (tools/ A/B), 0 = natural allocation */
int mdqe_debug_msda_patch(int v);      /* fused MSDA, encoder launch: 1 = a block iteration takes an 8 x 16 patch of queries, 0 (default; MDQE_MSDA_PATCH) = a run of 128 tokens */
int mdqe_debug_msda_stage_kb(int v);   /* fused MSDA (encoder / box level): LDS budget in KB of the staged coarse levels (default 150); tools/ A/B */
int mdqe_debug_msda_tp_staged(int v);  /* fused MSDA, decoder temporal launch: 1 (default) = frame-by-frame LDS staging (msda_fused_tp_kernel), 0 = v2 */
int mdqe_debug_msda_op_staged(int v); /* native MSDA op: 1 (default) = coarse levels staged in LDS (msda_fwd_v3_kernel), 0 = v2 */
int mdqe_debug_msda_variant(int v);   /* fused MSDA (tools/ only), bit field: block-to-query map 0 / 1 / 2 of the gather form; +4: its 8-waves-per-SIMD
                                        * hint; +8: coarse levels staged in LDS; (v >> 4) & 7: queries per block 32 << (k - 1); +128: 512-thread blocks;
                                        * +256: no 8-waves-per-SIMD build of the staged encoder kernel; +1024: first staged level as a compile-time
                                        * constant (a level's 16 corner loads in flight); -1 = default (by shape) */
int mdqe_debug_mha_variant(int v);   /* same for the 196-token decoder self-attention */

/* ---- NHWC convolution as implicit GEMM on the same kernel ---------------------------------------
 * X [NI,H,W,Cin] (Cin % 32 == 0; images x_img_stride floats apart, <=0: dense), Wt [Cout,KH,KW,Cin], Y [NI*OH*OW, ldy] ; zero padding; fused bias,
 * activation and residual; ksplit > 1: deterministic split-K as in mdqe_gemm_nt_f32 (workspace >= ksplit*NI*OH*OW*Cout floats)
 * (ResNet bottlenecks -- detectron2 build_resnet_backbone, call site
 * mdqe/mdqe.py:27,33; input_proj 3x3 s2 models/mdqe.py:40-43; MaskHead 3x3 segmentation.py:42-57). */
int mdqe_conv2d_nhwc_f32(const float* X, long x_img_stride, const float* Wt, const float* bias, float* Y, long ldy,
                         int NI, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                         int act, const float* residual, long ldr, int res_first, int tile, const void* w_split,
                         int ksplit, float* splitk_ws, void* stream);

/* ---- stride-1, pad-1 3x3 convolution as fp32 Winograd F(2x2,3x3) (csrc/winograd.hip) ------------
 * The same product as mdqe_conv2d_nhwc_f32(..., KH = KW = 3, stride = 1, pad = 1, no residual) in the exact fp32 mode, with 2.25x
 * fewer matrix multiplies; max-abs error about 1.8x the direct kernel's.  Weights are transformed once:
 * mdqe_winograd_weight_f32 turns the packed [Cout,3,3,Cin] weight into U [16][Cout][Cin] (computed in double, rounded once).
 * mdqe_conv3x3_winograd_f32: X [NI,H,W,Cin] (Cin % 32 == 0; images x_img_stride floats apart, <= 0: dense), Y [NI*H*W, ldy]
 * (Cout % 4 == 0, ldy % 4 == 0), fused bias and activation; workspace >= mdqe_winograd_workspace_bytes(NI, H, W, Cin, Cout) bytes,
 * one per stream.  MDQE_EINVAL outside the exact fp32 GEMM mode (mdqe_set_gemm_precision). */
int mdqe_winograd_weight_f32(const float* Wt, int Cout, int Cin, float* U, void* stream);
long mdqe_winograd_workspace_bytes(int NI, int H, int W, int Cin, int Cout);
int mdqe_conv3x3_winograd_f32(const float* X, long x_img_stride, const float* U, const float* bias, float* Y, long ldy,
                              int NI, int H, int W, int Cin, int Cout, int act, void* workspace, long ws_bytes, void* stream);
int mdqe_debug_winograd_tile(int tile);   /* tools/ A/B: K-step-16 tile code of the plane products (0 = by shape) */

/* ---- eval-time frame resize (ResizeShortestEdgeClip -> ResizeTransform -> PIL Image.resize(BILINEAR) on uint8 frames,
 * mdqe/data/augmentation.py:364-389, dataset_mapper.py:252-258), Pillow's two-pass fixed-point resampling bit for bit.
 * in: NI images [C,H,W] u8, in_img_stride bytes apart; out [NI,C,oh,ow] u8.  Coefficient tables (DEVICE int32), built on the
 * host: per output column X taps xmin[X] .. xmin[X]+xcnt[X]-1 with 22-bit weights xk[X*kxs + t]; same for rows. */
int mdqe_resize_pil_bilinear_u8(const unsigned char* in, long in_img_stride, int NI, int C, int H, int W, int oh, int ow,
                                const int* xmin, const int* xcnt, const int* xk, int kxs, const int* ymin, const int* ycnt,
                                const int* yk, int kys, unsigned char* out, void* stream);

/* ---- decoder surfaces as video input: semi-planar YUV 4:2:0 (NV12, P010) -> planar uint8 RGB, the tensor the entry above and the stem
 * take (csrc/yuv.hip).  What a hardware decoder or a capture device hands out: a luma plane of H rows and a chroma plane of ceil(H/2)
 * rows of interleaved U, V pairs, ceil(W/2) pairs per row; rows y_pitch / uv_pitch BYTES apart, surfaces y_stride / uv_stride BYTES
 * apart, the two planes independent of each other (views into one decoder allocation: chroma at pitch * aligned_height).  Any H >= 1,
 * W >= 1.  ONE definition, integers only:
 *   samples   Y = luma[r][c], U = chroma[r >> 1][2 * (c >> 1)], V = chroma[r >> 1][2 * (c >> 1) + 1]: chroma is replicated (nearest),
 *             what libyuv's and most decoders' default NV12 conversion does;
 *   fmt 0     NV12: samples are bytes;
 *   fmt 1     P010: samples are little-endian 16-bit words, the value is word >> 6 (10 bits, 0..1023; the low 6 bits are ignored);
 *   rule      y = (Y - yo) * cy, u = U - co, v = V - co in int32, >> the arithmetic shift (floor):
 *               R = clamp((y          + rv * v + 32768) >> 16, 0, 255)
 *               G = clamp((y + gu * u + gv * v + 32768) >> 16, 0, 255)
 *               B = clamp((y + bu * u          + 32768) >> 16, 0, 255)
 *   constants rint(x * 65536) of the standard matrices: luma gain 255/219 (limited, 8 bit), 255/876 (limited, 10 bit), 1 (full, 8 bit)
 *             or 255/1023 (full, 10 bit); chroma gains 2(1-Kr), -2Kb(1-Kb)/Kg, -2Kr(1-Kr)/Kg, 2(1-Kb) times 255/224, 255/896, 1 or
 *             255/1023; Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709), Kg = 1 - Kr - Kb.  MDQE_YUV_COEFFS below holds them,
 *             row = 4 * fmt + 2 * matrix + full_range, columns yo, co, cy, rv, gu, gv, bu.  |accumulator| < 3.7e7: int32 is safe.  Every
 *             output lies within 1 level of clamp(rint(the float64 matrix)).
 * out: [NI, 3, H, W] uint8, contiguous, planes R, G, B (bgr != 0: B, G, R).  MDQE_EINVAL, before any pointer is looked at, for H or W
 * <= 0, NI < 0, fmt / matrix outside {0, 1}, a pitch smaller than a row (W samples of luma, 2 * ceil(W/2) of chroma), a negative
 * stride, odd P010 pitches or strides, and NI * 3 * H * W >= 2^31; NI == 0 returns OK and launches nothing; odd P010 plane pointers are
 * MDQE_EINVAL.  Nothing else needs to be aligned: where every plane pointer, pitch, stride and W are multiples of 16 (or of 4) bytes
 * the launch moves 16 (4) bytes per access, otherwise single samples.  Reads stay inside W samples of a luma row, 2 * ceil(W/2) of a
 * chroma row, H luma rows and ceil(H/2) chroma rows: padding is never touched.  Never allocates, never synchronises. */
#define MDQE_YUV_COEFFS { \
  {16, 128, 76309, 104597, -25675, -53279, 132201}, /* nv12 bt601 limited */ \
  {0, 128, 65536, 91881, -22553, -46802, 116130},   /* nv12 bt601 full    */ \
  {16, 128, 76309, 117489, -13975, -34925, 138438}, /* nv12 bt709 limited */ \
  {0, 128, 65536, 103206, -12276, -30679, 121609},  /* nv12 bt709 full    */ \
  {64, 512, 19077, 26149, -6419, -13320, 33050},    /* p010 bt601 limited */ \
  {0, 512, 16336, 22903, -5622, -11666, 28947},     /* p010 bt601 full    */ \
  {64, 512, 19077, 29372, -3494, -8731, 34610},     /* p010 bt709 limited */ \
  {0, 512, 16336, 25726, -3060, -7647, 30313}       /* p010 bt709 full    */ }
int mdqe_yuv420sp_to_rgb_u8(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                            int NI, int H, int W, int fmt /*0 nv12, 1 p010*/, int matrix /*0 bt601, 1 bt709*/, int full_range,
                            int bgr, unsigned char* out /* [NI, 3, H, W] contiguous */, void* stream);

/* ---- LayerNorm over the last dim: y = LN(x + res) * gamma + beta (res may be NULL) -----------------
 * nn.LayerNorm call sites transformer_enc.py:103-108,136; transformer_dec.py:345-358,394-408,466,492. */
int mdqe_layernorm_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y,
                       long rows, int C, float eps, void* stream);

/* ---- GroupNorm on NHWC [NI, HW, C] (+ fused activation); workspace >= mdqe_groupnorm_workspace_bytes --
 * nn.GroupNorm call sites models/mdqe.py:36,42; segmentation.py:21-26,104-105,112. */
long mdqe_groupnorm_workspace_bytes(int NI, int G);
int mdqe_groupnorm_nhwc_f32(const float* x, long ldx, long x_img_stride, float* y, long ldy, long y_img_stride,
                            int NI, int HW, int C, int G,
                            const float* gamma, const float* beta, float eps, int act, void* workspace, void* stream);

/* ---- stem: (x-mean)/std (mdqe/mdqe.py:473-484) + zero pad to /32 (ImageList.from_tensors, mdqe.py:318)
 * + 7x7/s2/p3 im2col -> [NI*Hp/2*Wp/2, 160] (K=147 zero-padded) for the stem GEMM.
 * frames: NI CHW images (u8 or f32) h x w, frame_stride elements apart; mean/std are HOST float[3]. */
int mdqe_stem_im2col_f32(const void* frames, int is_u8, long frame_stride, int NI, int h, int w, int Hp, int Wp,
                         const float* mean3_host, const float* std3_host, float* out, void* stream);

/* ---- the same stem as ONE kernel: normalise + zero pad + 7x7/s2/p3 conv (3->64) + bias (folded FrozenBN) + ReLU, frames ->
 * NHWC activation [NI, Hp/2, Wp/2, 64]; no im2col buffer (mdqe/mdqe.py:473-484,318 + detectron2 BasicStem used by
 * mdqe/models/backbone.py).  wk: DEVICE float[154*64], k-major with k = kh*22 + kw*3 + c and entry kh*22+21 zero;
 * bias: DEVICE float[64]; mean/std HOST float[3]. */
int mdqe_stem_conv_f32(const void* frames, int is_u8, long frame_stride, int NI, int h, int w, int Hp, int Wp,
                       const float* mean3_host, const float* std3_host, const float* wk, const float* bias, float* out,
                       void* stream);

/* ---- 3x3/s2/p1 max pool NHWC (ResNet stem) */
int mdqe_maxpool3x3s2_nhwc_f32(const float* x, float* y, int NI, int H, int W, int C, void* stream);

/* ---- y = a + nearest_upsample(b)  (segmentation.py:47-55) */
int mdqe_upsample_nearest_add_nhwc_f32(const float* a, const float* b, float* y, int NI, int H, int W, int Hb, int Wb,
                                       int C, void* stream);

/* ---- depthwise 5x5 conv NHWC, weights [25][C]; up2 != 0 applies it to the virtual output of the depthwise
 * ConvTranspose2d(k=1,s=2,output_padding=1) (weights tw,tb [C]) of an input stored at (H/2)x(W/2)
 * (segmentation.py:28-31,59,92-98). H,W are output sizes. */
int mdqe_dwconv5x5_nhwc_f32(const float* x, const float* wt, const float* bias, float* y, int NI, int H, int W, int C,
                            int up2, const float* tw, const float* tb, void* stream);

/* The same two layers for C == 256 (one wave = the 64 float4 channel groups of a pixel; filter taps in registers):
 * mdqe_dwconv5x5_c256_f32 = the plain depthwise 5x5 on x [NI,H,W,256]; mdqe_dwconv5x5_up2_c256_f32 = ConvTranspose2d(k=1,s=2,
 * output_padding=1,groups=C) -> depthwise 5x5 in one pass, x [NI,Hs,Ws,256] -> y [NI,2Hs,2Ws,256], evaluated per 2x2
 * output quad (segmentation.py:28-29,59,92-98 of the mask-feature head); wt [25,256] tap-major. */
int mdqe_dwconv5x5_c256_f32(const float* x, const float* wt, const float* bias, float* y, int NI, int H, int W, void* stream);
int mdqe_dwconv5x5_up2_c256_f32(const float* x, const float* wt, const float* bias, const float* tw, const float* tb, float* y,
                                int NI, int Hs, int Ws, void* stream);

/* mdqe_dwconv5x5_up2_c256_f32 and the 256 -> 32 projection behind it (mdqe_gemm_nt_f32 with weight pw [32,256], bias pb [32], exact
 * fp32) as one kernel: out[pixel, 0:32] with rows ldo floats apart (ldo >= 32, ldo % 4 == 0), pixel = (img * 2Hs + Y) * 2Ws + X.  The
 * [NI,2Hs,2Ws,256] tensor between the two is never stored; the result has the bits of the two calls in sequence (the same depthwise
 * expressions, the K-step-16 kernel's summation order, bias last).  Every pointer 16-byte aligned.  128 KB of LDS per block. */
int mdqe_dwconv5x5_up2_pw_c256_f32(const float* x, const float* wt, const float* bias, const float* tw, const float* tb,
                                   const float* pw, const float* pb, float* out, long ldo, int NI, int Hs, int Ws, void* stream);

/* ---- tracker, device half (mdqe/tracking/OverTracker.py) ------------------------------------------
 * siou: out3[i,j,:] = (|A_i & B_j|, |A_i|, |B_j|) with A_i = saved[i*saved_stride + k] > 0, B_j = inp[j*inp_stride + k] > 0,
 * k < n (the overlapping frames of both are contiguous); feeds OverTracker._get_siou (:92-113).
 * accumulate: sum[r[k]*sum_stride + e] += src[c[k]*src_stride + e] (e < n), cnt[r[k]*cnt_stride + f] += 1 (f < nf);
 * r/c are HOST int arrays of any length  (OverTracker._update_memory :65-76). */
int mdqe_trk_siou_f32(const float* saved, long saved_stride, int n_saved, const float* inp, long inp_stride,
                      int n_in, long n, float* out3, void* stream);
int mdqe_trk_accumulate_f32(float* sum, long sum_stride, float* cnt, long cnt_stride, const float* src,
                            long src_stride, long n, int nf, const int* r_host, const int* c_host, int count,
                            void* stream);
/* siou_host (round 5): the same counts delivered to the HOST by the kernel itself -- one launch instead of memset + kernel +
 * device->host copy + synchronize on the tracker's per-clip critical path (the `.cpu()` of OverTracker.py:159).  acc: device scratch
 * of >= n_saved*n_in*3 floats, ZERO on entry and left zero; ticket: one device unsigned, zero on entry and left zero; out_host:
 * >= n_saved*n_in*3 64-bit words of host-coherent pinned memory (hipHostMallocCoherent).  The block that finishes last stores word k =
 * (seq << 32 | float bits of count k), seq != 0.  wait_counts: polls until every word carries seq (at most spin_us microseconds, then a
 * stream synchronize: kernel completion makes the stores visible in any case) and unpacks the counts; MDQE_ELAUNCH if they never arrive. */
int mdqe_trk_siou_host_f32(const float* saved, long saved_stride, int n_saved, const float* inp, long inp_stride,
                           int n_in, long n, float* acc, unsigned* ticket, unsigned long long* out_host,
                           unsigned seq, void* stream);
int mdqe_trk_wait_counts(const unsigned long long* out_host, int n_out, unsigned seq, int spin_us, float* counts, void* stream);

/* window flush, device half (OverTracker.get_result :195-225): window_mean: out[i,f,:] = sum[i,f0+f,:] / max(cnt[i,f0+f],1)
 * for i < n, f < nf (rows of `out` are nf frames apart).  carry: frames [src0, src0+k) of rows < n become frames [0,k) as
 * their mean logits with count 1 where seen; the rest of those rows is zeroed (`carry`: device scratch, n*k*hw floats). */
int mdqe_trk_window_mean_f32(const float* sum, const float* cnt, long hw, int mem_len, int n, int nf, long f0,
                             float* out, void* stream);
int mdqe_trk_carry_f32(float* sum, float* cnt, long hw, int mem_len, int n, int k, long src0, float* carry, void* stream);

/* ---- tracker, host half + drivers (csrc/tracker_native.hip) -----------------------------------------
 * The HOST state and decisions of OverTracker (mdqe/tracking/OverTracker.py:16-63 __init__/_init_memory, :65-90
 * _update_memory, :115-193 update, :195-225 get_result, :228-242 get_ctt_similarity) as an opaque object.  These
 * entry points are the exception to "never synchronise": mdqe_tracker_update* wait for one small device->host copy per
 * clip (the assignment needs the intersection counts), as the reference's update() does (`.cpu()` at :159).
 * All array arguments below are HOST pointers unless named bank_*, masks, counts_dev, out_masks, carry.
 *
 * mdqe_lsap_f64: scipy.optimize.linear_sum_assignment (the reference's call at OverTracker.py:159; scipy==1.8.1,
 *   requirements.txt:3) restated: cost [nr,nc] row-major -> min(nr,nc) (row, col) pairs in ascending row order.
 * create: thr = MODEL.MDQE.APPLY_CLS_THRES; E = embedding width; K = classes.
 * overlap -> (ni saved instances, bank frame s0, clip frame a, nf frames) of the frames of clip [f0, f0+n_frames) that the
 *   window already holds; decide: the update given counts3 [ni, n_in, 3] = (|A&B|, |A|, |B|) over those frames (NULL: no
 *   overlap) -> pairs (bank row r_idx[k] <- clip instance c_idx[k]) and the frame range (s0, a, nf) of the memory write;
 *   result: window class scores out_cls [n,K], n, ln (frames emitted) and, unless is_last, re-bases the host state
 *   (carry_valid [n, mem_len-win] optional).  A stand-in bank (CPU tests) drives these three.
 * update: overlap + counts (mdqe_trk_siou_host_f32 into buffers the object owns, then the flag wait; with MDQE_TRK_FAST=0 /
 *   mdqe_debug_trk_fast(0): siou kernel + D2H + sync through counts_dev / counts_host) + decide + accumulate kernel for one clip.  bank_sum [max_inst, win+T, hw],
 *   bank_cnt [max_inst, win+T]; masks [n_in, frames, hw] rows inst_stride floats apart; counts_dev / counts_host (pinned):
 *   scratch of max_inst*n_in*3 floats.  update_many: the same for a run of clips (clip i: host rows row0[i].. of
 *   scores/cls_probs/embeds, masks[i] = HOST array of device pointers).
 * get_result: result + window_mean into out_masks [n, ln, hw] + (unless is_last) carry. */
int mdqe_lsap_f64(const double* cost, int nr, int nc, int maximize, int* rows_out, int* cols_out, int* n_out);
int mdqe_tracker_create(int max_inst, int T, int win, int stride, int K, int E, float thr, void** handle);
int mdqe_tracker_destroy(void* handle);
int mdqe_tracker_state(void* handle, int* num_inst, int* num_clip, int* start_frame);
int mdqe_tracker_overlap(void* handle, int f0, int n_frames, int* ni, int* s0, int* a, int* nf);
int mdqe_tracker_decide(void* handle, int f0, int n_frames, int n_in, const float* scores, const float* cls_probs,
                        const float* embeds, const float* counts3, int* r_idx, int* c_idx, int* n_pairs,
                        int* s0, int* a, int* nf);
int mdqe_tracker_result(void* handle, int is_last, float* out_cls, int* n, int* ln, unsigned char* carry_valid);
int mdqe_tracker_update(void* handle, float* bank_sum, float* bank_cnt, long hw, int f0, int n_frames, int n_in,
                        const float* scores, const float* cls_probs, const float* embeds, const float* masks,
                        long inst_stride, float* counts_dev, float* counts_host, void* stream);
int mdqe_tracker_update_many(void* handle, float* bank_sum, float* bank_cnt, long hw, int n_clips, const int* f0,
                             const int* n_frames, const int* n_in, const int* row0, const float* scores,
                             const float* cls_probs, const float* embeds, const float* const* masks,
                             const long* inst_stride, float* counts_dev, float* counts_host, void* stream);
int mdqe_tracker_get_result(void* handle, int is_last, float* bank_sum, float* bank_cnt, long hw, float* out_masks,
                            float* carry, float* out_cls, int* n, int* ln, void* stream);

/* ---- per-clip stages as batch kernels (csrc/clip_ops.hip) --------------------------------------------
 * clip_assoc: inter-frame query association (transformer_dec.py:111-145): emb [frames, Q, E] (E in {16,32,64}), fidx [Bc, T]
 *   (device int32: cache frame of (clip, t)) -> idx [Bc, T, Q] = arg-max_q of e[f(b,t),q].e[f(b,ct),k] over the cells within
 *   +-wdw*|t-ct| of k's (Q = nb*nb grid cells).
 * clip_gather_init (:142-143,462,470-471): x [Bc*T*Q, C] = content[f(b,t), idx], ref [Bc*T*Q, 4] = (coords[..], 0.1, 0.1),
 *   xinst [Bc*Q, C] = x[b, ct]; idx NULL = identity.
 * box_refine (:473-480,492-503; util/misc.py:478-482; util/box_ops.py:8-19): boxes = sigmoid(delta + inverse_sigmoid(prev))
 *   [Bc*T*Q, 4]; ibox [Bc*Q, 4] = cxcywh of (min clamped top-left, max clamped bottom-right) over frames [t0, t1).
 * add_rows: out = a + b on row-strided operands.  time_fuse (:374-376): out[b,q,:] = sum_t softmax_t(w[b,t,q]) x[b,t,q,:]
 *   (+ pos into out_plus_pos when given). */
int mdqe_clip_assoc_f32(const float* emb, int Q, int E, const int* fidx, int Bc, int T, int ct, float wdw, int nb,
                        int* idx_out, void* stream);
int mdqe_clip_gather_init_f32(const float* content, const float* coords, const int* fidx, const int* idx, int Bc, int T,
                              int Q, int C, int ct, float* x, float* ref, float* xinst, void* stream);
int mdqe_box_refine_f32(const float* delta, const float* prev, int Bc, int T, int Q, int t0, int t1, float* boxes,
                        float* ibox, void* stream);
int mdqe_add_rows_f32(const float* a, long lda, const float* b, long ldb, float* out, long ldo, long rows, int C, void* stream);
int mdqe_time_fuse_f32(const float* w, const float* x, int Bc, int T, int Q, int C, float* out, const float* pos,
                       float* out_plus_pos, void* stream);
/* Round 3, fewer launches between the decoder's GEMMs.  box_head_refine: bbox_embed's last Linear(C -> 4) + the refinement
 * sigmoid(delta + inverse_sigmoid(prev)) + the clip-circumscribed box (transformer_dec.py:473-480,492-503) in one kernel; h [Bc*T*Q, K]
 * is the head's second hidden activation, W [4, K], bias [4].  time_fuse_dot: time_weights Linear(C -> 1) of the frame queries xw, the
 * softmax over the clip's frames and the weighted sum of src (:374-376) in one kernel.  Same arithmetic as the kernels they replace. */
int mdqe_box_head_refine_f32(const float* h, long ldh, const float* W, const float* bias, const float* prev, int Bc, int T, int Q, int K,
                             int t0, int t1, float* boxes, float* ibox, void* stream);
int mdqe_time_fuse_dot_f32(const float* xw, const float* wt, const float* bt, const float* src, int Bc, int T, int Q, int C, float* out,
                           void* stream);

/* inference_clip (mdqe/mdqe.py:368-428) for a batch of B clips.
 * clip_select (:373-379): cls [B,Q,K], emb [B,Q,C] -> kept [B,Q] (query indices of the kept ranks, score order), n_keep [B]:
 *   sort by best class score, keep >= min(thr, best), drop rank q if max_{p<q} cos(e_p, e_q) >= 0.99, cap at max_keep.
 *   Workspaces: order [B,Q] int, n_thr [B] int, inv_norm [B,Q], sim [B,Q,Q].
 * dyn_mask_nms: the fused dynamic-mask kernel + NMS.  HOST int arrays row0 / n / f0 [B] (first instance row, kept count,
 *   first cache frame of the clip).  coef [B,Q,M], feats [frames,H,W,M] channels-last ->
 *   logits [n_rows,T,H,W] = einsum 'qm,mthw->qthw' (:384); stats [n_rows,5] = (any(x>0), sum sigmoid(x)[hard], count(hard),
 *   sum_half sigmoid(x), count_half(hard)), hard = sigmoid(x) > 0.5, half = F.interpolate(scale_factor=0.5) grid of :394-396
 *   (every 2nd frame when T >= 5); mi [n_rows] = max_{p<q} soft-IoU (:398-405): `soft @ hard.t()` as one batched MFMA launch.
 *   Scratch: soft_h / hard_h [n_rows, Ph] (Ph = ceil(T/t_step)*(H/2)*(W/2)), part [mdqe_dyn_mask_workspace_floats()],
 *   gram [mdqe_nms_workspace_floats(max kept per clip)].
 * clip_finalize (:408-419): out [n_rows, 2+K+C] = (score, label, class scores, embedding) of the j-th selected row of clip b at
 *   row row0[b]+j, sel [n_rows] its instance row, n_sel [B].
 * rows_gather: out[i,:] = src[idx[i],:]. */
int mdqe_clip_select_f32(const float* cls, const float* emb, int B, int Q, int K, int C, float thr, int max_keep,
                         int* order_ws, int* n_thr_ws, float* inv_norm_ws, float* sim_ws, int* kept, int* n_keep, void* stream);
long mdqe_dyn_mask_workspace_floats(int n_rows, int T, int H, int W);
int mdqe_dyn_mask_nms_f32(const float* coef, const int* kept, const float* feats, int B, int Q, int M, int T, int H, int W,
                          const int* row0_host, const int* n_host, const int* f0_host, float* logits, float* soft_h,
                          float* hard_h, float* part, float* gram, float* stats, float* mi, void* stream);
long mdqe_nms_workspace_floats(int n_max);
int mdqe_clip_finalize_f32(const float* cls, const float* emb, const int* kept, const float* stats, const float* mi, int B,
                           int Q, int K, int C, float thr, const int* row0_host, const int* n_host, int* sel, int* n_sel,
                           float* out, void* stream);
int mdqe_rows_gather_f32(const float* src, const int* idx_dev, int n, long len, float* out, void* stream);

/* ---- per-row statistics of dynamic mask logits (mdqe/mdqe.py:387-413) in one pass -------------------
 * logits [n, T, H, W].  stats[r] = (any(x>0), sum sigmoid(x)[x>0], count[x>0], sum_half sigmoid(x), count_half[x>0]);
 * half = every 2nd pixel in y and x (and every 2nd frame when t_step == 2), i.e. F.interpolate(scale_factor=0.5,
 * nearest) of :394-396; soft_h / hard_h [n, Th*(H/2)*(W/2)] receive sigmoid(x) and [x>0] on that grid. */
int mdqe_mask_row_stats_f32(const float* logits, int n, int T, int H, int W, int t_step, float* stats5,
                            float* soft_h, float* hard_h, void* stream);

/* ---- nn.MultiheadAttention core for short sequences (transformer_dec.py:348-353,397-402) --------------
 * o[b,q,h,:] = softmax_k((q*D^-0.5).k) @ v ; qk rows hold q at col h*D and k at col C+h*D.  Q <= 256, D in {8,16,24,32}. */
int mdqe_mha_small_f32(const float* qk, long ldqk, const float* v, long ldv, float* o, long ldo, int B, int Q,
                       int C, int nh, void* stream);

/* ---- grid-guided query selection (transformer_dec.py:81-109): conf [NI,H,W,K] -> coords [NI,nb*nb,2] (x,y);
 * score_ws: NI*H*W floats. */
int mdqe_query_select_f32(const float* conf, int NI, int H, int W, int K, int nb, float* score_ws, float* coords,
                          void* stream);

/* ---- query content (transformer_dec.py:171-179): mean over levels of border-mode bilinear grid_sample of the
 * channels-last tokens [NI,N,C] at coords [NI,Qn,2]; level tables are HOST int[n_levels]. */
int mdqe_sample_levels_mean_f32(const float* tokens, int NI, long N, int C, const float* coords, int Qn,
                                const int* lvH_host, const int* lvW_host, const int* lvStart_host, int n_levels,
                                float* out, void* stream);

/* ---- final masks (mdqe/mdqe.py:357-358,458-462; util/misc.py:485-507) fused: x`factor` aligned-bilinear ->
 * sigmoid -> crop [:h,:w] -> nearest resize to (Ho,Wo) -> > 0.5.  logits [*,Fw,Hm,Wm] (one tracker window);
 * row k of out (uint8 [n_sel][out_inst_stride]) takes instance inst_idx_dev[k], frames written at f_off..  Any base address and
 * stride (dword stores only where an address is 4-byte aligned).  MDQE_FINAL_MASK_FLAT=1 in the environment selects the flat
 * one-byte-per-thread kernel instead of the band-mapped one: the same bytes (it also serves Ho * Wo >= 2^31). */
int mdqe_final_masks_u8(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                        int h, int w, int Ho, int Wo, unsigned char* out, long out_inst_stride, int f_off,
                        void* stream);

/* Same masks, straight to COCO run-length form (the result writer's mask_util.encode, mdqe/data/ytvis_eval.py:307-312 ->
 * cocoapi rleEncode): pos[(k*Fw+f)*cap + i] = i-th column-major pixel index at which mask (k,f) changes value (the value
 * before the first pixel is 0), n_pos[k*Fw+f] = number of changes (may exceed cap: only the first cap are stored).
 * Run lengths are the differences of consecutive positions; the dense mask is never written. */
int mdqe_final_masks_rle(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                         int h, int w, int Ho, int Wo, int cap, int* pos, int* n_pos, void* stream);

/* The same two sweeps with the geometry of every final mask gathered on the way -- what a consumer otherwise gets from the masks on
 * the host (pycocotools area / toBbox, mdqe/data/pycocotools/mask.py:93-101; BitMasks.get_bounding_boxes, mdqe/mdqe.py:554; the
 * visualiser's per-frame pass, demo/clip/visualizer_from_json.py:94-103; the `bboxes` / `areas` the YTVIS loader requires per frame,
 * mdqe/data/datasets/ytvis.py:280-290).  geom int32 [n_sel*Fw, 5]: row k*Fw+f = (area, xmin, ymin, xmax, ymax) of the set pixels of
 * (selected row k, window frame f) in output pixels, inclusive; an empty mask has area 0 and xmin = Wo > xmax = -1, ymin = Ho > ymax
 * = -1 (as mdqe_image_mask_stats_f32).  out / pos / n_pos exactly as the entry points above write them (one definition of the bit);
 * geom is fully overwritten on every call (no pre-initialisation), integers, identical from run to run; (long)Ho*Wo < 2^31. */
int mdqe_final_masks_u8_geom(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                             int h, int w, int Ho, int Wo, unsigned char* out, long out_inst_stride, int f_off,
                             int* geom, void* stream);
int mdqe_final_masks_rle_geom(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                              int h, int w, int Ho, int Wo, int cap, int* pos, int* n_pos, int* geom, void* stream);

/* The other form of a window's final masks: ONE plane per frame that says which track owns each pixel (the form of DAVIS / VIPSeg
 * PNGs, what a viewer paints from in a single pass).  With v_k the up-sampled logit of map inst_idx_dev[k] at the pixel and b_k its
 * final-mask bit (the same expressions as the entry points above: one definition of both), out[f_off + f, Y, X] = 0 if no b_k is set,
 * else inst_idx_dev[k*] + 1 for the smallest k* among the rows with b_k set and v_k equal to the largest v among them.  So out != 0
 * exactly on the union of the dense masks, and a label names a track whose dense mask holds the pixel.  out uint8 [>= f_off + Fw, Ho,
 * Wo]; n_sel <= 255 and every inst_idx_dev[k] < 255 (the caller's part: the indices live on the device).  geom: NULL, or int32
 * [n_sel*Fw, 5] with the geometry of each label's VISIBLE region, row k*Fw+f, layout and empty convention of mdqe_final_masks_u8_geom;
 * fully overwritten on every call, integers, identical from run to run.  Unlike the mask entry points, n_sel == 0 with Fw > 0 writes
 * zeros to the Fw frames (a window without tracks is all background).  Never allocates, never synchronises. */
int mdqe_final_label_map_u8(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                            int h, int w, int Ho, int Wo, unsigned char* out, int f_off, int* geom, void* stream);

/* The soft form of the same sweep: ONE plane per frame that holds a WEIGHT, the matte that compositing takes, instead of a name.
 * logits .. Wo are the label map's.  Row k takes part iff take == NULL or take[inst_idx_dev[k] + 1] != 0: take is uint8 [256] on the
 * device, indexed by the row's label as in the label map (entry 0 is unused; the kernel masks the index to 0..255, so an index the
 * caller should not have passed -- inst_idx_dev[k] >= 255 -- reads entry (index & 255) and never memory outside the table).  Per output pixel, with v_k the up-sampled logit and b_k
 * the final-mask bit of row k (the expressions of the entry points above: one definition of both), over the participating rows:
 *   vmax = the largest v_k;   U = the OR of the b_k;
 *   x = gain * vmax (fp32);   p = 1 / (1 + expf(-x));   a = (int)rintf(255 * p);
 *   out[f_off + f, Y, X] = U ? max(a, 128) : min(a, 127);   no participating row: 0.
 * So out >= 128 exactly on the union of the participating rows' dense masks, bit for bit, whatever gain is and whatever the last ulp
 * of expf is; away from that edge the plane is the rounded sigmoid, to the last ulp of expf.  out uint8 [>= f_off + Fw, Ho, Wo].
 * MDQE_EINVAL, before any pointer is looked at: the label map's checks (n_sel <= 255, (long)Ho*Wo < 2^31, Hm*Wm < 2^31, f_off >= 0)
 * and a gain that is not finite or outside (0, 64].  Fw == 0 returns OK and launches nothing; n_sel == 0 with Fw > 0 writes zeros.
 * Any Wo and any f_off (4 bytes per store where the address allows, single bytes otherwise).  One launch, no atomics: identical from
 * run to run.  Never allocates, never synchronises. */
int mdqe_final_matte_u8(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                        int h, int w, int Ho, int Wo, const unsigned char* take, float gain, unsigned char* out, int f_off,
                        void* stream);

/* A window's final masks scored against ground truth without leaving the device: the integers behind the video IoU of the YTVIS
 * evaluator (mdqe/data/pycocotools/ytvoseval.py:173-219).  logits, n_sel, inst_idx_dev, Fw, Hm, Wm, factor, h, w, Ho, Wo are exactly
 * mdqe_final_masks_u8's, and b_k(f, Y, X), the bit of selected row k at window frame f and output pixel (Y, X), is that entry point's
 * bit (the same device expression: one definition).  gt_bits: uint32 [>= f_off + Fw, Ho, Wo]; bit g (0 <= g < G <= 32) of the word at
 * (f_off + f, Y, X) says that ground-truth track g holds the pixel.  Ground-truth tracks may overlap; bit 31 is an ordinary bit.
 *   inter[k * inter_row_stride + g]  is INCREASED by the number of (f, Y, X), 0 <= f < Fw, with b_k set and bit g set.  The caller
 *                                    zeroes it once per video; consecutive windows add up; 64-bit, since a long 640p video passes
 *                                    2^31 pixels.  Columns g >= G of a row are not touched.
 *   area[k * Fw + f]                 is OVERWRITTEN with the number of (Y, X) with b_k set: column 0 of mdqe_final_masks_u8_geom's
 *                                    table (int32 [n_sel * Fw]).
 * Integer counters only (ballots, popcounts, integer LDS and global atomics): exact, identical from run to run.  (long)Ho*Wo < 2^31,
 * Hm*Wm < 2^31, n_sel*Fw < 2^31, 1 <= G <= 32, inter_row_stride >= G and f_off >= 0 are checked before any pointer is looked at
 * (MDQE_EINVAL); n_sel == 0 or Fw == 0 returns OK and launches nothing (inter and area stay as they are).  Any n_sel (rows go in
 * chunks of 256 per block; at most 34 KB of LDS).  Never allocates, never synchronises. */
int mdqe_final_masks_overlap(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                             int h, int w, int Ho, int Wo,
                             const uint32_t* gt_bits, int G, int f_off,
                             unsigned long long* inter, long inter_row_stride, int* area, void* stream);

/* The same sweep with the masks counted against EACH OTHER: how much of each track is hidden, and by whom -- the relation between the
 * tracks of a window, which neither the planes nor the label map says on its own.  logits .. Wo are the label map's.  At window frame f
 * and output pixel (Y, X), with b_k the final-mask bit of selected row k (the expression of the entry points above: one definition) and
 *   o = the owner: the smallest k among the rows with b_k set whose up-sampled logit equals the largest among them, none if no bit is
 *       set -- exactly the choice mdqe_final_label_map_u8 makes (the same device expression), so inst_idx_dev[o] + 1 is its label,
 *   occ[(k * Fw + f) * n_sel + j] = #{(Y, X) : b_k set and o == j}                  int32 [n_sel, Fw, n_sel].
 * So occ[k, f, k] is the area of k's VISIBLE region (column 0 of the label map's geometry table), the sum of occ[k, f, :] the area of
 * k's dense mask (column 0 of mdqe_final_masks_u8_geom's table), and for j != k occ[k, f, j] is the part of k's mask that track j
 * hides.  A row listed twice in inst_idx_dev follows from the rule: the earlier position owns.  Only selected rows can be owners.
 * occ is fully OVERWRITTEN on every call (the entry clears it itself).  Integer counters only (ballots, popcounts, integer LDS and
 * global atomics): exact, identical from run to run.  n_sel <= 255, (long)Ho*Wo < 2^31, Hm*Wm < 2^31 and (long)n_sel*n_sel*Fw < 2^31
 * are checked before any pointer is looked at (MDQE_EINVAL); n_sel == 0 or Fw == 0 returns OK and launches nothing.  Any n_sel <= 255:
 * the k axis goes in chunks of at most 16384 / n_sel - 1 rows per block (one chunk up to 127 rows, five at 255; at most 64 KB of LDS),
 * every chunk finding the owner over all rows.  Never allocates, never synchronises. */
int mdqe_final_masks_occlusion(const float* logits, int n_sel, const int* inst_idx_dev, int Fw, int Hm, int Wm, int factor,
                               int h, int w, int Ho, int Wo, int* occ, void* stream);
/* That entry's launch plan for 1 <= n_sel <= 255 (else MDQE_EINVAL), on the host, nothing launched: *chunk rows of the k axis a block,
 * *chunks of them (blockIdx.y), *lds_bytes of dynamic LDS a block asks for (ids[n_sel] | tab[chunk, n_sel]) and, where slots is not NULL
 * (int [*chunks * n_sel], at most 5 * 255), slots[b * n_sel + k] = the row of block-chunk b's table that selected row k counts into, or
 * -1 for a row of another chunk -- the kernel's own mapping (one definition), so every row >= 0 there lies below that chunk's rows. */
int mdqe_final_masks_occlusion_plan(int n_sel, int* chunk, int* chunks, long* lds_bytes, int* slots);

/* The picture a viewer paints from that map: out[f_off + f, Y, X, c] (uint8, pixel-interleaved, [>= f_off + F, Ho, Wo, 3]) from labels
 * (uint8 [F, Ho, Wo], what mdqe_final_label_map_u8 writes), the frames the caller handed in (frames: [F, 3, h0, w0] planar, uint8 if
 * is_u8 else float32, consecutive frames frame_stride ELEMENTS apart -- a view into a larger store works -- or NULL) and palette (uint8
 * [256, 3], in the frames' channel order: channel c of out is channel c of frames).  Integers only, ONE definition:
 *   source pixel  sy = (Y*h0) / Ho, sx = (X*w0) / Wo (exact integer division: nearest sampling, the identity at equal sizes);
 *   source value  s_c = frames[f, c, sy, sx]; float32 becomes min(max(rint(v), 0), 255), rint rounding half to even, NaN -> 0; no
 *                 frames: s_c = 0 (paints onto black: a DAVIS-style colour map);
 *   label         l = labels[f, Y, X];  l == 0 (background): out_c = s_c;
 *   contour       else edge = for some d in 1..contour and some direction (+-d, 0), (0, +-d) the neighbour lies INSIDE the image and
 *                 its label differs from l (a neighbour outside never counts: an object cut by the border gets no line along it;
 *                 contour = 0: no contours);
 *   colour        out_c = palette[l][c] if edge, else (s_c*(256 - a256) + palette[l][c]*a256 + 128) >> 8.
 * a256 in 0..256, contour in 0..3, Ho*Wo*3 < 2^31 and F*Ho*Wo < 2^31, all checked before any pointer is looked at; F == 0 returns OK
 * and launches nothing.  Nothing needs to be aligned (Wo, Ho*Wo*3, f_off*Ho*Wo*3 arbitrary).  No atomics: identical from run to run.
 * Never allocates, never synchronises. */
int mdqe_render_overlay_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                           const unsigned char* labels, int F, int Ho, int Wo,
                           const unsigned char* palette, int a256, int contour,
                           unsigned char* out, int f_off, void* stream);

/* The same map painted straight onto decoder surfaces, in the YUV domain, for an encoder (csrc/render_yuv.hip): semi-planar YUV 4:2:0
 * in, painted surfaces of the SAME format out.  y, y_pitch, y_stride, uv, uv_pitch, uv_stride, H, W, fmt (0 NV12, 1 P010) are exactly
 * mdqe_yuv420sp_to_rgb_u8's: pitches and strides in BYTES, a P010 sample's value is word >> 6.  F surfaces; labels: uint8 [F, H, W],
 * contiguous, at the surfaces' own size (nothing is resampled here); palette_yuv: uint16 [256, 3], rows (Y, U, V) in sample units, 0..255
 * for NV12 and 0..1023 for P010 (only those 8 / 10 bits of an entry are used).  The output planes have the input planes' layout with
 * their own pitches and strides; surface f is written at out_y + (f_off + f) * out_y_stride and out_uv + (f_off + f) * out_uv_stride.
 * Integers only, ONE definition (>> acts on non-negative values only):
 *   label     l = labels[f][r][c];
 *   contour   edge = for some d in 1..contour and some direction (+-d, 0), (0, +-d) the neighbour lies INSIDE the picture and its
 *             label differs from l: mdqe_render_overlay_u8's definition (contour = 0: no contours);
 *   blend     blend(s, p) = (s * (256 - a256) + p * a256 + 128) >> 8;
 *   pixel     px(s, p) = s if l == 0, else p if edge, else blend(s, p);
 *   luma      Yout[r][c] = px(Y[r][c], palette_yuv[l][0]);
 *   chroma    one (U, V) pair serves the in-picture pixels i of its 2 x 2 block, n = 1, 2 or 4 of them (odd right / bottom edges).  With
 *             C the pair's U (k = 1) or V (k = 2) and l_i, edge_i the pixels' own labels and edges:
 *               Cout = (sum_i px_i(C, palette_yuv[l_i][k]) + n / 2) >> log2(n),
 *             so a block whose pixels all have label 0 keeps C;
 *   P010      a word the rule leaves unchanged -- luma with l == 0, a chroma pair with every label of its block 0 -- is copied with all
 *             16 of its bits; every other word is written as value << 6.
 * A background pixel therefore keeps the decoder's bits exactly.  Writes cover W luma samples and 2 * ceil(W/2) chroma samples per row,
 * H and ceil(H/2) rows per surface: output padding is never written, input padding never read.
 * In and out: an output plane may BE its input plane -- the same address (after f_off), pitch and stride: painting in place; luma and
 * chroma independently -- since every sample is read and written by the one thread that owns it.  Any other overlap is refused
 * (MDQE_EINVAL): a surface of an output plane (its first to its last byte written, the rows' padding between them included) must not
 * meet a surface of an input plane, of the other output plane, the labels or the palette.  Planes may interleave as a decoder's
 * allocation does (luma 0, chroma 0, luma 1, ...).  Two surfaces of an output plane must not share bytes (F > 1: out strides >= the
 * bytes a surface spans).
 * MDQE_EINVAL, before any pointer is looked at, for a256 outside 0..256, contour outside 0..3, H or W <= 0, F < 0, f_off < 0, fmt outside
 * {0, 1}, an input or output pitch smaller than a row (W samples of luma, 2 * ceil(W/2) of chroma), a negative stride, odd P010 pitches
 * or strides, and F * H * W >= 2^31 - 1; F == 0 returns OK and launches nothing; odd P010 plane pointers and an odd palette pointer are
 * MDQE_EINVAL.  Nothing else needs to be aligned: where every plane pointer (in, out, labels), pitch, stride and W are multiples of 4
 * bytes the launch moves 4 bytes per access (16 where they are multiples of 16 and contour == 0), otherwise single samples.  One
 * launch, no atomics: identical from run to run.  Never allocates, never synchronises. */
int mdqe_render_overlay_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                 int F, int H, int W, int fmt /*0 nv12, 1 p010*/, const unsigned char* labels,
                                 const unsigned short* palette_yuv, int a256, int contour,
                                 void* out_y, long out_y_pitch, long out_y_stride,
                                 void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream);

/* The mosaic overlay (csrc/render_mosaic.hip): the two painters above with a PER-LABEL action, one of them a redaction mosaic.  Every
 * argument the two entries share with mdqe_render_overlay_u8 / mdqe_render_overlay_yuv420sp means what it means there; new are
 *   action  uint8 [256], device: action[l] is what happens to a pixel of label l -- 0 keep, 1 tint, 2 mosaic (any other value: undefined);
 *           action[0] is the background's;
 *   cell    the side of a mosaic cell in pixels, even, 2..64.
 * Integers only, ONE definition:
 *   edge    exactly mdqe_render_overlay_u8's definition on the LABELS, whatever the actions are;
 *   cells   cell x cell squares of the output grid anchored at (0, 0): pixel (Y, X) lies in cell (Y / cell, X / cell); the cells at the
 *           right and at the bottom are smaller.  mean_c(cell) = (sum s_c + n / 2) / n, integer division, the sum over ALL n in-picture
 *           pixels of the cell whatever their labels (64 * 64 * 1023 < 2^31).  A mosaic pixel therefore carries nothing finer than its
 *           cell, and a thin mask does not change what the cell shows;
 *   RGB     s_c is mdqe_render_overlay_u8's source value (nearest-sampled, float32 by the rint / clamp / NaN rule, no frames: 0).  With l the
 *           pixel's label:  action 0: out_c = s_c;
 *                           action 1: out_c = palette[l][c] if edge, else (s_c*(256 - a256) + palette[l][c]*a256 + 128) >> 8;
 *                           action 2: out_c = mean_c(cell of (Y, X));
 *   YUV     (values: word >> 6 for P010.)  Luma follows the RGB rule with luma cells of cell x cell.  A chroma cell is the (cell/2) x (cell/2)
 *           pairs under the same picture area -- chroma position (r, c) lies in cell (r / (cell/2), c / (cell/2)) -- and meanU, meanV are
 *           taken over its in-picture pairs of the ceil(H/2) x ceil(W/2) chroma plane.  The chroma rule of mdqe_render_overlay_yuv420sp
 *           stays: Cout = (sum_i px_i + n / 2) >> log2(n) over the n in-picture pixels i of the pair's 2 x 2 block, where px_i is C for
 *           action 0, the palette or blend value for action 1 and the cell's meanC for action 2 (cell is even: a block never straddles
 *           cells);
 *   P010    a luma word whose label has action 0 is copied with all 16 bits, and so is a chroma pair whose block's labels all have
 *           action 0; every other word is written as value << 6.
 * With action = {0, 1, 1, ..., 1} both entries are, by this definition, bit-identical to the two entries above.
 * MDQE_EINVAL for a cell that is odd or outside 2..64; every other check is that of the entry above, made before any pointer is looked
 * at; F == 0 returns OK and launches nothing.  mdqe_render_mosaic_yuv420sp does NOT paint in place: a cell's mean reads samples that
 * other threads write, so an output plane that meets an input plane in any way (or the other output plane, the labels, the palette,
 * the action table) is MDQE_EINVAL.  Alignment: RGB as above (nothing needs to be aligned); surfaces move 4 bytes per access where every
 * plane pointer (in, out, labels), pitch, stride and W are multiples of 4 bytes, otherwise single samples.  Only cells that hold a
 * pixel of action 2 are reduced.  One launch, no atomics on global memory: identical from run to run.  Never allocates, never
 * synchronises. */
int mdqe_render_mosaic_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                          const unsigned char* labels, int F, int Ho, int Wo,
                          const unsigned char* palette, const unsigned char* action, int a256, int contour, int cell,
                          unsigned char* out, int f_off, void* stream);
int mdqe_render_mosaic_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                int F, int H, int W, int fmt /*0 nv12, 1 p010*/, const unsigned char* labels,
                                const unsigned short* palette_yuv, const unsigned char* action, int a256, int contour, int cell,
                                void* out_y, long out_y_pitch, long out_y_stride,
                                void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream);

/* The blur overlay (csrc/render_blur.hip): the same two painters with a PER-LABEL action, one of them a Gaussian redaction blur.  Every
 * argument the two entries share with mdqe_render_mosaic_u8 / mdqe_render_mosaic_yuv420sp means what it means there; `cell` is replaced by
 *   taps     uint16 [radius + 1], device, radius in 0..32: the weight of a sample d away is taps[|d|], in units of 1/4096, and
 *            taps[0] + 2 * sum(taps[1..radius]) == 4096 (the caller's duty; render.blur_taps makes such tables).  The table is an input of
 *            the rule, as the palette is.  radius = 0 with taps = {4096}: the blur is the identity;
 *   taps_c   (surfaces) a second such table of radius_c in 0..16, for the chroma plane;
 *   action   uint8 [256], device: 0 keep, 1 tint, 3 blur; ANY other value acts as 0.  action[0] is the background's.
 * Integers only, ONE definition:
 *   edge     exactly mdqe_render_overlay_u8's definition on the LABELS, whatever the actions are;
 *   source   s_c(Y, X) is exactly mdqe_render_overlay_u8's source value: nearest-sampled onto the OUTPUT grid, float32 by the rint / clamp
 *            / NaN rule, no frames: 0.  The blur acts on the output grid, as the mosaic's cells do;
 *   blur     clamped coordinates replicate the picture's border: X' = min(max(X + d, 0), Wo - 1), Y' likewise.
 *              h_c(Y, X)    = (sum_{d = -R..R} taps[|d|] * s_c(Y, X') + 128) >> 8         (at most 16368: 14 bits)
 *              blur_c(Y, X) = (sum_{d = -R..R} taps[|d|] * h_c(Y', X) + 32768) >> 16      (the sum stays below 2^26)
 *            A constant picture is therefore unchanged.  The taps take in ALL pixels under the kernel whatever their labels: a sharp
 *            (kept or tinted) object next to a blurred background bleeds into it, and a blurred object takes in its surroundings --
 *            the behaviour of a plain Gaussian blur.  The blur that stops at region borders is mdqe_render_blur_within_u8 below;
 *   RGB      with l the pixel's label:  action 1: out_c = palette[l][c] if edge, else (s_c*(256 - a256) + palette[l][c]*a256 + 128) >> 8;
 *                                       action 3: out_c = blur_c(Y, X);
 *                                       else:     out_c = s_c;
 *   YUV      (values: word >> 6 for P010.)  Luma follows the RGB rule on the luma plane with `taps`.  Chroma is blurred on its own
 *            ceil(H/2) x ceil(W/2) grid of pairs, U and V separately, with taps_c and coordinates clamped to that plane.  The chroma rule
 *            of mdqe_render_overlay_yuv420sp stays: Cout = (sum_i px_i + n / 2) >> log2(n) over the n in-picture pixels i of the pair's
 *            2 x 2 block, where px_i is C for a kept pixel, the palette or blend value for action 1 and the pair's blurred C for action 3;
 *   P010     a luma word whose pixel is kept is copied with all 16 bits, and so is a chroma pair whose block's pixels are all kept; every
 *            other word is written as value << 6.
 * With action = {0, 1, 1, ..., 1} both entries are, by this definition, bit-identical to the plain painters.
 * MDQE_EINVAL for a radius outside 0..32 or a radius_c outside 0..16; every other check is that of the mosaic entries, made before any
 * pointer is looked at; F == 0 returns OK and launches nothing; a null or odd tap table is refused as the palette is.
 * mdqe_render_blur_yuv420sp does NOT paint in place: the taps read samples that other threads write, so an output plane that meets an
 * input plane in any way (or the other output plane, the labels, the palette, the action table, either tap table) is MDQE_EINVAL.
 * Nothing needs to be aligned.  Only tiles (16 x 64 pixels) that hold a pixel of action 3 are filtered.  One launch, no global scratch,
 * no atomics: identical from run to run.  Never allocates, never synchronises. */
int mdqe_render_blur_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                        const unsigned char* labels, int F, int Ho, int Wo,
                        const unsigned char* palette, const unsigned char* action, int a256, int contour,
                        const unsigned short* taps, int radius, unsigned char* out, int f_off, void* stream);
int mdqe_render_blur_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                              int F, int H, int W, int fmt /*0 nv12, 1 p010*/, const unsigned char* labels,
                              const unsigned short* palette_yuv, const unsigned char* action, int a256, int contour,
                              const unsigned short* taps, int radius, const unsigned short* taps_c, int radius_c,
                              void* out_y, long out_y_pitch, long out_y_stride,
                              void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream);

/* The edge-stopping blur overlay (csrc/render_blur_within.hip): the two blur painters above with a blur that stays INSIDE the blurred
 * region -- a normalised, membership-weighted Gaussian, the usual cure for the halo a sharp object smears into a blurred background.
 * The argument lists are those of mdqe_render_blur_u8 and mdqe_render_blur_yuv420sp, argument by argument.  Everything that is not the
 * blurred value is the plain entries' rule above: edge, source, the actions (0 keep, 1 tint, 3 blur, any other value as 0), the tints,
 * the chroma block mean, P010's kept words, every check and refusal (in place included), F == 0, nothing needs to be aligned, and only
 * tiles (16 x 64 pixels) that hold a pixel of action 3 are filtered.  The blurred value, integers only, ONE definition:
 *   member   m(Y, X) = 1 where action[labels[f, Y, X]] == 3, else 0;
 *   clamp    coordinates are clamped as in the plain rule, X' = min(max(X + d, 0), Wo - 1), Y' likewise: a border pixel is replicated
 *            TOGETHER WITH its membership;
 *   per channel c, with NO rounding between the passes:
 *              Hn_c(Y, X) = sum_{d = -R..R} taps[|d|] * m(Y, X') * s_c(Y, X')        Hw(Y, X) = sum_{d = -R..R} taps[|d|] * m(Y, X')
 *              N_c(Y, X)  = sum_{d = -R..R} taps[|d|] * Hn_c(Y', X)                   D(Y, X)  = sum_{d = -R..R} taps[|d|] * Hw(Y', X)
 *              within_c(Y, X) = (N_c + D // 2) // D                                   (// is the floor division; everything is >= 0)
 *            The value is defined only for pixels of action 3; there D >= taps[0]^2 > 0, because the pixel itself counts.  Elsewhere D
 *            may be 0 and nothing is computed;
 *   bounds   Hw <= 4096; Hn <= 4096 * 255 < 2^20 for 8-bit values and <= 4096 * 1023 < 2^22 for P010 values; D <= 2^24; for 8-bit values
 *            N + D // 2 <= 2^24 * 255 + 2^23 = 4 286 578 688 < 2^32, so 32 bits hold it; N of 10-bit values needs more than 32 bits (the
 *            kernel sums P010 in 64);
 *   RGB      action 3: out_c = within_c(Y, X); every other action as mdqe_render_blur_u8;
 *   YUV      (values: word >> 6 for P010.)  Luma follows the rule above on the luma plane with `taps`.  Chroma is filtered on its own
 *            ceil(H/2) x ceil(W/2) grid of pairs, U and V separately, with taps_c and coordinates clamped to that plane.  A pair is a
 *            member when ANY in-picture pixel of its 2 x 2 block has action 3: the pair of every blurred pixel is a member, so D > 0
 *            wherever the value is used.  The blurred pixel then enters its pair's block mean with the pair's within value, as it does
 *            with the pair's blurred C in the plain rule.
 * What follows from it:
 *   - a region whose members under the kernel all have the value v keeps v exactly (N = v * D), whatever lies outside it;
 *   - the value at a pixel of action 3 does not depend on the source value of ANY pixel whose action is not 3 (a kept or tinted object
 *     does not bleed into a blurred background, a blurred track takes in nothing of its surroundings);
 *   - where every pixel is a member D = 2^24, and the value differs from the plain rule's blur_c by at most 1: the plain rule's row
 *     rounding moves the exact mean by at most 1/32 before the final rounding;
 *   - with action = {0, 1, 1, ..., 1} both entries are bit-identical to the plain painters, and with radius = 0, taps = {4096} a pixel of
 *     action 3 keeps its source value.
 * The division is exact.  One launch, no global scratch, no atomics: identical from run to run.  Never allocates, never synchronises.
 * An RGB launch with a radius above 24 takes 68 KB of LDS, more than the 64 KB a kernel gets unasked; MDQE_ELAUNCH where the device does
 * not grant it. */
int mdqe_render_blur_within_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                               const unsigned char* labels, int F, int Ho, int Wo,
                               const unsigned char* palette, const unsigned char* action, int a256, int contour,
                               const unsigned short* taps, int radius, unsigned char* out, int f_off, void* stream);
int mdqe_render_blur_within_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                     int F, int H, int W, int fmt /*0 nv12, 1 p010*/, const unsigned char* labels,
                                     const unsigned short* palette_yuv, const unsigned char* action, int a256, int contour,
                                     const unsigned short* taps, int radius, const unsigned short* taps_c, int radius_c,
                                     void* out_y, long out_y_pitch, long out_y_stride,
                                     void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream);

/* The compositing painter (csrc/render_replace.hip): the overlay's picture mixed with a backdrop by a soft matte, so that tracks or the
 * background are REPLACED with an anti-aliased edge.  Every argument the entry shares with mdqe_render_mosaic_u8 means what it means
 * there (there is no `cell`); new are
 *   matte             uint8 [F, Ho, Wo], device: what mdqe_final_matte_u8 writes for the frames of `labels`;
 *   backdrop          uint8 [3], device: one colour in the frames' channel order -- or, with backdrop_picture = 1, uint8 [Ho, Wo, 3],
 *                     pixel-interleaved: one picture of the output's size, the same for every frame;
 *   mode              0 "background": the matte is the foreground that is kept; 1 "tracks": the matte covers what is replaced;
 *   action            uint8 [256], device: 0 keep, 1 tint, 4 replace; ANY other value acts as 0.  For this painter 4 acts as 0 too: WHAT
 *                     is replaced is said by the matte (made from the rows the caller's table selects), the action only says how the
 *                     pixel under it looks.
 * Integers only, ONE definition:
 *   base    mdqe_render_overlay_u8's pixel with the action deciding: action 1: palette[l][c] if edge, else (s_c*(256 - a256) +
 *           palette[l][c]*a256 + 128) >> 8; else s_c.  Source value, edge (on the LABELS) and blend are that entry's, unchanged;
 *   weight  Wt = matte[f, Y, X] (mode 0) or 255 - matte[f, Y, X] (mode 1);
 *   mix     mix(s, b, w) = (s*w + b*(255 - w) + 127) / 255, integer division (255 is odd: no ties; w = 255 gives s, w = 0 gives b);
 *   pixel   out_c = mix(base_c, B_c, Wt) with B = backdrop[c], or backdrop[Y][X][c] of the picture.
 * A pixel with Wt == 255 and a kept label therefore keeps the source byte.  MDQE_EINVAL for a mode or a backdrop_picture outside
 * {0, 1}; every other check is that of mdqe_render_mosaic_u8, made before any pointer is looked at; F == 0 returns OK and launches
 * nothing; a null matte or backdrop is refused as the labels are.  Nothing needs to be aligned.  One launch, no atomics: identical from
 * run to run.  Never allocates, never synchronises. */
int mdqe_render_replace_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                           const unsigned char* labels, int F, int Ho, int Wo,
                           const unsigned char* palette, const unsigned char* action, int a256, int contour,
                           const unsigned char* matte, const unsigned char* backdrop, int backdrop_picture, int mode,
                           unsigned char* out, int f_off, void* stream);
/* ... and on decoder surfaces: mdqe_render_mosaic_yuv420sp's arguments without `cell`, plus matte (uint8 [F, H, W]), mode, and the
 * backdrop as EITHER backdrop_yuv (uint16 [3]: Y, U, V in sample units; only the 8 / 10 bits are used) OR, with backdrop_yuv == NULL,
 * one surface (by, by_pitch, buv, buv_pitch) of the same H, W and fmt, the same for every frame.  Values are word >> 6 for P010.
 *   luma    Yout = mix(baseY, BY, Wt) with baseY the rule of mdqe_render_overlay_yuv420sp under the action (1 tints, else the sample);
 *   chroma  Cout = (sum_i mix(px_i(C), BC, Wt_i) + n / 2) >> log2(n) over the n in-picture pixels i of the pair's 2 x 2 block, px_i(C)
 *           being C or its tint by pixel i's action, label and edge, BC the colour's component or the backdrop surface's pair of
 *           that block;
 *   P010    a word the rule leaves unchanged -- a luma word whose label is kept (action != 1) with Wt == 255, a chroma pair whose whole
 *           block is such pixels -- is copied with all 16 bits; every other word is written as value << 6 (NV12: the same bytes).
 * In place is allowed under mdqe_render_overlay_yuv420sp's conditions: every sample is read and written by the thread that owns it.
 * Any other overlap of an output plane -- with an input plane, the labels, palette, action table, the matte or the backdrop -- is
 * MDQE_EINVAL, as is a backdrop pitch smaller than a row and (P010) an odd backdrop pointer or pitch.  mode outside {0, 1} is
 * MDQE_EINVAL before any pointer is looked at.  One launch, single samples at any alignment, no atomics. */
int mdqe_render_replace_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                                 int F, int H, int W, int fmt /*0 nv12, 1 p010*/, const unsigned char* labels,
                                 const unsigned short* palette_yuv, const unsigned char* action, int a256, int contour,
                                 const unsigned char* matte, const unsigned short* backdrop_yuv,
                                 const void* by, long by_pitch, const void* buv, long buv_pitch, int mode,
                                 void* out_y, long out_y_pitch, long out_y_stride,
                                 void* out_uv, long out_uv_pitch, long out_uv_stride, int f_off, void* stream);

/* Track boxes and captions on a painted picture (csrc/annotate.hip): the box and the text plate per instance that the demo's
 * visualiser draws on the host (demo/clip/visualizer.py:162,205; captions "[id] class score%", demo/visualizer.py:72-91).  An
 * ANNOTATION PASS: it runs behind any of the four painters above, IN PLACE on the painted picture, on the same stream; the painters
 * are not touched.  pic: uint8 [>= f_off + F, Ho, Wo, 3], frame f of the call is picture f_off + f; the surface entry's planes are
 * mdqe_render_overlay_yuv420sp's (pitches and strides in BYTES, fmt 0 NV12 / 1 P010, surface f at y + (f_off + f) * y_stride), read and
 * written.  geom: int32 [n*F, 5], row k*F + f = (area, xmin, ymin, xmax, ymax), the table mdqe_final_label_map_u8 writes; label l = k + 1.
 * palette / ink: uint8 [256, 3] (surfaces: uint16 [256, 3], rows (Y, U, V) in sample units), row l the colour of label l's box and plate /
 * of its text.  captions: uint8 [256, cap_len], row l the text of label l, ended by a 0 byte or by cap_len; NULL with cap_len == 0 (no
 * captions).  font: uint8 [64, 7], glyph ch - 32 for ch in 0x20..0x5F, 7 rows of 5 pixels, bit 4 the leftmost.  With Wo = W, Ho = H for
 * surfaces, integers only, ONE definition, for frame f and label l with (area, x0, y0, x1, y1) = geom[k*F + f]:
 *   live    area >= max(1, min_area) and 0 <= x0 <= x1 < Wo and 0 <= y0 <= y1 < Ho.  Any other row -- the empty row (0, Wo, Ho, -1, -1),
 *           garbage -- draws nothing; the entries are memory-safe for every table content;
 *   frame   (box > 0) the pixels with x0 <= X <= x1, y0 <= Y <= y1 and min(X - x0, x1 - X, Y - y0, y1 - Y) < box;
 *   plate   (cap_len > 0, and row l holds c >= 1 characters) w = (6c + 1) * scale by h = 9 * scale pixels at px = max(0, min(x0, Wo - w)),
 *           py = y0 - h if that is >= 0, else y0 (inside the box at the top edge); clipped to the picture;
 *   glyph   in a plate, u = X - px, v = Y - py, gx = u / scale - 1, gy = v / scale - 1: the pixel is INK when gx >= 0, 0 <= gy < 7,
 *           gx % 6 < 5 and bit 4 - gx % 6 of font[ch - 32][gy] is set, ch = caption byte gx / 6, a byte outside 0x20..0x5F drawn as '?';
 *           any other plate pixel has the plate colour;
 *   pixel   takes its FIRST hit among: the plates of the live labels in ascending l (ink: ink[l], else palette[l]), then the frames in
 *           ascending l (palette[l]).  A pixel that nothing hits is NOT WRITTEN;
 *   luma    the rule per sample with the Y components;
 *   chroma  a pair whose in-picture 2 x 2 block has no hit is not written (P010: it keeps all 16 bits of both words).  Any other pair:
 *           Cout = (sum_i px_i + n / 2) >> log2(n) over the block's n = 1, 2 or 4 in-picture pixels, px_i the hit's U (V) component for
 *           a hit pixel and the stored sample's VALUE otherwise -- mdqe_render_overlay_yuv420sp's chroma rule; P010 words are written as
 *           value << 6.
 * One thread owns each sample and each chroma pair: in place by construction.  A block owns a tile, compacts the plates and frames
 * that meet it into LDS in label order (capacity: all 255) and each pixel walks that list; a tile with an empty list returns without
 * reading or writing a pixel.  Stores are 4-byte wide where four neighbouring samples are all hit and their address is aligned,
 * single samples otherwise: nothing needs to be aligned.
 * MDQE_EINVAL, before any pointer is looked at, for box outside 0..4, scale outside 1..4, n outside 0..255, cap_len outside 0..64,
 * min_area < 0, F < 0, f_off < 0, Ho, Wo, H or W <= 0, F*Ho*Wo >= 2^31 - 1, and for the surface entry fmt outside {0, 1}, a pitch
 * smaller than a row, a negative stride, odd P010 pitches or strides, surfaces of a plane that share bytes (F > 1); odd P010 plane
 * pointers, odd palette_yuv / ink_yuv pointers and a luma plane that meets the chroma plane are MDQE_EINVAL too.  F == 0, n == 0 and
 * box == 0 with cap_len == 0 return OK and launch nothing.  ink, captions and font are looked at only when cap_len > 0.  One launch, no
 * atomics: identical from run to run.  Never allocates, never synchronises. */
int mdqe_annotate_u8(unsigned char* pic /* [.., Ho, Wo, 3] */, int F, int Ho, int Wo, int f_off,
                     const int* geom /* int32 [n*F, 5], row k*F+f: final_label_map's table */, int n,
                     const unsigned char* palette /*[256,3]*/, const unsigned char* ink /*[256,3]*/,
                     const unsigned char* captions /*[256, cap_len] or NULL*/, int cap_len,
                     const unsigned char* font /*[64, 7]*/, int box, int scale, int min_area, void* stream);
int mdqe_annotate_yuv420sp(void* y, long y_pitch, long y_stride, void* uv, long uv_pitch, long uv_stride,
                           int F, int H, int W, int fmt /*0 nv12, 1 p010*/, int f_off, const int* geom, int n,
                           const unsigned short* palette_yuv, const unsigned short* ink_yuv,
                           const unsigned char* captions, int cap_len, const unsigned char* font,
                           int box, int scale, int min_area, void* stream);

/* Per-track crops (csrc/crops.hip): one small fixed-size picture ("chip") per track and frame, cut from the frames the caller handed in and
 * resized on the device -- what a re-identification or attribute model, a thumbnail gallery or a reviewer takes next.  A second consumer
 * of the trio `annotate` reads: the frames, the label map, the map's geometry table.  labels: uint8 [F, Ho, Wo] as mdqe_final_label_map_u8
 * writes it, row k's label is k + 1; geom: int32 [n*F, 5], row k*F + f = (area, xmin, ymin, xmax, ymax) of that label's visible region;
 * frames, is_u8, frame_stride, h0, w0: exactly mdqe_render_overlay_u8's (never NULL here); the surface entry takes y .. bgr, exactly
 * mdqe_yuv420sp_to_rgb_u8's, in their place (h0 = H, w0 = W).  Chip size Sh x Sw, each 1..512; pad256 in 0..256 (the box grows by
 * pad256/256 of its width and height on each side); min_area >= 0; cutout in {0, 1}; fill = c0 | c1 << 8 | c2 << 16, three bytes in the
 * frames' channel order.  Integers only, ONE definition, for row k and window frame f with (area, xmin, ymin, xmax, ymax) = geom[k*F + f]:
 *   live       area >= max(1, min_area) and 0 <= xmin <= xmax < Wo and 0 <= ymin <= ymax < Ho: mdqe_annotate_u8's definition.  Any other
 *              row -- the empty row, garbage -- is not live; the entries are memory-safe for every table content;
 *   rect       px = ((xmax - xmin + 1) * pad256 + 128) >> 8, X0 = max(xmin - px, 0), X1 = min(xmax + px, Wo - 1), cw = X1 - X0 + 1; the
 *              same with y and Ho gives py, Y0, Y1, ch;
 *   footprint  of chip pixel (i, j), exact integer divisions: rows Ya = Y0 + (i*ch)/Sh up to but not including Yb = Y0 + ((i+1)*ch + Sh -
 *              1)/Sh, columns Xa = X0 + (j*cw)/Sw up to but not including Xb = X0 + ((j+1)*cw + Sw - 1)/Sw.  Never empty, never leaves
 *              the rect: a rect smaller than the chip is replicated, a larger one box-averaged;
 *   counted    every (Y, X) of the footprint; with cutout only those with labels[f, Y, X] == k + 1;
 *   source     mdqe_render_overlay_u8's: sy = (Y*h0)/Ho, sx = (X*w0)/Wo, s_c = frames[f, c, sy, sx], float32 as min(max(rint(v), 0), 255)
 *              with NaN -> 0; for surfaces the (R, G, B) -- bgr: (B, G, R) -- that mdqe_yuv420sp_to_rgb_u8 defines for sample (sy, sx);
 *   value      with m counted pixels and sum_c their channel sums: chip[i, j, c] = fill_c if m == 0, else (sum_c + m/2) / m;
 *   not live   the whole chip is fill and the rect written is (0, 0, -1, -1); otherwise the rect written is (X0, Y0, X1, Y1).
 * Frames taken: window frames f = f_first, f_first + f_step, ... < F, Fc of them.  The chip of (row k, t-th taken frame) is uint8 [Sh, Sw,
 * 3], pixel-interleaved, at out + k*out_row_stride + (c_off + t)*Sh*Sw*3; its rect int32 [4] at rects + k*rect_row_stride + (c_off + t)*4
 * (strides in elements).  Both are fully overwritten on every call and need no pre-initialisation; nothing else is written.
 * MDQE_EINVAL, before any pointer is looked at, for Sh or Sw outside 1..512, pad256 outside 0..256, min_area < 0, cutout outside {0, 1},
 * fill outside 0..0xFFFFFF, n outside 0..255, F < 0, Ho, Wo, h0 or w0 <= 0, Ho*Wo >= 2^24 (a uint32 sum of bytes cannot overflow), h0*Ho
 * or w0*Wo >= 2^31, f_first < 0, f_step < 1, c_off < 0, (c_off + Fc)*Sh*Sw*3 >= 2^31, a row stride smaller than the c_off + Fc chips /
 * rects of a row (n > 1), n * Fc * ceil(Sh*Sw / 256) >= 2^31, is_u8 outside {0, 1}, frames less than 3*h0*w0 apart (F > 1), and for
 * the surface entry every refusal of mdqe_yuv420sp_to_rgb_u8 (fmt, matrix, pitches, strides; odd P010 plane pointers).  n == 0, F == 0
 * or no frame taken (f_first >= F) return OK and launch nothing; NULL pointers give MDQE_ENULL.  Nothing needs to be aligned.
 * One launch, no floating point (but the float32 frames' rint), no atomics: identical from run to run.  A block of 256 threads owns 256
 * consecutive pixels of one chip; a chip whose footprints hold at most 256 source pixels gives each thread one chip pixel, a larger
 * footprint is summed by a whole wave, lanes striding it, with a cross-lane reduction -- integer sums, so either split gives the same
 * bits.  Never allocates, never synchronises. */
int mdqe_track_crops_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                        const unsigned char* labels, int F, int Ho, int Wo, const int* geom, int n,
                        int f_first, int f_step, int Sh, int Sw, int pad256, int min_area, int cutout, int fill,
                        unsigned char* out, long out_row_stride, int c_off, int* rects, long rect_row_stride, void* stream);
int mdqe_track_crops_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                              int H, int W, int fmt /*0 nv12, 1 p010*/, int matrix /*0 bt601, 1 bt709*/, int full_range, int bgr,
                              const unsigned char* labels, int F, int Ho, int Wo, const int* geom, int n,
                              int f_first, int f_step, int Sh, int Sw, int pad256, int min_area, int cutout, int fill,
                              unsigned char* out, long out_row_stride, int c_off, int* rects, long rect_row_stride, void* stream);

/* Track paths (csrc/paths.hip): where each track has been.  A third consumer of the label map, beside the annotation pass and the crops:
 * the centroid of every label's visible region per frame, and the trail of those centroids over the last frames painted onto a picture.
 * A centroid does not jump when an occluder cuts a mask the way a box centre does.  labels: uint8 [F, Ho, Wo] as mdqe_final_label_map_u8
 * writes it, row k's label is k + 1.  Integers only, ONE definition, for row k and frame f:
 *   moments  mom[k*F + f] = (m, SX, SY), int64: m the number of pixels with labels[f, Y, X] == k + 1, SX the sum of their X, SY of their Y
 *            (labels above n are not counted anywhere);
 *   present  m >= max(1, min_area);
 *   point    of a present row (cx, cy) = ((SX + m/2) / m, (SY + m/2) / m), integer divisions (the rounding of the crops and the mosaic);
 *            of any other row (-1, -1).  With pts != NULL it goes to pts[k*pts_row_stride + 2*(p_off + f) + {0, 1}] (int32, the stride in
 *            elements): a point table whose columns are frames, which a caller keeps over several windows.
 * mom and the written pts columns are fully overwritten on every call and need no pre-initialisation; nothing else is written.  Three
 * launches at most (zero the table; a sweep that gathers runs of equal labels in registers and adds them in closed form to a 64-bit LDS
 * table, then to the global one with 64-bit atomic adds; the division -- left out with pts == NULL): integer sums do not depend on their
 * order, identical from run to run.  Never allocates, never synchronises.
 * MDQE_EINVAL, before any pointer is looked at, for n outside 0..255, min_area < 0, F < 0, Ho or Wo <= 0 or > 16384, F*Ho*Wo >= 2^31 - 1,
 * p_off < 0, pts_row_stride < 2*(p_off + F) with n > 1 (two writers otherwise).  n == 0 or F == 0 return OK and launch nothing; NULL
 * labels or mom give MDQE_ENULL.  Nothing needs to be aligned.
 *
 * Trails: an ANNOTATION PASS like mdqe_annotate_u8 -- in place on a painted picture, behind any painter, on the same stream; pic and the
 * surface planes are that entry's (frame f of the call is picture f_off + f).  pts: the point table above; palette: uint8 [256, 3]
 * (surfaces: uint16 [256, 3], rows (Y, U, V) in sample units).  For frame f and label l = k + 1, with Wo = W, Ho = H for surfaces:
 *   points   columns j = p_off + f - trail .. p_off + f of row k; a column j < 0 is absent, and so is a point with x < 0, y < 0, x >= Wo
 *            or y >= Ho: the entries are memory-safe for every table content;
 *   strokes  each present point P gives the degenerate segment (P, P); each pair of present points A, B with no present point in a
 *            column between them the segment (A, B) -- gaps are bridged, an occluded track keeps one line;
 *   hit      with d = B - A, p = (X, Y) - A, L2 = d.d, s = p.d: if L2 == 0 or s <= 0, pixel (X, Y) is hit when 4*(p.p) <= width*width;
 *            if s >= L2 the same with p = (X, Y) - B; otherwise when 4*c*c <= width*width*L2, c = p.x*d.y - p.y*d.x.  64-bit integers
 *            (coordinates below 2^14: 4*c*c < 2^61).  Round caps; a width-1 line has a pixel in every column (row, on steep lines);
 *   pixel    takes palette[l] of the FIRST label in ascending l that hits it.  A pixel that nothing hits is NOT WRITTEN;
 *   luma     the rule per sample with the Y component;
 *   chroma   mdqe_annotate_yuv420sp's rule: a pair whose in-picture 2 x 2 block has no hit is not written (P010: it keeps all 16 bits of
 *            both words); any other pair is Cout = (sum_i px_i + n / 2) >> log2(n) over the block's in-picture pixels, px_i the hit's
 *            component for a hit pixel and the stored sample's VALUE otherwise, written as value << 6 for P010.
 * One thread owns each sample and each chroma pair: in place by construction.  A block owns a tile and compacts the segments whose box,
 * grown by `width`, meets it into LDS in label order, in chunks of 512 that keep that order; a tile without a segment returns without
 * reading or writing a pixel.  One launch, no atomics: identical from run to run.  Never allocates, never synchronises.
 * MDQE_EINVAL, before any pointer is looked at, for trail outside 1..64, width outside 1..5, n outside 0..255, F < 0, f_off < 0,
 * p_off < 0, Ho, Wo, H or W <= 0 or > 16384, F*Ho*Wo >= 2^31 - 1, pts_row_stride < 2*(p_off + F) with n > 1, and for the surface entry
 * every plane refusal of mdqe_annotate_yuv420sp.  F == 0 and n == 0 return OK and launch nothing; NULL pointers give MDQE_ENULL. */
int mdqe_label_centroids_u8(const unsigned char* labels, int F, int Ho, int Wo, int n, int min_area, long long* mom /* int64 [n*F, 3] */,
                            int* pts /* int32 or NULL */, long pts_row_stride, int p_off, void* stream);
int mdqe_render_trails_u8(unsigned char* pic /* [.., Ho, Wo, 3] */, int F, int Ho, int Wo, int f_off,
                          const int* pts, long pts_row_stride, int p_off, int n, int trail, int width,
                          const unsigned char* palette /*[256,3]*/, void* stream);
int mdqe_render_trails_yuv420sp(void* y, long y_pitch, long y_stride, void* uv, long uv_pitch, long uv_stride,
                                int F, int H, int W, int fmt /*0 nv12, 1 p010*/, int f_off,
                                const int* pts, long pts_row_stride, int p_off, int n, int trail, int width,
                                const unsigned short* palette_yuv, void* stream);

/* Track outlines (csrc/polygons.hip): the label map's visible regions as polygons, traced on the device.  A fourth consumer of the
 * label map.  labels: uint8 [F, Ho, Wo] as mdqe_final_label_map_u8 writes it, 0 = background, row k's label is k + 1; rows k = 0..n-1
 * are traced and a label above n is "not this region", as in mdqe_label_centroids_u8.  Integers only, ONE definition:
 *   lattice   vertices (X, Y), 0 <= X <= Wo, 0 <= Y <= Ho; pixel (x, y) covers the square (x, y)..(x + 1, y + 1); X goes right, Y down.
 *   edges     for label v in frame f let R be the pixels that hold v.  Every unit crack between a pixel of R and a pixel outside R (or
 *             outside the picture) is a directed edge with R on its RIGHT.  For pixel (x, y) of R:
 *               top,    if (x, y-1) is not in R: (x, y)     -> (x+1, y),   heading E;
 *               right,  if (x+1, y) is not in R: (x+1, y)   -> (x+1, y+1), heading S;
 *               bottom, if (x, y+1) is not in R: (x+1, y+1) -> (x, y+1),   heading W;
 *               left,   if (x-1, y) is not in R: (x, y+1)   -> (x, y),     heading N.
 *   successor among the edges of the same label and frame that leave the head vertex: the right turn before straight on before the left
 *             turn.  A bijection on the edges, so they fall into closed rings; regions are 4-connected; a ring may touch itself at a
 *             vertex (a pinch), visits a vertex at most twice and never crosses itself.
 *   vertices  a ring's vertices are the tails of those of its edges whose predecessor has another heading: the corners only, collinear
 *             points dropped.  Every ring has an even number of them, at least 4.
 *   order     a corner's key is (f, Y, X, heading out) with E < S < W < N.  A ring starts at its smallest corner and is listed along the
 *             successors; the rings of a call are listed by ascending start key, whatever their label, and each names its row.
 *   holes     a ring is a hole exactly when its start corner's heading out is S; an outer ring's is E.  With A2 = sum(x_i * y_{i+1} -
 *             x_{i+1} * y_i) over a ring, outer rings have A2 > 0, holes A2 < 0, and the A2 of the rings of (k, f) sum to twice the
 *             region's pixel count; an even-odd fill of them is the region.
 *   min_area  the rings of a region (k, f) of fewer than max(1, min_area) pixels are left out entirely (counted by a pass of this entry's
 *             own, made only for min_area > 1).
 * xy: int32 [cap_vertices, 2], (X, Y), ring after ring in ring order; rings: int32 [cap_rings, 5], (row k, frame f, first vertex, vertex
 * count, hole 0|1); totals: int32 [2], the TRUE vertex and ring counts whatever the caps.  Both outputs are fully overwritten up to the
 * counts, identical from run to run (every index comes from a scan; the only atomics count).  Where either count exceeds its cap, xy and
 * rings hold unspecified data inside their caps and nothing is written outside them: call again with the true counts.
 * The launches are in csrc/polygons.hip's head: mark and count corners per lattice vertex from an LDS tile of labels, scan, link each
 * corner to its successor along its straight run, rank by ceil(log2(cap_vertices)) rounds of pointer jumping (a number the host fixes
 * from the cap), scan the ring starts and sizes, emit.  No workgroup waits for another inside a launch.  workspace: at least
 * mdqe_label_polygons_workspace(F, Ho, Wo, cap_vertices) bytes (-1 for sizes the entry refuses), 16-byte aligned, device memory, one per
 * stream; it holds 2 bytes per lattice vertex and 45 per vertex of the cap.  Never allocates, never synchronises.
 * MDQE_EINVAL, before any pointer is looked at, for n outside 0..255, min_area < 0, F < 0, Ho or Wo <= 0 or > 16384, F*Ho*Wo >= 2^31 - 1,
 * cap_vertices outside 1..2^26, cap_rings outside 1..2^24, and a workspace that is too small.  n == 0 or F == 0 write totals = (0, 0),
 * which is all they launch; NULL totals, and then NULL labels, xy, rings or workspace, give MDQE_ENULL. */
int mdqe_label_polygons_u8(const unsigned char* labels, int F, int Ho, int Wo, int n, int min_area,
                           int cap_vertices, int cap_rings,
                           int* xy,        /* [cap_vertices, 2]: (X, Y), ring after ring in ring order */
                           int* rings,     /* [cap_rings, 5]: (row k, frame f, first vertex, vertex count, hole 0|1) */
                           int* totals,    /* [2]: the TRUE vertex and ring counts, whatever the caps */
                           void* workspace, long workspace_bytes, void* stream);
long mdqe_label_polygons_workspace(int F, int Ho, int Wo, int cap_vertices);

/* The redaction margin (csrc/grow.hip): a copy of the label map in which chosen labels have GROWN by up to `radius` pixels, for the
 * overlay painters to take in place of the map (a mask under-covers hair, fingers and blurred borders).  labels: uint8 [F, Ho, Wo] as
 * mdqe_final_label_map_u8 writes it; out: uint8 [F, Ho, Wo];
 *   grow     uint8 [256], device: label g GROWS when g >= 1 and grow[g] != 0.  grow[0] is ignored: the background never grows;
 *   radius   0..32, in pixels.
 * Integers only, ONE definition, for frame f and pixel (Y, X) with l = labels[f, Y, X]:
 *   kept       if l grows, out = l: a growing region is never overwritten;
 *   candidates otherwise, the pixels (Y', X') of the SAME frame, inside the picture, whose label grows and for which
 *              d2 = (Y - Y')^2 + (X - X')^2 <= radius^2 (a Euclidean disc);
 *   pixel      without a candidate out = l; else out is the label of the candidate with the smallest pair (d2, label) in
 *              lexicographic order: the nearest, and of equally near ones the smallest label.
 * Growing labels spread over the background and over tracks that do not grow.  Nothing is read beyond the picture's border (no
 * replication).  radius = 0, or a table without a growing label, gives out == labels.  A single pixel grows to 1, 5, 13, 29, 81 pixels
 * at radius 0, 1, 2, 3, 5.  The minimum separates: a column pass keeps, per (Y, X'), the smallest (dy^2, label) over |dy| <= radius; a
 * row pass takes the smallest (dx^2 + that dy^2, label) over |dx| <= radius and accepts d2 <= radius^2 -- exactly the definition.
 * MDQE_EINVAL for a radius outside 0..32, a negative F, Ho or Wo, F*Ho*Wo >= 2^31 - 1 -- all before any pointer is looked at -- and,
 * when F*Ho*Wo > 0, for a null labels, grow or out and for an out that meets labels or grow in any byte: the entry does NOT work in
 * place, a pixel reads its neighbours' labels.  F == 0 or an empty picture returns OK and launches nothing.  Nothing needs to be
 * aligned.  Only tiles (16 x 64 pixels) whose neighbourhood of `radius` holds a growing label are searched; the others are copied.  One
 * launch, no global scratch, no atomics: identical from run to run.  Never allocates, never synchronises. */
int mdqe_grow_labels_u8(const unsigned char* labels, int F, int Ho, int Wo,
                        const unsigned char* grow /* [256], device */, int radius,
                        unsigned char* out /* [F, Ho, Wo] */, void* stream);

/* Object removal (csrc/plate.hip): a BACKGROUND PLATE learned from the pixels no track covers, and the picture of it that the
 * compositing painters (mdqe_render_replace_u8 / mdqe_render_replace_yuv420sp) take as their backdrop picture or surface, so that
 * replaced tracks show the scene behind them.  Per video and device, STATE on the output grid, int32, 16-byte aligned, all zero when fresh:
 *   RGB       plate   [Ho, Wo, 4]  cells (P_0, P_1, P_2, n);
 *   surfaces  plate_y [H, W, 2]    cells (P, n), and plate_c [ch, cw, 4] cells (P_U, P_V, n, 0), ch = (H + 1) / 2, cw = (W + 1) / 2.
 * P is the sample in 24.8 fixed point, n the number of observations, saturating at n_max (1..256).  A state started from an empty-scene
 * picture holds P = 256 * value and n = 1 everywhere.  Integers only, ONE definition:
 *   observed  block: uint8 [F, Ho, Wo] (surfaces: [F, H, W]), non-zero = "not background here": the label map, or that map grown by a
 *             margin (mdqe_grow_labels_u8 with every label growing).  RGB pixel (Y, X) and a luma sample are observed in frame f iff
 *             block[f, Y, X] == 0; a chroma pair iff every in-picture pixel of its 2 x 2 block is;
 *   value     RGB: s_c is exactly mdqe_render_overlay_u8's source value (nearest-sampled onto the output grid, float32 by the rint /
 *             clamp / NaN rule; frames are required); surfaces: the sample itself, word >> 6 for P010;
 *   update    per observed value, the call's frames in order:  n' = min(n + 1, n_max);  d = 256 * s - P;
 *             P' = P + floordiv(d + (n' >> 1), n'), floordiv rounding towards minus infinity;  n = n'.  (The channels of a cell share n.)
 *             The first observation sets P = 256 * s, the first n_max form a rounded cumulative mean, later ones an exponential mean
 *             of weight 1 / n_max; a background that does not change is reproduced exactly; P stays in [0, 256 * max sample].
 *   picture   a seen cell (n > 0) shows (P + 128) >> 8 per channel.  A never-seen cell (Y, X) shows the value of the seen cell
 *             (Y', X') of its plane with the smallest triple (d2, Y', X') in lexicographic order, d2 = (Y - Y')^2 + (X - X')^2 <= reach^2;
 *             without one it shows `fill`.  Nothing is read beyond the plane.  The chroma plane does the same on its own grid with
 *             reach (reach + 1) / 2 and the fill's (U, V).  P010 words are written as value << 6.
 * The minimum separates as mdqe_grow_labels_u8's does: a column pass keeps, per (Y, X'), the smallest key dy^2 << 8 | (dy + reach) over
 * the seen cells with |dy| <= reach; a row pass scans dx = -reach .. reach ascending and takes a strictly smaller dx^2 << 8 + key --
 * exactly the definition's triple.
 * mdqe_plate_update_u8: frames, is_u8, frame_stride, h0, w0 are mdqe_render_overlay_u8's (frames not NULL); mdqe_plate_update_yuv420sp:
 * y .. fmt are mdqe_render_overlay_yuv420sp's (pitches and strides in BYTES).  One thread per state cell walks the F frames: one
 * 16-byte (luma: 8-byte) load and store of the cell per launch.  mdqe_plate_picture_u8: out uint8 [Ho, Wo, 3], pixel-interleaved,
 * fill uint8 [3], device; mdqe_plate_picture_yuv420sp: ONE surface (out_y, out_y_pitch, out_uv, out_uv_pitch) of H x W fmt, fill_yuv
 * uint16 [3] (Y, U, V) in sample units, device (only the 8 / 10 bits are used).  A tile (16 x 64 cells) whose own cells are all seen
 * skips the search.  Output padding is never written.
 * MDQE_EINVAL, before any pointer is looked at: n_max outside 1..256, reach outside 0..32, negative F, Ho, Wo (surfaces: H or W <= 0),
 * Ho * Wo * 4 >= 2^31, F * Ho * Wo >= 2^31 - 1, h0 or w0 < 1, h0 * Ho or w0 * Wo >= 2^31, frame_stride < 3 * h0 * w0, fmt outside {0, 1},
 * a pitch smaller than a row, a negative stride, odd P010 pitches or strides.  F == 0 or an empty picture returns OK and launches
 * nothing.  Then: a null pointer, a state that is not 16-byte aligned, odd P010 plane pointers, and ANY overlap of the state with
 * an input (frames or surfaces, block, fill) or an output, or of an output with the fill, are MDQE_EINVAL.  Outputs need no alignment
 * (single samples).  One launch each, no atomics, no global scratch: identical from run to run.  Never allocates, never synchronises. */
int mdqe_plate_update_u8(const void* frames, int is_u8, long frame_stride, int h0, int w0,
                         const unsigned char* block, int F, int Ho, int Wo, int n_max, int* plate /* [Ho, Wo, 4] */, void* stream);
int mdqe_plate_update_yuv420sp(const void* y, long y_pitch, long y_stride, const void* uv, long uv_pitch, long uv_stride,
                               int F, int H, int W, int fmt /*0 nv12, 1 p010*/, const unsigned char* block, int n_max,
                               int* plate_y /* [H, W, 2] */, int* plate_c /* [ch, cw, 4] */, void* stream);
int mdqe_plate_picture_u8(const int* plate, int Ho, int Wo, int reach, const unsigned char* fill /* [3], device */,
                          unsigned char* out /* [Ho, Wo, 3] */, void* stream);
int mdqe_plate_picture_yuv420sp(const int* plate_y, const int* plate_c, int H, int W, int fmt /*0 nv12, 1 p010*/, int reach,
                                const unsigned short* fill_yuv /* [3], device */,
                                void* out_y, long out_y_pitch, void* out_uv, long out_uv_pitch, void* stream);

/* ---- COCO single-image branch, after the decoder (MDQE.inference_image, mdqe/mdqe.py:486-556), on the centre frame's
 * low-resolution logits [n,Hm,Wm]; aligned_bilinear x`factor` in closed form, crop [:h,:w].
 * stats[k] = {sum(sigmoid*[sigmoid>0.5]), count(sigmoid>0.5), xmin, ymin, xmax, ymax of (logit > 0)} (:512-516, :526;
 * BitMasks.get_bounding_boxes = [xmin, ymin, xmax+1, ymax+1]; xmin > xmax for an empty mask).
 * final masks: F.interpolate(bilinear, align_corners=False) of the cropped up-sampled logits to (Ho,Wo), > 0 (:545-547);
 * row k of out (uint8 [n_sel,Ho,Wo]) takes mask idx_dev[k]. */
int mdqe_image_mask_stats_f32(const float* logits, int n, int Hm, int Wm, int factor, int h, int w, float* stats, void* stream);
int mdqe_image_final_masks_u8(const float* logits, int n_sel, const int* idx_dev, int Hm, int Wm, int factor, int h, int w,
                              int Ho, int Wo, unsigned char* out, void* stream);

/* ---- SwinV2 backbone (mdqe/backbone/swin_transformer_v2.py) --------------------------------------------
 * layernorm_post: y = LN(x)*gamma + beta + post (res-post-norm :287-288).
 * patch4_im2col: normalise + zero-pad + 4x4/s4 im2col, k = c*16+kh*4+kw -> [NI*Hp/4*Wp/4, 48] (PatchEmbed :466-479).
 * swin_window: mode 0 gathers the zero-padded, cyclically shifted map into window-ordered rows [B*nW*ws*ws, C];
 *              mode 1 writes dst[b,y,x,:] = shortcut[b,y,x,:] + rows (window reverse + un-shift + crop, :252-288).
 * window_attn: cosine attention of WindowAttention.forward (:147-186) on qkv rows [n_windows*N, 3C]; scale [nh] =
 *              exp(clamp(logit_scale)), bias [nh,N,N] = 16*sigmoid(cpb), mask [nW,N,N] or NULL (device arrays).
 * patch_merge_gather: [B,H,W,C] -> [B*ceil(H/2)*ceil(W/2), 4C] in the order x0|x1|x2|x3 of PatchMerging (:311-335). */
int mdqe_layernorm_post_f32(const float* x, const float* gamma, const float* beta, const float* post, float* y,
                            long rows, int C, float eps, void* stream);
/* Round 4: the window partition and its reverse without their copies (SwinTransformerBlock.forward, swin_transformer_v2.py:236-288).
 * mdqe_gemm_nt_swin_f32: C = window_partition(roll(pad(X))) W^T + bias -- the qkv product (WindowAttention.forward :153-155) reads its A
 *   rows from the NHWC map X [B, H, Wd, lda] through the window order; C [B*Hp*Wp, ldc], Hp / Wp = H / Wd rounded up to multiples of ws;
 *   padded positions read zeros.  Exact-fp32 mode only (MDQE_EINVAL in the split-precision mode: partition first, then mdqe_gemm_nt_f32).
 * mdqe_layernorm_swin_scatter_f32: out[b,y,x,:] = shortcut[b,y,x,:] + LN(rows[r,:]) * gamma + beta with r the window-order row of the
 *   pixel: norm1, window reverse, un-shift, crop and the residual add (:273-287) in one pass; out may alias shortcut. */
int mdqe_gemm_nt_swin_f32(const float* X, long lda, const float* W, const float* bias, float* C, long ldc, int B, int H, int Wd,
                          int ws, int shift, int N, int K, void* stream);
int mdqe_layernorm_swin_scatter_f32(const float* rows, const float* gamma, const float* beta, const float* shortcut, float* out,
                                    int B, int H, int W, int C, int ws, int shift, float eps, void* stream);
int mdqe_patch4_im2col_f32(const void* frames, int is_u8, long frame_stride, int NI, int h, int w, int Hp, int Wp,
                           const float* mean3_host, const float* std3_host, float* out, void* stream);
int mdqe_swin_window_f32(const float* src, const float* shortcut, float* dst, int B, int H, int W, int C, int ws,
                         int shift, int mode, void* stream);
int mdqe_window_attn_f32(const float* qkv, long ld, float* o, long ldo, int n_windows, int N, int C, int nh,
                         const float* scale, const float* bias, const float* mask, int nW, void* stream);
int mdqe_patch_merge_gather_f32(const float* x, float* out, int B, int H, int W, int C, void* stream);

#ifdef __cplusplus
}
#endif
#endif
