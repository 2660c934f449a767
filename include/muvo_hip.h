/* muvo_hip.h — C ABI of libmuvo_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the MUVO
 * world-model training step.  Plain pointers and sizes only (no torch types); every tensor is
 * caller-allocated device memory, fp32 contiguous NCHW / NCDHW unless stated; `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  The library keeps no global state besides the last error
 * string.  Every entry returns 0 on success, a negative MUVO_ERR_* otherwise; muvo_last_error() gives
 * the message.  The host side (muvo_amd/ops.py) binds these through ctypes and raises RuntimeError.
 *
 * Each group cites the reference op it replaces (paths relative to the reference repository).
 */
#ifndef MUVO_HIP_H
#define MUVO_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MUVO_OK 0
#define MUVO_ERR_INVALID_ARG (-1)
#define MUVO_ERR_HIP (-2)
/* (no collective error code: the library launches no collectives - gradient exchange is torch.distributed over RCCL, muvo_amd/parallel.py) */

#define MUVO_ACT_NONE 0
#define MUVO_ACT_RELU 1
#define MUVO_ACT_LEAKY 2 /* slope parameter */
#define MUVO_ACT_ELU 3   /* alpha = 1 */
#define MUVO_ACT_TANH 4
#define MUVO_ACT_SIGMOID 5

const char* muvo_last_error(void);
int muvo_abi_version(void);
/* one-launch self test of the MFMA operand/accumulator lane maps; returns 0 when C = A*B is exact */
int muvo_selftest_mfma(void* stream);
/* Deterministic mode (also MUVO_DETERMINISTIC=1 in the environment): reductions that otherwise depend on the arrival order of
 * float / double atomics (split-K partial sums, weight-gradient pixel ranges, bias / statistics / loss partial sums) run with one
 * contributor per address or are added in index order: two runs of the same step give bit-identical results.  A debugging
 * aid for parity work - slower (the affected kernels lose their split parallelism).  The reference has no counterpart
 * (torch.use_deterministic_algorithms plays this role for its cuDNN / ATen kernels). */
int muvo_set_deterministic(int on);
/* Clears the library-owned statistics accumulators of every stream (all-zero between operations by construction: the consuming
   kernel clears what it read).  For the caller's error path: an exception between a statistics pass and its consumer leaves
   partial sums behind that every later normalisation on that stream would add to (muvo_amd/ops.py: reset_accumulators). */
int muvo_reset_accumulators(void);
int muvo_get_deterministic(void);

/* ---- convolution family (conv_gemm.hip) -------------------------------------------------------
 * Replaces nn.Conv2d / nn.Conv3d / nn.ConvTranspose2d forward, data-gradient and weight-gradient:
 * muvo/models/common.py:549-632 (ConvDecoder), :161-202,498-546 (VoxelDecoder1), :102-130 (DecoderDS),
 * :249-367 (1x1 heads), muvo/layers/layers.py:9-66, timm ResNet-18 (muvo/models/mile.py:24,81).
 * Axes are (D,H,W); 2-D problems use D = 1, ksz[0] = 1, stride[0] = 1, pad[0] = 0, dil[0] = 1.
 * Weight layout is PyTorch's: Conv [Cout][Cin][kD][kH][kW], ConvTranspose [Cin][Cout][kD][kH][kW]. */
typedef struct muvo_conv_desc {
  int32_t nd;         /* 2 or 3 */
  int32_t transposed; /* 0 Conv, 1 ConvTranspose */
  int32_t N, Cin, Cout;
  int32_t in_sz[3], out_sz[3];
  int32_t ksz[3], stride[3], pad[3], dil[3];
} muvo_conv_desc;

/* Matrix-pipe arithmetic of the large contractions (process-wide; packed weights depend on it, so repack after a
 * change).  MUVO_CONV_F32: exact fp32-input MFMA (157 TFLOP/s peak).  MUVO_CONV_BF16X3: every fp32 operand is split
 * into bf16 hi + lo and each product formed as hi*hi + hi*lo + lo*hi on bf16 MFMA with fp32 accumulation
 * (3/16 of the fp32-MFMA cost, per-product relative error <= ~1e-5).  Initial value: env MUVO_CONV_MFMA=f32|bf16x3. */
#define MUVO_CONV_F32 0
#define MUVO_CONV_BF16X3 1
#define MUVO_CONV_MODE_DEFAULT MUVO_CONV_BF16X3
/* Products per fp32 product on the split-product implicit-GEMM kernels (MUVO_CONV_BF16X3 mode): 3 = hi*hi + hi*lo + lo*hi
 * (default, fp32-equivalent); 1 = hi*hi only, i.e. plain bf16 operands with fp32 accumulation - the arithmetic of the
 * reference's shipped PRECISION '16-mixed' (muvo/config.py:40) and of BASELINE.json configs[4] ("bf16").  An EXTENSION outside
 * the fp32 1e-3 parity contract: a third of the MFMA work; the voxel 3x3x3 kernels keep three products. */
int muvo_conv_set_products(int n);
int muvo_conv_get_products(void);
int muvo_conv_set_mode(int mode);
int muvo_conv_get_mode(void);
/* Which convolutions use the split-product kernels in MUVO_CONV_BF16X3 mode.  gflop_per_item >= 0: every phase with
 * at least this much work per batch item (GFLOP, 2*MAC); smaller ones stay on exact fp32 MFMA (env
 * MUVO_BF16X3_MIN_GFLOP sets the same threshold at start-up).  Negative (the initial state without the env variable):
 * the built-in policy fitted to per-layer timings on MI355X - an operation needs >= 0.1 GFLOP and >= 256 result pixels
 * per batch item and >= 16 reduction channels (weight gradients: >= 0.05 GFLOP per item and more than one tap). */
int muvo_conv_set_bf16x3_min_gflop(double gflop_per_item);
/* nn.Linear on token-major activations [rows][features] with thousands of rows (the transformer encoder:
 * muvo/models/mile.py:96-101, 558-561 - nn.TransformerEncoderLayer in_proj / out_proj / linear1 / linear2) on the bf16x3
 * implicit-GEMM kernels, as a 1x1 convolution over a one-row image of `rows` pixels.  Needs in_f % 8 == 0, out_f % 16 == 0,
 * both >= 64.  pack: w [out_f][in_f] -> the two packed operands (sizes from pack_floats); split: x -> bf16 hi/lo planes
 * (workspace_bytes(rows, features)); forward: y = act(x W^T + b) from the planes of x; dgrad: dx = dz W from the planes
 * of dz; wgrad: dw += dz^T x from both (scratch: out_f * in_f floats, all-zero on entry, left all-zero). */
int muvo_linear_bf16x3_pack_floats(int in_f, int out_f, int64_t* fwd_floats, int64_t* dgrad_floats);
int muvo_linear_bf16x3_pack(int in_f, int out_f, const float* w, float* wp_fwd, float* wp_dgrad, void* stream);
int64_t muvo_linear_bf16x3_workspace_bytes(int64_t rows, int features);
int muvo_linear_bf16x3_split(const float* x, int64_t rows, int features, void* ws, void* stream);
int muvo_linear_bf16x3_forward(int64_t rows, int in_f, int out_f, const void* ws_x, const float* wp_fwd, const float* bias,
                               float* y, int act, float slope, void* stream);
int muvo_linear_bf16x3_dgrad(int64_t rows, int in_f, int out_f, const void* ws_dz, const float* wp_dgrad, float* dx,
                             void* stream);
int muvo_linear_bf16x3_wgrad(int64_t rows, int in_f, int out_f, const void* ws_x, const void* ws_dz, float* scratch,
                             float* dw, void* stream);
/* Batched weight packing: all packed copies go stale with every optimizer step; instead of one or more small launches per
 * layer, list the layers once in a host array of muvo_pack_table_item_bytes()-sized entries (add appends the phases of a
 * layer and advances *n_items / *n_blocks; it returns 1 and appends nothing for shapes served by the voxel / head kernels,
 * which keep using muvo_conv_pack_weights), copy the array to the device, and call run after each optimizer step: one
 * launch refreshes every listed copy.  Source and destination pointers are captured at add time. */
int64_t muvo_pack_table_item_bytes(void);
int muvo_conv_pack_table_add(void* host_items, int capacity, int* n_items, int64_t* n_blocks, const muvo_conv_desc* d,
                             const float* w, float* wp_fwd, float* wp_dgrad);
int muvo_linear_bf16x3_pack_table_add(void* host_items, int capacity, int* n_items, int64_t* n_blocks, int in_f, int out_f,
                                      const float* w, float* wp_fwd, float* wp_dgrad);
int muvo_pack_table_run(const void* dev_items, int n_items, int64_t n_blocks, void* stream);
/* sizes (in floats) of the K-major packed weight buffers used by forward/wgrad and by dgrad */
int muvo_conv_pack_sizes(const muvo_conv_desc* d, int64_t* fwd_floats, int64_t* dgrad_floats);
/* repack w into wp_fwd and/or wp_dgrad (either may be NULL) */
int muvo_conv_pack_weights(const muvo_conv_desc* d, const float* w, float* wp_fwd, float* wp_dgrad, void* stream);
/* bytes of workspace that forward (op 0: ws), dgrad (op 1: ws) and wgrad (op 2: ws_x, op 3: ws_dy) need for this shape
 * in the current mode (0 = none; the bf16x3 kernels read channels-last bf16 hi/lo copies of their activation operands,
 * which the call writes there first).  The copy of x is the same for op 0 and op 2, the copy of dy for op 1 and op 3. */
int64_t muvo_conv_workspace_bytes(const muvo_conv_desc* d, int op);
/* kernel family that serves this shape in the current mode (for profiling/roofline attribution): 0 exact-fp32 implicit
 * GEMM, 1 bf16x3 implicit GEMM, 2 4x4x1-MFMA small-channel Conv3d, 3 float4 VALU heads, 4 bf16x3 small-channel Conv3d;
 * op 0 fwd, 1 dgrad, 2 wgrad */
int muvo_conv_kernel_family(const muvo_conv_desc* d, int op);
/* family 1 only: 1 = the launch uses the eight-wave ping-pong tiles (256x128 / 128x256), 0 = the four-wave small tiles */
int muvo_conv_kernel_variant(const muvo_conv_desc* d, int op);
/* y = act(conv(x, w) + bias); bias may be NULL; ws may be NULL when muvo_conv_workspace_bytes(d, 0) == 0 */
int muvo_conv_forward(const muvo_conv_desc* d, const float* x, const float* wp_fwd, const float* bias, float* y, int act,
                      float slope, void* ws, void* stream);
/* dx = conv_data_grad(dy, w) (dy already multiplied by act'(y) by the caller); ws_valid != 0: ws already holds the split
 * planes of dy (written by muvo_conv_prepare_dy), dy itself is then not read by the bf16x3 path */
int muvo_conv_dgrad(const muvo_conv_desc* d, const float* dy, const float* wp_dgrad, float* dx, void* ws, int ws_valid,
                    void* stream);
/* muvo_conv_forward that also accumulates, per (n, output channel), the sum and the sum of squares of the ACTIVATED output into
 * moments[N][Cout][2] (doubles, all-zero on entry): the statistics of the instance norm that follows the convolution
 * (ConvInstanceNorm3d, common.py:190-202), taken from the epilogue registers instead of a pass over the output tensor.  Only
 * the bf16x3 voxel kernels (muvo_conv_kernel_family(d, 0) == 4) do this: ask muvo_conv_forward_moments_supported first.
 * muvo_adain_fwd_moments consumes such a buffer (and leaves it all-zero). */
/* muvo_conv_forward + the 1x1 head on its output (ConvDecoder stage + RGBHead / LidarReHead, muvo/models/common.py:608-632,
 * 287-303): logits (N, CO, out spatial) = head_b + head_w (CO, Cout) . y per pixel, formed in the convolution's epilogue from
 * the activated values while they are stored - the head's forward makes no pass over y.  Ask _supported first (eight-wave
 * bf16x3 tiles, no split-K, Cout % 64 == 0, CO <= 4, CO * Cout <= 1024, y below 2 GB). */
int muvo_conv_forward_head_supported(const muvo_conv_desc* d, int CO);
int muvo_conv_forward_head(const muvo_conv_desc* d, const float* x, const float* wp_fwd, const float* bias, float* y, int act,
                           float slope, void* ws, const float* head_w, const float* head_b, int CO, float* logits, void* stream);
int muvo_conv_forward_moments_supported(const muvo_conv_desc* d);
int muvo_conv_forward_moments(const muvo_conv_desc* d, const float* x, const float* wp_fwd, const float* bias, float* y, int act,
                              float slope, double* moments, void* stream);
int muvo_adain_fwd_moments(const float* x, const float* style, float* y, float* save_mean, float* save_rstd, double* moments,
                           int N, int C, int64_t S, float eps, void* stream);
/* AdaIN folded into the consumer (muvo/models/common.py:190-202: conv -> AdaptiveInstanceNorm3d -> next conv inside a
 * DecoderBlock3d).  muvo_adain_affine: statistics from `moments` (as muvo_adain_fwd_moments; cleared) -> save_mean / save_rstd
 * (N*C, for muvo_adain_bwd) and aff[N][C][2] = (style_scale * rstd, style_shift - style_scale * rstd * mean); no pass over x.
 * muvo_conv_forward_affine / muvo_conv_wgrad_affine: the convolution / its weight gradient on scale * x + shift per (n, input
 * channel) with zero padding applied after the map (bf16x3 voxel kernels with 8 / 16 input channels:
 * muvo_conv_affine_supported); moments (may be NULL) as in muvo_conv_forward_moments; dw / dbias are accumulated. */
int muvo_adain_affine(const float* style, double* moments, float* save_mean, float* save_rstd, float* aff, int N, int C, int64_t S,
                      float eps, void* stream);
int muvo_conv_affine_supported(const muvo_conv_desc* d);
int muvo_conv_forward_affine(const muvo_conv_desc* d, const float* x, const float* aff, const float* wp_fwd, const float* bias,
                             float* y, int act, float slope, double* moments, void* stream);
int muvo_conv_wgrad_affine(const muvo_conv_desc* d, const float* x, const float* aff, const float* dy, float* dw, float* dbias,
                           void* stream);
/* Grouped Linear: L <= 16 layers y_l = x W_l^T + b_l on the same input x (M <= 24 rows, K features, K % 4 == 0) in one launch
 * per pass — the style projections of all AdaptiveInstanceNorm layers of a decoder (muvo/models/common.py:205-246,227-246:
 * `self.latent_affine(style)` per layer on the same latent).  W[l]: (N[l], K) row-major, b[l]: (N[l]) or NULL, Y[l]: (M, N[l]).
 * bwd: dx (M, K) is OVERWRITTEN with sum_l dY_l W_l (NULL: skipped); dW[l] / db[l] are accumulated (NULL entries / NULL
 * arrays: skipped).  The pointer arrays are host arrays. */
int muvo_grouped_linear_fwd(const float* x, int M, int K, int L, const float* const* W, const float* const* b, float* const* Y,
                            const int* N, void* stream);
int muvo_grouped_linear_bwd(const float* x, int M, int K, int L, const float* const* W, float* const* dY, float* dx,
                            float* const* dW, float* const* db, const int* N, void* stream);
/* Routing query of the three grouped launches (host code only): the forward row template (8 | 24) and its grid, the grids of
 * the data-gradient (K / 64 column blocks x 128-row weight slabs) and weight-gradient (K / 256 x 16-row groups) kernels. */
typedef struct muvo_grouped_linear_route_info {
  int32_t fwd_rm, fwd_grid;
  int32_t dgrad_grid[2], wgrad_grid[2];
} muvo_grouped_linear_route_info;
int muvo_grouped_linear_route(int M, int K, int L, const int* N, muvo_grouped_linear_route_info* out);
/* Clock probe of the dominant kernel class (eight-wave bf16x3 implicit-GEMM tiles): shader clock (MHz) and wall time per
 * K step (32 deep, 24 MFMA 32x32x16 per wave) that workgroup 0 of the most recent launch measured over its K loop.  The
 * kernels run power-limited well below the 2.4 GHz the dense MFMA peak is quoted at; bench.py reports both. */
int muvo_bf3_loop_clock(double* shader_mhz, double* us_per_k_step);
/* Last stage of VoxelDecoder1 fused (common.py:541-545 + VoxelSemHead :354-367): AdaIN of the last convolution's output x
 * (N,C,S) followed by the 1x1x1 class head (head_w (CO,C), head_b (CO)) -> logits (N,CO,S).  The normalised tensor is never
 * written; backward recomputes it and forms dy = head_w^T dlogits on the fly.  `moments`: the (sum, sum of squares) buffer of
 * muvo_conv_forward_moments (cleared).  muvo_adain_head_bwd: dx (N,C,S) (incl. the LeakyReLU derivative of the producing
 * convolution, as muvo_adain_bwd), dstyle (N,2C) overwritten, dhead_w / dhead_b accumulated; ws: 2*N*C doubles. */
int muvo_adain_head_supported(int C, int CO, int64_t S);
int muvo_adain_head_fwd(const float* x, const float* style, float* save_mean, float* save_rstd, double* moments, const float* head_w,
                        const float* head_b, float* logits, int N, int C, int CO, int64_t S, float eps, void* stream);
int muvo_adain_head_bwd(const float* x, const float* style, const float* save_mean, const float* save_rstd, const float* head_w,
                        const float* dlogits, float* dx, float* dstyle, float* dhead_w, float* dhead_b, double* ws, int N, int C,
                        int CO, int64_t S, int act, float slope, void* stream);
/* dx += conv_data_grad(dy, w) for the 1x1 output heads (muvo_conv_kernel_family(d, 1) == 3; RGBHead / LidarReHead / VoxelSemHead,
 * common.py:274-303,354-367): the head hangs off a decoder trunk, dx already holds the gradient that came back through the
 * trunk, so no separate add pass over the feature map is needed */
int muvo_conv_dgrad_accumulate(const muvo_conv_desc* d, const float* dy, const float* wp_dgrad, float* dx, void* stream);
/* backward preamble when muvo_conv_kernel_family(d, 1) == muvo_conv_kernel_family(d, 2) == 1: ws_dy <- split planes of
 * dy * act'(y) (y may be NULL with MUVO_ACT_NONE), dbias += its per-channel sums (dbias may be NULL) */
int muvo_conv_prepare_dy(const muvo_conv_desc* d, const float* y, const float* dy, int act, float slope, void* ws_dy,
                         float* dbias, void* stream);
/* The same preamble for a layer whose output also feeds a 1x1 head with CO <= 4 produced channels (RGBHead / LidarReHead behind the
 * transposed convolutions of ConvDecoder, common.py:608-632): planes of (dy + W_head^T dhead) * act'(y).  dy: gradient from the
 * trunk, NULL at the last stage (its output feeds the head only); dhead (N, CO, S); head_w (CO, Cout).  The head's data gradient
 * (a pass over all Cout channels of the feature map) is never written.  dhead_w (CO, Cout) / dhead_b (CO), optional and only with
 * an activation (y is then read by the pass anyway): the head's weight / bias gradient sum_pixels dhead * y, accumulated. */
int muvo_conv_prepare_dy_head_supported(const muvo_conv_desc* d, int CO);
int muvo_conv_prepare_dy_head(const muvo_conv_desc* d, const float* y, const float* dy, const float* dhead, const float* head_w,
                              int CO, int act, float slope, void* ws_dy, float* dbias, float* dhead_w, float* dhead_b, void* stream);
/* The operand layout of the bf16x3 kernels on its own: x (N,C,S) fp32 -> ws = [bf16 hi plane | bf16 lo plane] channels-last
 * (N,S,roundup(C,8)) (+ 16 zero bytes + scratch); optionally multiplied by act'(y) first and with per-channel sums added to
 * dbias (the backward preamble above without a descriptor).  ws: muvo_split_planes_bytes(N, C, S) bytes. */
int64_t muvo_split_planes_bytes(int N, int C, int64_t S);
int muvo_split_planes(const float* x, void* ws, int N, int C, int64_t S, const float* y, int act, float slope, float* dbias,
                      void* stream);
/* dw += conv_weight_grad(x, dy) (PyTorch layout); dbias += sum(dy) if non-NULL.
 * dwp_scratch: fwd_floats floats of workspace that must be ALL-ZERO on entry and is left all-zero on return (the split-K
 * partial sums accumulate in it with float atomics; the unpack pass clears what it reads, so no memset is needed per call).  ws_x / ws_dy: see muvo_conv_workspace_bytes (may be NULL
 * when 0 bytes); flags bit 0 / bit 1: ws_x / ws_dy already hold the copies written by muvo_conv_forward(x) /
 * muvo_conv_dgrad(dy) for the same tensors, so wgrad does not rewrite them. */
int muvo_conv_wgrad(const muvo_conv_desc* d, const float* x, const float* dy, float* dwp_scratch, float* dw, float* dbias,
                    void* ws_x, void* ws_dy, int flags, void* stream);

/* db[m] += sum_{n,s} dy[n][m][s] (bias gradient of any NCHW-like tensor) */
int muvo_bias_grad_nchw(const float* dy, float* db, int N, int M, int64_t S, void* stream);

/* ---- strided batched GEMM (gemm.hip) ------------------------------------------------------------
 * Replaces nn.Linear fwd/bwd (mile.py:151-161, transition.py, common.py:53-68,205-246), the matmuls of
 * nn.MultiheadAttention (mile.py:96-101) and ConvTranspose2d on a 1x1 input (common.py:578-581).
 * C[b1][b2][m][n] = act(alpha * sum_k A[m*sam + k*sak] * B[k*sbk + n*sbn] + bias[n / bias_div])
 * mode 1: C += alpha * A*B with float atomics (split-K; bias/act must be unset). */
typedef struct muvo_gemm_desc {
  int32_t M, N, K;
  int64_t sam, sak, sbk, sbn, scm;
  int32_t B1, B2;
  int64_t a_b1, a_b2, b_b1, b_b2, c_b1, c_b2;
  float alpha;
  int32_t bias_div;
  int32_t act;
  float slope;
  int32_t mode;
} muvo_gemm_desc;
int muvo_gemm(const muvo_gemm_desc* d, const float* A, const float* B, float* C, const float* bias, void* stream);
/* Routing query: what muvo_gemm would launch for this descriptor (host code only: nothing is launched, no device is needed).
 * A / B count only by their 16-byte alignment; has_bias as `bias != NULL` of the call.  The same MUVO_GEMM_KSPLIT_BLOCKS /
 * MUVO_GEMM_KSPLIT_MINTILES / MUVO_SKINNY_KS_BLOCKS values and the same deterministic mode as the launch itself.
 * kernel: MUVO_GEMM_TILED (fp32 MFMA tiles bm x bn, loaders a_lay / b_lay: 0 lanes along m / n, 1 lanes along k; ksplit K ranges,
 * grid (n tiles, m tiles, batches * ksplit)) or one of the skinny kernels (rm: row template; bm = bn = 0, a_lay = b_lay = -1;
 * ksplit: the KS of the n-contiguous kernel = grid[1], else 1). */
enum { MUVO_GEMM_TILED = 0, MUVO_GEMM_SKINNY_KVEC = 1, MUVO_GEMM_SKINNY_KCONTIG = 2, MUVO_GEMM_SKINNY_NCONTIG = 3 };
typedef struct muvo_gemm_route_info {
  int32_t kernel, rm, bm, bn, a_lay, b_lay, ksplit;
  int32_t grid[3];
  int32_t block;
} muvo_gemm_route_info;
int muvo_gemm_route(const muvo_gemm_desc* d, const float* A, const float* B, int has_bias, muvo_gemm_route_info* out);

/* ---- normalisation (norm.hip) --------------------------------------------------------------------
 * Train-mode BatchNorm2d (batch statistics over N*S, running stats momentum update, unbiased running
 * var) fused with ReLU and a residual add: res_mode 0 none, 1 add before ReLU (BasicBlock,
 * layers.py:48-66), 2 add after ReLU (DecoderDS, common.py:128).  ws: 2*C doubles of workspace. */
int muvo_bn_train_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                      float* save_mean, float* save_rstd, float* running_mean, float* running_var, double* ws, int N, int C,
                      int64_t S, float eps, float momentum, int res_mode, int relu, void* stream);
/* mask_mode 0: no ReLU; 1: ReLU mask from y > 0; 2: ReLU mask from bn(x) > 0 (residual added after the ReLU).
 * dgamma/dbeta are accumulated (+=). dres (may be NULL) receives the masked gradient for the residual branch. */
int muvo_bn_train_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* beta,
                      const float* save_mean, const float* save_rstd, float* dx, float* dres, float* dgamma, float* dbeta,
                      double* ws, int N, int C, int64_t S, int mask_mode, void* stream);
/* AdaptiveInstanceNorm3d (common.py:227-246): y = style[:, :C] * (x-mean)/sqrt(var+eps) + style[:, C:]
 * x_batch_stride = 0 broadcasts one (C,S) tensor over the batch (VoxelDecoder1.constant_tensor). ws: 2*N*C doubles. */
int muvo_adain_fwd(const float* x, const float* style, float* y, float* save_mean, float* save_rstd, double* ws, int N,
                   int C, int64_t S, int64_t x_batch_stride, float eps, void* stream);
/* act/slope: when x is the output of an activation (conv + LeakyReLU in ConvInstanceNorm3d, common.py:190-202) the
 * returned dx is already multiplied by that activation's derivative (MUVO_ACT_NONE: plain AdaIN gradient) */
int muvo_adain_bwd(const float* x, const float* style, const float* dy, const float* save_mean, const float* save_rstd,
                   float* dx, float* dstyle, double* ws, int N, int C, int64_t S, int64_t x_batch_stride, int act,
                   float slope, void* stream);
/* post-LN transformer sub-layer tail: z = x + dropout(a); y = LayerNorm(z) (nn.TransformerEncoderLayer, mile.py:96-101) */
int muvo_add_dropout_layernorm_fwd(const float* x, const float* a, const float* gamma, const float* beta, float* y,
                                   float* z, float* mean, float* rstd, int rows, int E, float eps, float p, uint64_t seed,
                                   void* stream);
int muvo_add_dropout_layernorm_bwd(const float* dy, const float* z, const float* mean, const float* rstd,
                                   const float* gamma, float* dx, float* da, float* dgamma, float* dbeta, int rows, int E,
                                   float p, uint64_t seed, void* stream);

/* ---- elementwise / layout / pooling / resampling (elementwise.hip) ------------------------------- */
int muvo_act_fwd(const float* x, float* y, int64_t n, int act, float slope, void* stream);
int muvo_act_bwd(const float* y, const float* dy, float* dx, int64_t n, int act, float slope, void* stream);
int muvo_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, void* stream);
int muvo_axpby(const float* a, const float* b, float* out, int64_t n, float alpha, float beta, void* stream);
int muvo_copy2d(const float* src, float* dst, int64_t rows, int64_t cols, int64_t ld_src, int64_t ld_dst, int accumulate,
                void* stream);
int muvo_colsum_acc(const float* x, float* out, int64_t rows, int64_t cols, int64_t ld, void* stream);
int muvo_batchsum(const float* x, float* out, int N, int64_t inner, int accumulate, void* stream);
/* tokens[(l0+l)][n][c] = x[n][c][l] + pos[c][l] + temb[c*temb_stride]  (mile.py:542-557) and its inverse (:560-561) */
int muvo_nchw_to_tokens(const float* x, const float* pos, const float* temb, int temb_stride, float* tokens, int N, int C,
                        int L, int l0, void* stream);
int muvo_tokens_to_nchw(const float* tokens, float* x, int N, int C, int L, int l0, void* stream);
/* F.max_pool2d 3x3 s2 p1 (ResNet stem) / 2x2 s2 (DecoderDS, common.py:127-128); idx: one byte per output = position a*k + b of
 * the (first) maximum inside its window, consumed by the backward pass */
int muvo_maxpool2d_fwd(const float* x, float* y, uint8_t* idx, int64_t NC, int H, int W, int OH, int OW, int k, int s, int p,
                       void* stream);
int muvo_maxpool2d_bwd(const float* dy, const uint8_t* idx, float* dx, int64_t NC, int H, int W, int OH, int OW, int k, int s,
                       int p, void* stream);
int muvo_avgpool_fwd(const float* x, float* y, int64_t G, int64_t S, void* stream);
int muvo_avgpool_bwd(const float* dy, float* dx, int64_t G, int64_t S, void* stream);
/* F.interpolate(scale_factor=2, mode='trilinear', align_corners=False) (common.py:169) */
int muvo_upsample3d_x2_fwd(const float* x, float* y, int64_t NC, int D, int H, int W, void* stream);
int muvo_upsample3d_x2_bwd(const float* dy, float* dx, int64_t NC, int D, int H, int W, void* stream);
/* Routing queries: what the pooling / upsample / softmax entry points would launch (host code only: nothing is launched, no
 * device is needed; the launchers launch from the same decision).  Pointers count only by their alignment.  A kernel that moves
 * 16 bytes per access of a pointer is chosen only when that pointer is 16-byte aligned.
 * muvo_upsample3d_route: in / out = x / y forward, dy / dx backward.  Three kernels per direction.  Forward: SCALAR, VEC (float4
 * stores of y) and ROW (float4 loads of x, 16-byte stores of y); backward: SCALAR, VEC and ROW (both: 16-byte loads of dy, 16- resp.
 * 8-byte stores of dx).  segs / dseg: the d segments of the backward ROW kernel and their length (1 / D otherwise). */
enum { MUVO_UPSAMPLE_SCALAR = 0, MUVO_UPSAMPLE_VEC = 1, MUVO_UPSAMPLE_ROW = 2 };
typedef struct muvo_upsample3d_route_info {
  int32_t kernel;
  int32_t grid[3], block[3];
  int32_t segs, dseg;
} muvo_upsample3d_route_info;
int muvo_upsample3d_route(int backward, int64_t NC, int D, int H, int W, const void* in, const void* out,
                          muvo_upsample3d_route_info* r);
/* muvo_maxpool2d_route: in / out = x / y forward, dy / dx backward.  k: the template instance (3: 3/2/1, 2: 2/2/0); load16: the
 * forward kernel reads x as aligned 16-byte pairs; v8: the backward is the eight-column 3x3 kernel (16-byte loads of dy, 4-byte
 * loads of idx, 16-byte stores of dx) instead of the generic one. */
typedef struct muvo_maxpool2d_route_info {
  int32_t k, load16, v8;
  int32_t grid[3], block[3];
} muvo_maxpool2d_route_info;
int muvo_maxpool2d_route(int backward, int64_t NC, int H, int W, int k, int s, int p, const void* in, const void* idx,
                         const void* out, muvo_maxpool2d_route_info* r);
/* the MAXV template instance (columns held per lane: 8 or 17) of muvo_softmax_dropout_fwd / _bwd; -1 for an invalid length */
int muvo_softmax_dropout_route(int cols);
/* PreProcess (muvo/models/preprocess.py:102-225): u8 -> /255 -> crop -> (label, ImageNet-normalised) */
int muvo_preprocess_image(const uint8_t* img, float* label, float* norm, int64_t NC, int C, int H, int W, int top, int left,
                          int CH, int CW, const float* mean3, const float* std3, void* stream);
int muvo_preprocess_route(const uint8_t* img, float* norm, int64_t NC, int C, int H, int W, int OH, int OW,
                          const float* mean3, const float* std3, void* stream);
/* Fused multi-head self-attention core of nn.TransformerEncoderLayer (muvo/models/mile.py:96-101,558), csrc/attention.hip, one
 * unit with two paths that share every tile step, the layouts, the exact-fp32 MFMA arithmetic and the dropout mask index, so one
 * seed gives one mask on either:
 * qkv (L, N, 3*H*DH) packed in-projection (q | k | v along the last axis, heads contiguous inside each), out (L, N, H*DH) =
 * dropout(softmax(q k^T / sqrt(DH))) v per (n, head), lse (N*H, L) row log-sum-exp saved for the backward pass; the L x L
 * matrices never reach HBM.  p / seed: attention-probability dropout, mask index ((n*H + h)*L + query)*L + key (same as
 * muvo_softmax_dropout_*).  Both backward entry points write all of dqkv (dq, dk, dv) - no atomics, no communication between
 * workgroups: bit-reproducible.
 * Resident path, muvo_attention_*: K and V of a head live whole in LDS.  muvo_attention_supported: DH in {16,32,48,64}, L <= 384
 * and 2 * roundup(L,16) * (DH+4) * 4 bytes (+ 8 * roundup(L,16)) <= 160 KB of LDS; otherwise use the streamed or the unfused
 * entry points. */
int muvo_attention_supported(int L, int DH);
int muvo_attention_fwd(const float* qkv, float* out, float* lse, int L, int N, int H, int DH, float p, uint64_t seed,
                       void* stream);
int muvo_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int L, int N, int H,
                       int DH, float p, uint64_t seed, void* stream);
/* Streamed path, muvo_attention_stream_*, any L >= 1: the same kernels with the keys (forward, dQ) or the queries (dK, dV)
 * passing through LDS in blocks of bk rows, the forward carries a running maximum and running sum per query (online softmax), a
 * workgroup owns bq rows.  muvo_attention_stream_supported: DH in {16,32,48,64}
 * and L >= 1.  muvo_attention_stream_blocks reports the compiled (bq, bk).  muvo_attention_stream_bwd takes a caller-allocated
 * workspace dws of N*H*L floats: the dQ kernel stores D = dout . out per query there and the dK/dV kernel, queued after it on
 * the same stream, reads it; the contents afterwards are D (nothing to keep). */
int muvo_attention_stream_supported(int L, int DH);
int muvo_attention_stream_blocks(int* bq, int* bk);
int muvo_attention_stream_fwd(const float* qkv, float* out, float* lse, int L, int N, int H, int DH, float p, uint64_t seed,
                              void* stream);
int muvo_attention_stream_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, float* dws,
                              int L, int N, int H, int DH, float p, uint64_t seed, void* stream);
/* Key-padding mask: the four entry points above with a mask at the end of the argument list; same kernels, same constraints per
 * path (resident: muvo_attention_supported; streamed: any L >= 1), same LDS.  key_mask (N, L) bytes, N the frame axis of qkv,
 * one row for all heads of a frame, mask_stride bytes from one row to the next; a non-zero byte means the key is ignored
 * (torch's src_key_padding_mask).  The kernels read it from global memory, a lane's four keys as one dword: key_mask and
 * mask_stride must be multiples of 4 and mask_stride >= roundup(L, 4) (bytes of a row beyond L are never looked at).
 * key_mask == NULL: no mask, the unmasked kernels run.
 *  - A masked key gets the score -inf BEFORE the row maximum is taken: it adds nothing to the sum, to lse, to out, to dq, and
 *    its own dk and dv rows are exactly 0.  Queries are never masked: a masked token still attends and gets its out row.
 *  - The dropout mask index stays ((n*H + h)*L + query)*L + key with L the full length: with p > 0 the live (query, key) pairs
 *    draw the bits they draw without a mask.
 *  - A frame (or a row) with NO live key is defined as out = 0, lse = -inf, dqkv = 0 and nothing non-finite but that lse
 *    (torch returns NaN there, which ends a training step); the backward never forms exp(s - lse) for a masked pair.
 *  - An all-zero mask gives the bits of the unmasked entry point; like those, every call is bit-reproducible. */
int muvo_attention_mask_fwd(const float* qkv, float* out, float* lse, int L, int N, int H, int DH, float p, uint64_t seed,
                            void* stream, const uint8_t* key_mask, int64_t mask_stride);
int muvo_attention_mask_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int L, int N,
                            int H, int DH, float p, uint64_t seed, void* stream, const uint8_t* key_mask, int64_t mask_stride);
int muvo_attention_stream_mask_fwd(const float* qkv, float* out, float* lse, int L, int N, int H, int DH, float p, uint64_t seed,
                                   void* stream, const uint8_t* key_mask, int64_t mask_stride);
int muvo_attention_stream_mask_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                   float* dws, int L, int N, int H, int DH, float p, uint64_t seed, void* stream,
                                   const uint8_t* key_mask, int64_t mask_stride);
/* The whole recurrent state-space model (muvo/models/transition.py:76-173) as two persistent kernels (csrc/rssm.hip): one
 * workgroup per CU walks the T time steps, 4 grid barriers per step; T <= 64, H/S/E/A multiples of 4; B <= 64 sequences, run as
 * consecutive launches over slabs of 4 (sequences are independent).  The grid is clamped to what the occupancy calculator says
 * is co-resident; a barrier spin that still times out (2 s) raises the sticky word barrier_word[1] and ends the kernel.
 * weights[18] (PyTorch [out][in] layouts): pre_gru_net.0.{weight,bias}, recurrent_model.{weight_ih,weight_hh,bias_ih,bias_hh},
 *   prior_action_module.0.{weight,bias}, posterior_action_module.0.{weight,bias}, prior.module.0.{weight,bias},
 *   prior.module.2.{weight,bias}, posterior.module.0.{weight,bias}, posterior.module.2.{weight,bias}.
 * emb (B,T,E), act (B,T,AD), noise (B,T,2,S) [prior, posterior draws]; use_prior_mask bit t: step t+1 continues from the PRIOR
 *   sample of step t (transition.py:118-124), else from the posterior sample.
 * out7 (B,T,.): hidden state h (H) — shared by the prior and posterior dicts —, prior mu, sigma, sample, posterior mu, sigma,
 *   sample (S).  keep12 (B,T,.), written for the backward pass: h_prev (H), z_prev (S), a_prev (AD), u (H), gi (3H), gh (3H),
 *   x_prior (H+A), x_post (H+E+A), y1_prior (H+A), y1_post (H+E+A), mls_prior (2S), mls_post (2S).
 * muvo_rssm_backward: kept5 = {h_prev, gi, gh, mls_prior, mls_post}; upstream7 = gradients of out7 (NULL = none);
 *   grads10 (B,T,.) written: d_emb (E), dmls_prior, dmls_post (2S), dy1_prior (H+A), dy1_post (H+E+A), dgi, dgh (3H), du (H),
 *   dla_prior, dla_post (A) — the weight gradients are dW = dY^T X over the B*T rows (caller: one skinny GEMM per weight):
 *   W_post2: dmls_post x y1_post; W_post0: dy1_post x x_post; W_prior2: dmls_prior x y1_prior; W_prior0: dy1_prior x x_prior;
 *   W_ih: dgi x u; W_hh: dgh x h_prev; W_pre: du x z_prev; action modules: dla x a_prev; biases: column sums of the dY.
 *   wt_scratch: muvo_rssm_transposed_floats() floats (the transposed weights are rebuilt by every call); scratch:
 *   muvo_rssm_scratch_floats() floats; barrier_word: four 32-bit words of device memory (ops.rssm_barrier_words), zero
 *   before the first call: [0] the barrier counter (reset by every launch), [1] the sticky time-out flag (the caller polls
 *   it: ops.rssm_check); the kernels touch no other word.  csrc/rssm.hip names the entries of every table in these orders. */
int muvo_rssm_supported(int B, int T, int H, int S, int E, int A, int AD);
int64_t muvo_rssm_transposed_floats(int H, int S, int E, int A);
int64_t muvo_rssm_scratch_floats(int B, int H, int S, int E, int A);
int muvo_rssm_forward(int B, int T, int H, int S, int E, int A, int AD, const float* const* weights, const float* emb,
                      const float* act, const float* noise, uint64_t use_prior_mask, float* const* out7, float* const* keep12,
                      uint32_t* barrier_word, float min_std, void* stream);
int muvo_rssm_backward(int B, int T, int H, int S, int E, int A, int AD, const float* const* weights, float* wt_scratch,
                       const float* noise, uint64_t use_prior_mask, const float* const* kept5, const float* const* upstream7,
                       float* const* grads10, float* scratch, uint32_t* barrier_word, void* stream);
/* Training-time augmentation inside PreProcess.forward (muvo/models/preprocess.py:45-48,213-214; PixelAugmentation :295-333,
 * RouteAugmentation :336-367; torchvision 0.15.2 tensor algorithms).  The random draws are explicit inputs.
 * muvo_pixel_augment: img (F,3,H,W) in [0,1] (the cropped image = rgb_label_1) is augmented IN PLACE, norm (F,3,H,W) receives
 *   the ImageNet-normalised result; frames whose row says "nothing" are left untouched in both.  params: F rows of
 *   MUVO_PIXAUG_STRIDE floats: [0] 0 none / 1 gaussian blur 5x5 / 2 sharpen, [1] sigma | sharpness factor, [2] colour jitter
 *   on (0/1), [3..6] order of the colour ops (0 brightness, 1 contrast, 2 saturation, 3 hue), [7..10] their factors.
 *   tmp: F*3*H*W floats, gray_sum: F doubles (scratch).
 * muvo_preprocess_route_aug: muvo_preprocess_route + RouteAugmentation of sample b (all S frames alike); params (may be
 *   NULL): B rows of MUVO_ROUTEAUG_STRIDE floats: [0] 0 none / 1 drop / 2 end of route / 3 affine, [1] rows zeroed (mode 2),
 *   [2..7] torchvision's inverse affine matrix (_get_inverse_affine_matrix, center (0,0)). */
#define MUVO_PIXAUG_STRIDE 16
#define MUVO_ROUTEAUG_STRIDE 8
int muvo_pixel_augment(float* img, float* norm, float* tmp, const float* params, double* gray_sum, int64_t frames, int H, int W,
                       const float* mean3, const float* std3, void* stream);
int muvo_preprocess_route_aug(const uint8_t* img, float* out, const float* params, int B, int S, int C, int H, int W, int OH,
                              int OW, const float* mean3, const float* std3, void* stream);
int muvo_divide_scalar(const float* x, float* y, int64_t n, float divisor, void* stream);
int muvo_resize_bilinear(const float* x, float* y, int64_t NC, int H, int W, int OH, int OW, void* stream);
int muvo_resize_nearest_f32(const float* x, float* y, int64_t NC, int D, int H, int W, int OD, int OH, int OW, void* stream);
int muvo_resize_nearest_u8(const uint8_t* x, uint8_t* y, int64_t NC, int D, int H, int W, int OD, int OH, int OW,
                           void* stream);
/* attention probabilities: P = softmax(S), Pd = dropout(P) (functional MHA dropout); cols <= 1088 */
int muvo_softmax_dropout_fwd(const float* S, float* P, float* Pd, int64_t rows, int cols, float p, uint64_t seed, void* stream);
int muvo_softmax_dropout_bwd(const float* P, const float* dPd, float* dS, int64_t rows, int cols, float p, uint64_t seed,
                             void* stream);
/* nn.GRUCell pointwise part and RepresentationModel sampling (muvo/models/transition.py:18-24,49-52,176-181) */
int muvo_gru_fwd(const float* gi, const float* gh, const float* h, float* hnew, int B, int H, void* stream);
int muvo_gru_bwd(const float* gi, const float* gh, const float* h, const float* dhnew, float* dgi, float* dgh, float* dh,
                 int B, int H, void* stream);
int muvo_rssm_sample_fwd(const float* mu_logsigma, const float* eps, int64_t eps_ld, float* mu, float* sigma, float* sample,
                         int B, int S, float min_std, void* stream);
int muvo_rssm_sample_bwd(const float* mu_logsigma, const float* eps, int64_t eps_ld, const float* dmu, const float* dsigma,
                         const float* dsample, float* dmls, int B, int S, void* stream);

/* ---- losses + optimiser (losses.hip): muvo/losses.py:53-287, muvo/trainer.py:251-390,1022-1060 ------ */
/* SpatialRegressionLoss over channels [c0,c1) of (F,Ct,HW) tensors; loss = weight * masked mean; stats2: 2 doubles */
int muvo_spatial_loss_fwd(const float* pred, const float* target, int64_t F, int Ct, int64_t HW, int c0, int c1, int norm,
                          float ignore, float weight, double* stats2, float* loss, void* stream);
int muvo_spatial_loss_bwd(const float* pred, const float* target, float* dpred, int64_t F, int Ct, int64_t HW, int c0, int c1,
                          int norm, float ignore, float weight, const double* stats2, const float* gout, void* stream);
/* the same with an explicit pixel mask (F, HW) uint8 instead of `target[:, c0] != ignore` (instance_mask argument of
 * SpatialRegressionLoss.forward, muvo/losses.py:87-90: LOSSES.RGB_INSTANCE, muvo/trainer.py:303-321); mask NULL = the plain form */
int muvo_spatial_loss_masked_fwd(const float* pred, const float* target, const uint8_t* mask, int64_t F, int Ct, int64_t HW, int c0,
                                 int c1, int norm, float ignore, float weight, double* stats2, float* loss, void* stream);
int muvo_spatial_loss_masked_bwd(const float* pred, const float* target, const uint8_t* mask, float* dpred, int64_t F, int Ct,
                                 int64_t HW, int c0, int c1, int norm, float ignore, float weight, const double* stats2,
                                 const float* gout, void* stream);
/* VoxelLoss (CE mean) + SemScalLoss + GeoScalLoss in one pass; loss3 = {ce, sem_scal, geo_scal} * weight */
int muvo_voxel_loss_stats_doubles(int C);
int muvo_voxel_loss_coef_floats(int C);
int muvo_voxel_loss_fwd(const float* logits, const uint8_t* target, int64_t F, int C, int64_t V, const float* class_w,
                        float weight, double* stats, float* coef, float* loss3, void* stream);
int muvo_voxel_loss_bwd(const float* logits, const uint8_t* target, float* dlogits, int64_t F, int C, int64_t V,
                        const float* class_w, float weight, const float* coef, const float* gout3, void* stream);
/* per-pixel class-weighted cross entropy of SegmentationLoss (muvo/losses.py:22-37, F.cross_entropy(reduction='none')):
 * logits (N,C,HW), target (N,HW) bytes, class_w C floats or NULL, loss / gloss (N,HW); the top-k / mean reduction stays with
 * the caller (losses.py:44-50) */
int muvo_seg_ce_fwd(const float* logits, const uint8_t* target, const float* class_w, float* loss, int64_t N, int C, int64_t HW,
                    void* stream);
int muvo_seg_ce_bwd(const float* logits, const uint8_t* target, const float* class_w, const float* gloss, float* dlogits, int64_t N,
                    int C, int64_t HW, void* stream);
int muvo_l1_rows_fwd(const float* p, const float* t, int64_t rows, int cols, float weight, float* loss, void* stream);
int muvo_l1_rows_bwd(const float* p, const float* t, float* dp, int64_t rows, int cols, float weight, const float* gout,
                     void* stream);
int muvo_kl_loss_fwd(const float* prior_mu, const float* prior_sigma, const float* post_mu, const float* post_sigma, int B,
                     int T, int S, float weight, float* loss, void* stream);
int muvo_kl_loss_bwd(const float* prior_mu, const float* prior_sigma, const float* post_mu, const float* post_sigma,
                     float* d_prior_mu, float* d_prior_sigma, float* d_post_mu, float* d_post_sigma, int B, int T, int S,
                     float weight, float alpha, const float* gout, void* stream);
/* torch.optim.AdamW step over a flat parameter segment; grad_scale multiplies g (1/world_size after a sum all-reduce) */
int muvo_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int step, float grad_scale, void* stream);

/* ---- Chamfer-distance training loss (chamfer.hip): CDLoss, muvo/losses.py:352-367 with reducer = mean -----------------------
 * pred (F,Cp,n), target (F,Ct,n) channel-planar fp32; x, y, z are planes 0, 1, 2 and further planes are never read.
 * loss[0] = weight * mean_f ( mean_j min_i |p_i - t_j| + mean_i min_j |p_i - t_j| ).  The nearest neighbour is chosen by the
 * fp32 squared distance of the coordinate differences, the lowest index wins a tie, the square root is taken for the winner.
 * ws: muvo_chamfer_loss_ws_doubles(F, n) doubles of scratch (written, then read; no need to clear).  idx_pt / idx_tp: (F,n)
 * int32 each - idx_pt[f,i] = the target nearest to prediction point i, idx_tp[f,j] = the prediction point nearest to target
 * j - or both NULL when no backward follows (the loss value is bit-identical either way).
 * Backward: dpred (F,Cp,n) is written completely, planes >= 3 with zeros; d|a - b| = (a - b)/|a - b| and exactly 0 where the
 * two points coincide; gout = the upstream gradient of the scalar, on the device.  The mean_j min_i term is a scatter into the
 * selected prediction points (fp32 atomics, equal destinations of a wave combined first); in deterministic mode every
 * prediction point sums its senders in index order instead and the result is bit-reproducible.  F <= 65535, n <= 2^30. */
int64_t muvo_chamfer_loss_ws_doubles(int64_t F, int64_t n);
int muvo_chamfer_loss_fwd(const float* pred, const float* target, int64_t F, int Cp, int Ct, int64_t n, float weight, double* ws,
                          int32_t* idx_pt, int32_t* idx_tp, float* loss, void* stream);
int muvo_chamfer_loss_bwd(const float* pred, const float* target, const int32_t* idx_pt, const int32_t* idx_tp, float* dpred, int64_t F,
                          int Cp, int Ct, int64_t n, float weight, const float* gout, void* stream);

/* ---- Lovasz-softmax training loss of the voxel head (lovasz.hip; an extension) -----------------------
 * logits (F,C,V) fp32, labels (F,V) bytes, 2 <= C <= 16, F*C <= 65535, V <= 2^30.  A voxel with label >= C is ignored: absent
 * from the ranking, gradient exactly 0.  Per frame f and class c: e_v = |[label_v == c] - softmax(logits_v)_c|, ranked descending
 * with ties by ascending voxel index (a stable segmented radix sort on the device), L_fc = sum_i e_(i) g_i with g_i the increment
 * of the Jaccard loss at rank i in its closed form (fp64).  loss[0] = weight / F * sum_f (sum_{c present in f} L_fc) /
 * max(1, #present_f); class c is present in frame f iff one valid voxel of f has label c.
 * ws: muvo_lovasz_ws_bytes(F, C, V) bytes of 16-byte aligned scratch (written, then read; no need to clear); after the call its
 * first F*C doubles hold L_fc.  errors (F,C,V): e, 0 at ignored voxels, or NULL.  dlde (F,C,V): g at the voxel's rank - 0 at
 * ignored voxels and for absent classes, not scaled by weight, 1/F or 1/#present - or NULL when no backward follows.  present
 * (F,C) bytes.  The loss value is bit-identical with and without the optional outputs; no float atomics: every call on the same
 * inputs gives the same bits.
 * Backward: the ranking is fixed; dlogits (F,C,V) is written completely (zeros at ignored voxels) from dlde, the sign of
 * de/dp (-1 foreground, +1 background) and the softmax Jacobian; gout = the upstream gradient of the scalar, on the device. */
int64_t muvo_lovasz_ws_bytes(int64_t F, int C, int64_t V);
int muvo_lovasz_fwd(const float* logits, const uint8_t* labels, int64_t F, int C, int64_t V, float weight, void* ws, float* errors,
                    float* dlde, uint8_t* present, float* loss, void* stream);
int muvo_lovasz_bwd(const float* logits, const uint8_t* labels, const float* dlde, const uint8_t* present, float* dlogits, int64_t F, int C,
                    int64_t V, float weight, const float* gout, void* stream);

/* ---- evaluation metrics of the validation path (muvo/metrics.py via muvo/trainer.py:426-490) ----------------------------
 * All accumulators are caller-zeroed device buffers the kernels ADD into (several batches may share them).
 * muvo_ssim_frames: sums[n] += sum over (c, y, x) of the SSIM map of frame n (valid 11x11 Gaussian window given as 121
 *   floats, losses.py:304-314); mean = sums / (C (H-10) (W-10)).  Replaces SSIMLoss._ssim, losses.py:316-339.
 * muvo_sqdiff_frames: sums[n] += sum (pred - target)^2 over the L elements of frame n (PSNRMetric.psnr, metrics.py:305-309).
 * muvo_chamfer_sums: sums[2n] += sum_i min_j |a_i - b_j|, sums[2n+1] += sum_j min_i |a_i - b_j| for point sets a (N,P,3),
 *   b (N,Q,3) (CDMetric.add_batch, metrics.py:243-249).
 * muvo_ssc_counts: prediction = argmax over the C logits (N,C,V); counts[0..2] += completion tp/fp/fn, counts[3+3j..] +=
 *   tp/fp/fn of class j over voxels with label != 255 (trainer.py:482-490, SSCMetrics.add_batch, metrics.py:77-100).
 * muvo_seg_confusion: the confusion matrix behind the bird's-eye-view, lidar and camera IoU (torchmetrics.JaccardIndex as fed
 *   by trainer.py:427-478).  logits (F,C,P) float32, label (F,P) bytes, 2 <= C <= 16; counts is uint64[C*C + 1]:
 *   counts[t*C + p] += pixels with label t and prediction p = first maximum over the C planes (strict >, torch.argmax on
 *   finite input; NaN logits are outside the contract), counts[C*C] += pixels with label >= C, which reach no other bin.
 *   One launch, no host read: the matrix stays on the device until the caller reads it.
 * muvo_seg_confusion_index: the same from n already arg-maxed byte predictions; a prediction >= C also goes to counts[C*C]. */
int muvo_ssim_frames(const float* pred, const float* target, const float* window, double* sums, int N, int C, int H, int W,
                     float c1, float c2, void* stream);
/* SSIM as a training loss (LOSSES.SSIM: trainer.py:312-318, SSIMLoss losses.py:292-348): muvo_ssim_maps = muvo_ssim_frames plus
 * the derivative maps dA, dB, dC (N*C*(H-10)*(W-10) floats each) of every SSIM value w.r.t. the prediction's window mean,
 * E[p^2] and E[p t]; muvo_ssim_bwd: dpred = scale * adjoint window pass (scale = upstream gradient / number of SSIM values) */
int muvo_ssim_maps(const float* pred, const float* target, const float* window, double* sums, float* dA, float* dB, float* dC, int N,
                   int C, int H, int W, float c1, float c2, void* stream);
int muvo_ssim_bwd(const float* pred, const float* target, const float* window, const float* dA, const float* dB, const float* dC,
                  float* dpred, int N, int C, int H, int W, float scale, void* stream);
int muvo_sqdiff_frames(const float* pred, const float* target, double* sums, int N, int64_t L, void* stream);
int muvo_chamfer_sums(const float* a, const float* b, double* sums, int N, int P, int Q, void* stream);
int muvo_ssc_counts(const float* logits, const uint8_t* label, uint64_t* counts, int64_t F, int C, int64_t V, void* stream);
int muvo_seg_confusion(const float* logits, const uint8_t* label, uint64_t* counts, int64_t F, int C, int64_t P, void* stream);
int muvo_seg_confusion_index(const uint8_t* pred, const uint8_t* label, uint64_t* counts, int64_t n, int C, void* stream);

/* ---- BEV lifting: FrustumPooling (muvo/models/frustum_pooling.py:67-217) as called from Mile.encode (mile.py:506-522) ----
 * muvo_frustum_cells: cells[b][d][h][w] = (iz*ny + iy)*nx + ix of the frustum point, -1 outside the grid (get_geometry
 *   :108-128 + the index part of voxel_pooling :139-158).  combine = R K^-1 per frame (3x3 row major), trans = camera position,
 *   xs/ys/ds = pixel columns, rows and depth bin centres of the frustum (:92-106); sx, ox, sy, oy = BEV intrinsics
 *   (geometry_utils.py:8-19), bz/dz = first cell centre and cell size along "up" (gen_dx_bx :10-21).
 * muvo_frustum_pool_fwd: out[b][c*nz + iz][iy][ix] = sum over the lifted points of the cell of depth[b][d][p] * feat[b][c][p]
 *   (outer product mile.py:519 + voxel_pooling :130-182).  mask: (B,D,HW) bytes, non-zero = lift (NULL = all, mile.py:511-518).
 *   acc: B*ncell*C floats of scratch (channels-last accumulator).  Valid for nz = 1 or any nz (out is (B, C, ncell) with the
 *   up index inside the cell number; the caller reorders for nz > 1).
 * muvo_frustum_pool_bwd: gradients of the above w.r.t. feat and depth (QuickCumsum.backward :56-64 chained through the outer
 *   product); g_cl: B*ncell*C floats of scratch.  Deterministic (no atomics).
 * muvo_depth_expectation: e[b][p] = sum_d ds[d] depth[b][d][p] (get_depth_map :211-214). */
int muvo_frustum_cells(const float* combine, const float* trans, const float* xs, const float* ys, const float* ds, int32_t* cells,
                       int B, int D, int H, int W, float sx, float ox, float sy, float oy, float bz, float dz, int nx, int ny,
                       int nz, void* stream);
int muvo_frustum_pool_fwd(const float* feat, const float* depth, const uint8_t* mask, const int32_t* cells, float* acc, float* out,
                          int B, int C, int D, int64_t HW, int ncell, void* stream);
int muvo_frustum_pool_bwd(const float* feat, const float* depth, const uint8_t* mask, const int32_t* cells, const float* gout,
                          float* g_cl, float* dfeat, float* ddepth, int B, int C, int D, int64_t HW, int ncell, void* stream);
int muvo_depth_expectation(const float* depth, const float* ds, float* e, int B, int D, int64_t HW, void* stream);
/* adjoint of muvo_resize_bilinear (backward of F.interpolate(..., 'bilinear', align_corners=False) in `Decoder`, common.py:96) */
int muvo_resize_bilinear_bwd(const float* dy, float* dx, int64_t NC, int H, int W, int OH, int OW, void* stream);
/* softmax over the channel dimension of (B, C, HW): depth distribution of the mono depth head (mile.py:509) */
int muvo_softmax_channel_fwd(const float* x, float* y, int B, int C, int64_t HW, void* stream);
int muvo_softmax_channel_bwd(const float* y, const float* dy, float* dx, int B, int C, int64_t HW, void* stream);

/* ---- input pipeline on the device: per-frame work of CarlaDataset.load_single_element_time_t (muvo/data/dataset.py:275-327) ----
 * muvo_range_projection: raw lidar sweep (P,3) float32 in the sensor frame + CARLA object tags -> range_view_pcd_xyzd (4,H,W)
 *   float32 (x, y, z in the ego frame, depth; empty pixels 0,0,0,-1) and optionally the label image (H,W): convert_coor_lidar
 *   (data/data_preprocessing.py:119-122), label remap and ego-box masking (dataset.py:281-290), PointCloud.do_range_projection
 *   (muvo/utils/geometry_utils.py:176-213; float64 geometry, the closest point of a pixel wins, exact ties: lowest index).
 *   remap: 256-entry table; ego_dim: EGO_VEHICLE_DIMENSION (constants.py:8); scratch: 12*H*W bytes.
 * muvo_voxel_grid: sparse voxel rows (Q,4) int64 (x, y, z, tag) -> dense uint8 grid (dataset.py:316-327: tag 255 -> 0, remap,
 *   later rows win); scratch: 4*X*Y*Z bytes. */
int muvo_range_projection(const float* points_xyz, const uint8_t* obj_tag, const uint8_t* remap, int64_t P, const double* lidar_pos,
                          const double* ego_dim, double fov_down_deg, double fov_up_deg, int H, int W, void* scratch,
                          float* xyzd, uint8_t* seg, void* stream);
int muvo_voxel_grid(const int64_t* rows, int64_t Q, const uint8_t* remap, int X, int Y, int Z, uint32_t* scratch, uint8_t* voxels,
                    void* stream);
/* ---- dataset frame preparation, batched over the F = b*s frames of a batch (csrc/dataset.hip; muvo/data/dataset.py:231-369) ----
 * The host reads and decodes the files of a recording; these entry points turn the raw frames into the batch dict.  Frames are
 * a grid dimension: one call per batch, no host loop over frames, no host sync.  Every output is bit-exact (integer work, or
 * float64 in the reference's order of operations).
 * muvo_birdview_decode_frames: integer bird's-eye view (F,H,W) int32 -> bit planes birdview (F,n_classes,H,W) float32
 *   (integer_to_binary), label (F,H,W) int64 = highest set bit, n_classes-1 where none is set (calculate_birdview_labels), and
 *   instance_mask (F,H,W) uint8 = bit 3 | bit 4 (dataset.py:266).
 * muvo_label_components_frames: scipy.ndimage.label of each (1,H,W) mask with the default structure (4-connectivity in the
 *   plane): labels (F,H,W) int32, components numbered 1, 2, ... by their first pixel in row-major order, background 0.  Union-find
 *   by smallest linear index in 32x32 LDS tiles, borders merged with atomicMin, flattened, roots numbered by a scan; every loop
 *   is bounded by the pixel count (csrc/dataset.hip).  Any H, W with H*W < 2^30.  scratch: 2*F*H*W int32.
 * muvo_depth_semantic_decode_frames: RGBA (F,H,W,4) uint8 -> semantic_image (F,H,W) int64 = remap[A], image_instance_mask (F,H,W)
 *   uint8 = A == vehicle_tag | A == pedestrian_tag, depth_color (F,3,H,W) float64 = RGB / 255.0, depth (F,H,W) float64 =
 *   (65536 R + 256 G + B) / (256^3 - 1), values > 0.999 -> -1 (dataset.py:330-352).  Each output may be NULL (not all).
 * muvo_range_projection_frames / muvo_voxel_grid_frames: muvo_range_projection / muvo_voxel_grid over padded arrays
 *   points_xyz (F,Pmax,3), obj_tag (F,Pmax), rows (F,Qmax,4) with per-frame counts num_points / num_rows (F) int32 on the device
 *   (clamped to the padding); xyzd (F,4,H,W), seg (F,H,W) int64 or NULL, voxels (F,X,Y,Z).  scratch: 12*F*H*W bytes /
 *   4*F*X*Y*Z bytes.  Same device functions, same results frame by frame. */
int muvo_birdview_decode_frames(const int32_t* birdview_int, int F, int H, int W, int n_classes, float* birdview, int64_t* label,
                                uint8_t* instance_mask, void* stream);
int muvo_label_components_frames(const uint8_t* mask, int F, int H, int W, int32_t* scratch, int32_t* labels, void* stream);
int muvo_depth_semantic_decode_frames(const uint8_t* depth_semantic, int F, int H, int W, const uint8_t* remap, int vehicle_tag,
                                      int pedestrian_tag, int64_t* semantic_image, uint8_t* image_instance_mask, double* depth_color,
                                      double* depth, void* stream);
int muvo_range_projection_frames(const float* points_xyz, const uint8_t* obj_tag, const int32_t* num_points, const uint8_t* remap, int F,
                                 int64_t Pmax, const double* lidar_pos, const double* ego_dim, double fov_down_deg, double fov_up_deg,
                                 int H, int W, void* scratch, float* xyzd, int64_t* seg, void* stream);
int muvo_voxel_grid_frames(const int64_t* rows, const int32_t* num_rows, const uint8_t* remap, int F, int64_t Qmax, int X, int Y, int Z,
                           uint32_t* scratch, uint8_t* voxels, void* stream);
/* ---- voxel labels from raw sensor data: the reference's offline step data/generate_voxels.py::voxelize_one ->
 * data/data_preprocessing.py::merge_pcd + voxel_filter, for F frames per call ----
 * depth_semantic (F,H,W,4) uint8: R, G, B = 24-bit depth code, A = CARLA tag; points_xyz (F,Pmax,3) float32 in the lidar sensor
 * frame, obj_tag (F,Pmax) uint8, num_points (F) int32 or NULL (= Pmax everywhere; rows beyond num_points[f] are never read).
 * Camera pixels are unprojected (depth < 1000, camera-frame range < max_range) and moved to the ego frame, lidar points by
 * convert_coor_lidar; points inside the ego-vehicle box are dropped (mask_ego); b = p + off must lie in [0, hi) on every axis;
 * np.divmod(b, res) gives voxel and remainder; every occupied voxel takes the raw tag of the point with the smallest squared
 * remainder (exact ties: the lowest global index, camera pixels row-major first, lidar points after them), or 6 if any of its
 * points has tag 6 (road line).  All geometry in float64, operation by operation as the reference; integer atomics only, so the
 * result is independent of the execution order.
 * Outputs (either may be NULL, not both):
 *   rows (F,cap,4) int64 x, y, z, tag ascending in x + y*Dx + z*Dx*Dy, counts (F) int32 = rows written per frame
 *     (cap >= min(H*W + Pmax, Dx*Dy*Dz) holds every possible result);
 *   dense (F,Dx,Dy,Dz) uint8 = remap[tag == 255 ? 0 : tag], 0 where empty: what muvo_voxel_grid makes of the rows.
 * scratch: muvo_voxelize_scratch_bytes(F, Dx, Dy, Dz) bytes (15 per voxel and frame; -1 for sizes the entry refuses). */
typedef struct muvo_voxelize_geom {
  double cam[3];      /* float32(forward), float32(-right), float32(up) of the camera position, widened (convert_coor_img) */
  double lidar[3];    /* lidar position forward, right, up */
  double f, cx, cy;   /* W / (2 tan(fov pi / 360)), W / 2, H / 2 */
  double max_range;
  double ego_lo[3], ego_hi[3];
  double off[3];      /* offset + res * size / 2 */
  double hi[3];       /* size * res */
  double res;
  int32_t mask_ego, H, W, Dx, Dy, Dz;
} muvo_voxelize_geom;
int64_t muvo_voxelize_scratch_bytes(int F, int Dx, int Dy, int Dz);
int muvo_voxelize_frames(const uint8_t* depth_semantic, const float* points_xyz, const uint8_t* obj_tag, const int32_t* num_points, int F,
                         int64_t Pmax, const muvo_voxelize_geom* geom, const uint8_t* remap, void* scratch, int64_t* rows, int64_t cap,
                         int32_t* counts, uint8_t* dense, void* stream);
/* convert_instance_mask_to_center_and_offset_label (muvo/utils/instance_utils.py:4-35, called from
 * PreProcess.prepare_bev_labels, preprocess.py:68-100): instance ids (F,H,W) uint8 (0 = background) -> centre heat map
 * center (F,H,W) = max over the instances of the frame of exp(-d^2 / sigma^2) around the rounded centroid, and offset (F,2,H,W)
 * = centroid - pixel (rows, then columns) on instance pixels, `ignore` elsewhere.  scratch: F*256*3 doubles. */
int muvo_instance_labels(const uint8_t* instance, int64_t F, int H, int W, float sigma, float ignore, double* scratch, float* center,
                         float* offset, void* stream);

/* ---- measurement aid for the data-parallel path on ONE GPU (muvo_amd/parallel.py: SegmentedGradReducer(fake_peers=G)) ----
 * Lightning's implicit DDP (train.py:93-98) all-reduces the gradients; on a one-GPU box a one-rank RCCL all-reduce is a no-op, so
 * nothing ever ran beside the big-LDS convolution tiles and the persistent recurrent kernels.  muvo_fake_allreduce stands in for
 * the collective's LOCAL footprint: `workgroups` resident workgroups of 256 threads (RCCL's channels) walk buf (n floats, n % 4 == 0,
 * 16-byte aligned), read every element twice (own copy + "received" copy: two uncached loads), write 0.5 * (a + b) - bit-identical
 * to the input, so parity is unchanged - and sleep `sleep` x 64 clocks per 16-KB round, which sets the rate (calibrated by the
 * caller to the xGMI ring's ~1 ms per 100 MB).  The loop has a fixed trip count: every wave terminates. */
int muvo_fake_allreduce(float* buf, int64_t n, int workgroups, int sleep, void* stream);

/* antialiased linear resize of (NC, H, W) float planes: EVAL.RESOLUTION of PreProcess.forward (muvo/models/preprocess.py:209-210,
 * functional_resize_batch :252-273: torchvision 0.15.2 `resize(image, size, antialias=True)`, i.e. ATen's _upsample_bilinear2d_aa -
 * per axis the triangle filter of width in/out around scale * (i + 0.5), weights normalised, horizontal pass first).  ynorm (may be
 * NULL): (y - mean[c]) / std[c] with c = plane index % C (the ImageNet normalisation that follows, preprocess.py:217; host arrays). */
int muvo_resize_bilinear_aa(const float* x, float* y, float* ynorm, const float* mean, const float* std, int64_t NC, int C, int H,
                            int W, int OH, int OW, void* stream);

/* ---- BatchNorm that writes its consumer's operand format (round 4; muvo/layers/layers.py:9-66, muvo/models/common.py:102-130, timm
 * ResNet-18: conv -> BatchNorm2d (train mode) -> ReLU -> conv) ----
 * muvo_bn_train_fwd_planes = muvo_bn_train_fwd that ALSO stores the channels-last bf16 hi / lo planes of its result into `planes`
 * (muvo_split_planes_bytes(N, C, S) bytes: what the bf16x3 convolution kernels read, otherwise made by a separate split pass over
 * y); y may be NULL when the planes are the only thing the consumers need.  muvo_bn_train_bwd_planes = muvo_bn_train_bwd whose dx
 * goes out as planes (dx may be NULL): the operand of the data- and weight-gradient kernels of the convolution that produced x
 * (muvo_conv_dgrad with ws_valid, muvo_conv_wgrad with flag 2) - muvo_conv_prepare_dy is not needed.  Same arithmetic per element
 * as the unfused kernels (bit-identical results).  muvo_conv_forward_planes: muvo_conv_forward with ws_valid (x may be NULL then). */
int muvo_bn_train_fwd_planes(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                             float* save_mean, float* save_rstd, float* running_mean, float* running_var, int N, int C,
                             int64_t S, float eps, float momentum, int res_mode, int relu, void* planes, void* stream);
int muvo_bn_train_bwd_planes(const float* x, const float* y, const float* dy, const float* gamma, const float* beta,
                             const float* save_mean, const float* save_rstd, float* dx, float* dres, float* dgamma,
                             float* dbeta, int N, int C, int64_t S, int mask_mode, void* planes, void* stream);
int muvo_conv_forward_planes(const muvo_conv_desc* d, const float* x, const float* wp_fwd, const float* bias, float* y, int act,
                             float slope, void* ws, int ws_valid, void* stream);

/* ---- ResNet-18 stem (timm resnet18 conv1: Conv2d(3 | 4, 64, 7, stride 2, padding 3, bias=False); muvo/models/mile.py:24,81) as a direct
 * convolution on bf16x3 split products (csrc/conv_stem.hip): the input patch of an output tile in LDS, operands built from it without
 * a gather.  w / dw: the parameter and its gradient in PyTorch's layout (64, Cin, 7, 7) - no packed copy; dw is accumulated into
 * (float atomics: not offered in the deterministic mode).  bias may be NULL; relu != 0 applies max(0, .) in the epilogue.
 * muvo_stem_conv_supported: 1 when the descriptor is such a stem (even input height / width) and MUVO_STEM_KERNEL != 0. */
int muvo_stem_conv_supported(const muvo_conv_desc* d);
int muvo_stem_conv_forward(const muvo_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int relu, void* stream);
int muvo_stem_conv_wgrad(const muvo_conv_desc* d, const float* x, const float* dy, float* dw, void* stream);

/* ---- prediction export (csrc/export.hip; the reference's sim_run.py:75-92 does this on the host after copying whole tensors) ----
 * Occupied-voxel rows: for F frames of a grid (X, Y, Z), z fastest, the voxels whose class is not 0 as rows x, y, z, class of four
 * uint16 - the recorder's (Q, 4) uint16 voxel files - in ascending h = (x*Y + y)*Z + z (the order of torch.where), the frames
 * concatenated: frame f owns rows [counts[0] + ... + counts[f-1], ... + counts[f]).
 *   muvo_voxel_rows_logits: class = first maximum over the C planes of logits (F, C, X, Y, Z) float32 with a strict > comparison
 *     (torch.argmax on finite input; non-finite logits are outside the contract), 2 <= C <= 16.  The logits are read once.
 *   muvo_voxel_rows_grid: class = grid (F, X, Y, Z) uint8 itself.
 * counts (F) int64 always receives the true number of rows per frame; rows beyond `cap` are not written (rows may be NULL with
 * cap 0: counts only).  muvo_voxel_rows_write writes the rows of the preceding counting call on the same scratch and counts (grid:
 * the same grid again, NULL after muvo_voxel_rows_logits), so a caller can size `rows` from the counts and the input is still read
 * only once.  rows must be 8-byte aligned.  scratch: muvo_voxel_rows_scratch_bytes(F, X, Y, Z) bytes (1 per voxel and frame plus
 * the chunk counters; -1 for sizes the entries refuse: an axis beyond 65536, 2^31 voxels or more, F beyond 65535).
 * muvo_image_u8: y[i] = trunc(x[i] * 255.0f) saturated to [0, 255], NaN -> 0, for n contiguous float32 elements (any n; 16-byte
 * loads where x is 16-byte and y 4-byte aligned).  For 0 <= x*255 < 256 this is numpy's (x * 255).astype(np.uint8). */
int64_t muvo_voxel_rows_scratch_bytes(int F, int X, int Y, int Z);
int muvo_voxel_rows_logits(const float* logits, int F, int C, int X, int Y, int Z, void* scratch, uint16_t* rows, int64_t cap,
                           int64_t* counts, void* stream);
int muvo_voxel_rows_grid(const uint8_t* grid, int F, int X, int Y, int Z, void* scratch, uint16_t* rows, int64_t cap, int64_t* counts,
                         void* stream);
int muvo_voxel_rows_write(const uint8_t* grid, int F, int X, int Y, int Z, const void* scratch, const int64_t* counts, uint16_t* rows,
                          int64_t cap, void* stream);
int muvo_image_u8(const float* x, uint8_t* y, int64_t n, void* stream);

/* ---- prediction panels (csrc/visualise.hip) ------------------------------------------------------------------------------------
 * Tiles of the reference's picture grids (trainer.py:569-1007), written from device tensors straight into a caller-allocated
 * uint8 panel.  A call places F = b * T tiles: frame f belongs to sample f / T and time step t = t0 + f % T, and its padded
 * tile starts at row y0 + t * ystep, column x0 + t * xstep (+ sepw when t >= tsep) of the sample's PH x PW planes.  Channel c
 * of sample n starts at byte n * sample_stride + c * chan_stride.  Every entry checks, before it launches anything, that every
 * tile lies inside its planes and the planes inside `panel_bytes`.
 * Common arguments: pad / padbyte - a border of `pad` pixels of value `padbyte` on every channel is part of the tile
 * ((h + 2 pad) x (w + 2 pad)); rotate (class tiles) - the padded tile goes in as torch.rot90(k = 1): out[i][j] = in[j][Wp - 1 - i],
 * (w + 2 pad) rows x (h + 2 pad) columns.  palette: 256 x 3 bytes R, G, B on the device.
 *   muvo_panel_image: channels c0 .. c0 + nch - 1 (nch = 1 or 3) of (F, C, h, w) float32; bytes by the rule of muvo_image_u8.
 *   muvo_panel_logits: (F, C, h, w) float32, 2 <= C <= 16; class = first maximum over C (strict >), then the palette.
 *   muvo_panel_labels: (F, h, w) uint8 or int64 (is_int64); palette entry of the value's low byte.
 *   muvo_panel_fill: h x w of `value` inside the border, on nch channels.
 *   muvo_panel_bars: one action value per frame -> the (int(h/4), w + 10) bar of trainer.py:679-706 without the text: all 255,
 *     rows [5, int(h/4) - 5), columns [mid, mid + k) for v >= 0 else [mid + k, mid), mid = int(w/2) + 5,
 *     k = (int)((float)(w / 2.0) * v), clipped to the tile (NaN: no bar); kind 0: (0, 200, 0) / (200, 0, 0) for v >= 0 / v < 0,
 *     kind 1: (0, 0, 200).
 *   muvo_panel_scatter: range view (F, C, H, W) float32 with x, y in channels 0, 1 and the range in channel C - 1 ->
 *     pcd_xy_image (trainer.py:980-1007) on a 256 x 256 tile: zeros, then 255 at ((int)r, (int)c) for every point with
 *     d * scale > 0, 0 < r < 256, 0 < c < 256, r = (-(x * scale)) * 2.56f + 128f, c likewise from y; fp32, uncontracted.
 *   muvo_panel_voxel_top_*: logits (F, C, X, Y, Z) float32 (first maximum) or a grid (F, X, Y, Z) uint8 -> an X x Y tile, pixel
 *     [i][j] = column x = X - 1 - i, y = j: z* = the highest z whose class is not 0; none: palette[0]; otherwise per channel
 *     (p * (96 + (159 * z*) / max(Z - 1, 1))) / 255 in integers, p = palette[class at z*]. */
typedef struct MuvoTilePlace {
  int64_t sample_stride, chan_stride;
  int32_t PH, PW;
  int32_t T, t0;
  int32_t x0, y0, xstep, ystep;
  int32_t tsep, sepw;
} MuvoTilePlace;
int muvo_panel_image(const float* src, int F, int C, int c0, int h, int w, int pad, int padbyte, int nch, uint8_t* panel, int64_t panel_bytes,
                     const MuvoTilePlace* place, void* stream);
int muvo_panel_logits(const float* src, int F, int C, int h, int w, const uint8_t* palette, int pad, int padbyte, int rotate, uint8_t* panel,
                      int64_t panel_bytes, const MuvoTilePlace* place, void* stream);
int muvo_panel_labels(const void* src, int is_int64, int F, int h, int w, const uint8_t* palette, int pad, int padbyte, int rotate,
                      uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place, void* stream);
int muvo_panel_fill(int F, int h, int w, int value, int pad, int padbyte, int nch, uint8_t* panel, int64_t panel_bytes,
                    const MuvoTilePlace* place, void* stream);
int muvo_panel_bars(const float* values, int kind, int F, int h, int w, uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place,
                    void* stream);
int muvo_panel_scatter(const float* range_view, int F, int C, int H, int W, float scale, int pad, int padbyte, uint8_t* panel,
                       int64_t panel_bytes, const MuvoTilePlace* place, void* stream);
int muvo_panel_voxel_top_logits(const float* logits, int F, int C, int X, int Y, int Z, const uint8_t* palette, int pad, int padbyte,
                                uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place, void* stream);
int muvo_panel_voxel_top_grid(const uint8_t* grid, int F, int X, int Y, int Z, const uint8_t* palette, int pad, int padbyte, uint8_t* panel,
                              int64_t panel_bytes, const MuvoTilePlace* place, void* stream);

/* ---- point-to-point ICP between lidar frames (icp.hip): the registration behind the reference's `_traj` panel -----------------
 * (compute_pcd_transformation, geometry_utils.py:248-267: open3d registration_icp, point-to-point, identity start).
 * src (Fs,Cs,n), tgt (Ft,Ct,n) channel-planar fp32 (the same tensor twice is fine); planes 0..2 = x, y, z, plane 3 = range; a
 * point is valid iff range > 0 (NaN: invalid) and the coordinates of invalid points never reach a result.  Coordinates are
 * multiplied by `scale` in fp32 on load.  Work list: P pairs, pair p registers frame src_frames[p] of src (the moving cloud)
 * onto frame tgt_frames[p] of tgt; both lists are device int32.
 * state: P x muvo_icp_state_doubles() doubles per pair - [0..11] T (3x4 row-major, target ~ T [source; 1]), [12] fitness =
 *   inliers / valid queries, [13] inlier_rmse, [14] [15] the same of the previous evaluation, [16] inliers, [17] iterations
 *   (= rigid fits applied), [18] status (MUVO_ICP_*), [19] evaluations, [20] valid queries, [21] valid target points.
 * done: P int32, non-zero once the pair has stopped; its state is never written again and its workgroups return at once.
 * muvo_icp_init: T = init (P x 12 doubles) or the identity (init NULL); a pair without a valid query or without a valid target
 *   point stops at once with the identity (MUVO_ICP_EMPTY; a frame index outside its tensor: MUVO_ICP_BAD_FRAME).  Queries are
 *   the source points 0, stride, 2 stride, ...
 * muvo_icp_iterate: `count` times { correspond; update }.  correspond: every valid query, moved by T (fp64, rounded to fp32),
 *   takes the valid target point with the smallest fp32 squared distance of the coordinate differences (lowest index on a tie)
 *   and is an inlier iff d^2 <= threshold^2 (fp32); per workgroup 17 fp64 sums over the inliers go to ws
 *   (muvo_icp_ws_doubles(P, n, stride) doubles, written then read) with plain stores.  update: sums them in block order, sets
 *   fitness / rmse, then stops the pair - fewer than 3 inliers (MUVO_ICP_FEW_INLIERS), not the first evaluation and
 *   |d fitness| < 1e-6 and |d rmse| < 1e-6 (MUVO_ICP_CONVERGED), iterations == max_iteration (MUVO_ICP_MAX_ITERATION) - with T
 *   unchanged, or sets T <- U T with U the least-squares rigid motion of the inlier pairs (Horn's quaternion form in fp64: a
 *   proper rotation always).  Atomics only in the grid build (below), where only the order inside a
 *   cell depends on them: results do not depend on scheduling.
 *   corr (P,n) int32 or NULL: the target index of every query of the LAST correspond that ran for the pair, -1 = invalid or
 *   gated out (entries of non-query points are left alone); sums (P,17) or NULL: count, sum d^2, sum s (3), sum q (3),
 *   sum s q^T (9, row = component of s) of that evaluation, s = the moved query, q = its target point.
 * n <= 2^24, P <= 65535. */
#define MUVO_ICP_RUNNING 0
#define MUVO_ICP_CONVERGED 1
#define MUVO_ICP_MAX_ITERATION 2
#define MUVO_ICP_FEW_INLIERS 3
#define MUVO_ICP_EMPTY 4
#define MUVO_ICP_BAD_FRAME 5
int64_t muvo_icp_state_doubles(void);
int64_t muvo_icp_ws_doubles(int64_t P, int64_t n, int64_t stride);
int muvo_icp_init(const float* src, const float* tgt, int64_t Fs, int64_t Ft, int Cs, int Ct, int64_t n, const int32_t* src_frames,
                  const int32_t* tgt_frames, int64_t P, int64_t stride, const double* init, double* state, int32_t* done, void* stream);
int muvo_icp_iterate(const float* src, const float* tgt, int Cs, int Ct, int64_t n, const int32_t* src_frames, const int32_t* tgt_frames,
                     int64_t P, float scale, float threshold, int64_t stride, int max_iteration, int count, double* ws, double* state,
                     int32_t* done, int32_t* corr, double* sums, void* stream);
/* The same registration with a grid-accelerated search: every output bit - corr, sums, state, done - equals muvo_icp_iterate's.
 * Definition: per query the exhaustive search contributes the lexicographic minimum of (fp32 d^2, target index) over the valid
 * target points, and only where that d^2 <= threshold^2 (fp32); the grid search finds exactly that minimum among the target
 * points that can lie within the threshold, with the same d = fmaf(dz, dz, fmaf(dy, dy, dx dx)) on the same fp32 operands, the
 * same gate and the same reduction (same queries per workgroup and lane, same order, same update kernel).
 * muvo_icp_grid_build (after muvo_icp_init, once per registration: the pose moves only the sources): per pair that is not done,
 *   the valid target points whose three scaled coordinates are finite (any other can never win) are binned into cubic cells
 *   (edge threshold / 8, doubled until the bounding box has at most 2^17 cells) - bounding box, histogram and scatter with
 *   integer atomics, exclusive scan.  Atomics only here, where only the order of the points inside a cell depends on them;
 *   the winner rule is lexicographic, so results do not depend on scheduling.  grid: muvo_icp_grid_bytes(P, n) bytes, 16-byte
 *   aligned, written here and read by muvo_icp_iterate_grid (same tgt, Ct, n, tgt_frames, P, scale; the threshold may differ).
 * muvo_icp_iterate_grid: muvo_icp_iterate with the search over the grid; a query whose moved coordinates are not finite has no
 *   candidate (corr -1), as in the exhaustive search where all its distances are NaN or inf. */
int64_t muvo_icp_grid_bytes(int64_t P, int64_t n);
int muvo_icp_grid_build(const float* tgt, int Ct, int64_t n, const int32_t* tgt_frames, int64_t P, float scale, float threshold,
                        const int32_t* done, void* grid, int64_t grid_bytes, void* stream);
int muvo_icp_iterate_grid(const float* src, const float* tgt, int Cs, int Ct, int64_t n, const int32_t* src_frames, const int32_t* tgt_frames,
                          int64_t P, float scale, float threshold, int64_t stride, int max_iteration, int count, double* ws, double* state,
                          int32_t* done, int32_t* corr, double* sums, const void* grid, int64_t grid_bytes, void* stream);

/* ---- dense optical flow between camera frames (flow.hip): the flow behind the reference's `_flow` panel ------------------------
 * The reference calls cv2.calcOpticalFlowFarneback(img1, img2, None, 0.5, 3, 15, 3, 5, 1.2, 0) (trainer.py:1009-1020).  This is
 * Farneback's two-frame method (polynomial expansion, SCIA 2003) with those parameters, but the numbers are OUR DEFINITION:
 * parity with cv2's output is not pinned anywhere.  tests/flow_reference.py restates the definition in numpy.
 * Input: two stacks of RGB frames (F, 3, h, w) float32 (the same tensor twice is fine) and P pairs; pair p goes from frame
 *   pairs_a[p] of frames_a to frame pairs_b[p] of frames_b.  pairs_a / pairs_b are HOST int32 arrays: they are validated before
 *   anything is launched and travel as kernel arguments, P <= muvo_flow_max_pairs() per call.  Index -1 is an all-white frame.
 *   Bytes by the rule of muvo_image_u8; grey = (4899 R + 9617 G + 1868 B + 8192) >> 14 on the bytes, then fp32.
 * Pyramid: L = 3 levels, dropped from the top while min(h, w) 0.5^(L-1) < 32.  Level k is (h + 2^(k-1)) >> k rows (round half
 *   up; columns alike).  Level k > 0 is the level-0 grey image blurred with a normalised Gaussian of sigma = (2^k - 1) / 2 and
 *   max(round(5 sigma) | 1, 3) taps (3 and 9; along x, then along y, replicated border), then resized bilinearly: source
 *   coordinate (o + 0.5) (n_in / n_out) - 0.5 clamped to [0, n_in - 1], second tap min(i + 1, n_in - 1), value
 *   (1 - fy) ((1 - fx) v00 + fx v01) + fy ((1 - fx) v10 + fx v11).  The coarsest level starts from zero flow; a finer level from
 *   the coarser flow resized the same way and multiplied by 2.
 * Polynomial expansion: per pixel the weighted least-squares fit of 1, x, y, x^2, y^2, xy over the 11 x 11 neighbourhood
 *   (replicated border), weight g(x) g(y), g the normalised Gaussian of sigma 1.2.  Moments: vertically sum g f, y g f, y^2 g f,
 *   then horizontally; the constant 6 x 6 normal matrix is inverted on the host in float64.  Kept: b_x, b_y, A_xx, A_yy and
 *   A_xy = half the xy coefficient.
 * One iteration (3 per level), flow d: the second frame's five values are sampled bilinearly at (x + dx, y + dy) with weights
 *   (1-a)(1-b), a(1-b), (1-a)b, ab, summed in that order.  Inside (0 <= x + dx < w - 1 and 0 <= y + dy < h - 1): A = (A0 + A1) / 2,
 *   db = (b0 - b1) / 2; outside: A = A0, db = 0.  b = db + A d.  The five values are multiplied by s(y) s(x), s = 0.14, 0.14,
 *   0.4472, 0.4472, 0.4472 for the five outermost rows / columns and 1 elsewhere.  The products Axx^2 + Axy^2, Axy (Axx + Ayy),
 *   Ayy^2 + Axy^2, Axx bx + Axy by, Axy bx + Ayy by are averaged over the 15 x 15 box (replicated border; 15 vertical sums, then
 *   15 horizontal, times 1/225) to g11, g12, g22, h1, h2 and d = ((g22 h1 - g12 h2), (g11 h2 - g12 h1)) / (g11 g22 - g12^2 + 1e-3).
 * fp32 throughout, uncontracted, every sum in ascending tap order, no atomics: a call is bit-reproducible and a pair's flow
 * does not depend on the other pairs.  flow: (P, 2, h, w) float32, [dx, dy] with frame_b(x + d) ~ frame_a(x).
 * h, w in 16..8192; ws: muvo_flow_workspace_bytes(P, h, w) bytes (-1 for sizes the entry refuses), 4-byte aligned.
 * muvo_flow_colour: the colour coding of trainer.py:1014-1020 (again our definition) of P flow fields as padded tiles of a
 *   3-channel panel (MuvoTilePlace as above, frame = pair): magnitude m = sqrtf(dx^2 + dy^2), angle = atan2f(dy, dx) in degrees
 *   in [0, 360); hue = trunc(angle / 2) (at most 179); saturation = trunc((m - min) 255 / (max - min)) with min / max over the
 *   pair's field, 0 when max = min; value 255; RGB by the 8-bit sextant formula in integers: i = hue / 30, r = hue % 30,
 *   p = 255 - sat, q = 255 - (2 sat r + 30) / 60, t = 255 - (2 sat (30 - r) + 30) / 60, (v,t,p) (q,v,p) (p,v,t) (p,q,v) (t,p,v)
 *   (v,p,q) for i = 0 .. 5.  A zero field is an all-255 tile.  Tiles are written in 2-pixel groups: every tile must start at an
 *   even panel column.  ws: muvo_flow_colour_ws_bytes(P) bytes.
 * muvo_flow_epe: acc[0] += sum |a - b|, acc[1] += sum |a|, acc[2] += the number of pixels, over the pixels at least 5 from the
 *   border of P pairs of flow fields (P, 2, h, w); |.| in fp32, sums in fp64 per workgroup (ws: muvo_flow_epe_ws_doubles(P)
 *   doubles), added to the device doubles acc[0..2] in a fixed order. */
int64_t muvo_flow_max_pairs(void);
int64_t muvo_flow_workspace_bytes(int64_t P, int h, int w);
int muvo_flow_farneback(const float* frames_a, int64_t Fa, const float* frames_b, int64_t Fb, int h, int w, const int32_t* pairs_a,
                        const int32_t* pairs_b, int64_t P, void* ws, int64_t ws_bytes, float* flow, void* stream);
int64_t muvo_flow_colour_ws_bytes(int64_t P);
int muvo_flow_colour(const float* flow, int64_t P, int h, int w, void* ws, int64_t ws_bytes, int pad, int padbyte, uint8_t* panel,
                     int64_t panel_bytes, const MuvoTilePlace* place, void* stream);
int64_t muvo_flow_epe_ws_doubles(int64_t P);
int muvo_flow_epe(const float* flow_a, const float* flow_b, int64_t P, int h, int w, double* ws, int64_t ws_doubles, double* acc, void* stream);

/* ---- first-hit ray casting through voxel class grids (raycast.hip): the `_voxel` panel and the RayIoU metric --------------------
 * OUR DEFINITION (the reference draws its voxel figures with matplotlib and has no ray metric); tests/raycast_reference.py restates
 * it in numpy float32 and the kernels equal that restatement bit for bit.
 * Grid cell (x, y, z) of a class grid (X, Y, Z) uint8 is the unit cube [x, x+1) x [y, y+1) x [z, z+1) in grid coordinates and is
 * occupied when its class is not 0.  A ray is seven fp32 numbers ox oy oz dx dy dz tmax; d need not have unit length.  Everything
 * is fp32 with + - x /, comparisons and floorf only, uncontracted, with correctly rounded division, in this order:
 *   1 slabs: t0 = 0, t1 = tmax, entry = 3.  For a = x, y, z with d_a != 0: inv_a = 1 / d_a; ta = (0 - o_a) inv_a; tb = (N_a - o_a) inv_a;
 *     (lo, hi) = (ta, tb) if ta <= tb else (tb, ta); the ray misses unless lo <= hi (only a NaN fails this); if lo > t0: t0 = lo and
 *     entry = a; if hi < t1: t1 = hi.  For d_a == 0 the ray misses unless 0 <= o_a < N_a.  The ray misses if every d_a is 0 and
 *     unless t0 < t1.  A NaN anywhere (origin, direction, tmax) therefore ends in a miss, an infinite direction component too.
 *   2 start cell: c_a = floorf(o_a + d_a t0) clamped to [0, N_a - 1] (compared as floats, then converted); t = t0, face = entry -
 *     face 3: the ray starts inside the grid.
 *   3 loop, at most X + Y + Z + 3 iterations whatever the input: an occupied cell is the hit - its linear index (x Y + y) Z + z, t,
 *     face.  Otherwise best = +inf and, for a = x, y, z with d_a != 0: tn_a = ((float)(c_a + (d_a > 0 ? 1 : 0)) - o_a) inv_a (fresh
 *     from the cell, never accumulated); if tn_a < best: best = tn_a, axis = a (strict: ties go x before y before z).  A miss if no
 *     axis was taken or best > t1; the axis' cell moves by sign(d_a), a miss if it leaves the grid; t = best, face = axis.
 * A miss is index -1, t 0, face 0.
 * Bricks: the occupancy of a frame as one uint64 per 4 x 4 x 4 block, (ceil(X/4), ceil(Y/4), ceil(Z/4)) words, bit
 *   (x&3) 16 + (y&3) 4 + (z&3); cells past the grid are 0.  muvo_raycast_brick_words: the words of F frames (-1 for sizes the
 *   entries refuse: F in 1..65535, every axis in 1..2048, fewer than 2^30 voxels).  muvo_raycast_bricks_grid packs (F, X, Y, Z)
 *   uint8; muvo_raycast_bricks_logits takes logits (F, C, X, Y, Z) float32, 2 <= C <= 16, class = first maximum over C (strict >, the
 *   rule of muvo_panel_logits), and also writes that class grid (F, X, Y, Z) uint8: the march never reads the logits.
 * muvo_raycast: rays (R, 7) on the device, the same table for all F frames -> hit (F, R) int32, t (F, R) float32, face (F, R)
 *   uint8.  The march takes occupancy from the words and reads a class byte only at a hit.  R <= 2^24.
 * muvo_panel_voxel_view: march + shading of an R x R ray table (ray i R + j is pixel (i, j)) as padded tiles of a 3-channel panel
 *   (MuvoTilePlace as above): a miss is palette[0]; a hit per channel (palette[class][ch] S[face] (96 + (159 z) / max(Z - 1, 1)))
 *   / 65025 in integers, S = (176, 208, 255, 255).  R <= 4096.
 * muvo_ray_iou_counts: every ray through a label grid and a prediction grid of one size, counts (3, C, 3) uint64 = threshold x class
 *   x (tp, fp, fn) on the device, added to: with the label's hit (cl, tl) and the prediction's (cp, tp), per threshold k - both hit,
 *   cl == cp and fabsf(tp - tl) res <= thresholds[k] (fp32): tp[cl] += 1; otherwise fn[cl] += 1 if the label hit and fp[cp] += 1 if
 *   the prediction hit; nothing when both miss.  Classes >= C are not counted.  thresholds: 3 HOST floats.  Integer atomics: the
 *   counts do not depend on scheduling.  depth[0] += sum of fabsf(tp - tl) res, depth[1] += the number of rays, both over the rays
 *   that hit in both grids: fp32 terms, fp64 partial sums per workgroup (ws: muvo_ray_iou_ws_doubles(F, R) doubles) added in a
 *   fixed order. */
int64_t muvo_raycast_brick_words(int F, int X, int Y, int Z);
int muvo_raycast_bricks_grid(const uint8_t* grid, int F, int X, int Y, int Z, uint64_t* bricks, int64_t words, void* stream);
int muvo_raycast_bricks_logits(const float* logits, int F, int C, int X, int Y, int Z, uint8_t* grid, uint64_t* bricks, int64_t words, void* stream);
int muvo_raycast(const uint8_t* grid, const uint64_t* bricks, int F, int X, int Y, int Z, const float* rays, int64_t R, int32_t* hit, float* t,
                 uint8_t* face, void* stream);
int muvo_panel_voxel_view(const uint8_t* grid, const uint64_t* bricks, int F, int X, int Y, int Z, const float* rays, int R, const uint8_t* palette, int pad,
                          int padbyte, uint8_t* panel, int64_t panel_bytes, const MuvoTilePlace* place, void* stream);
int64_t muvo_ray_iou_ws_doubles(int64_t F, int64_t R);
int muvo_ray_iou_counts(const uint8_t* label, const uint64_t* label_bricks, const uint8_t* pred, const uint64_t* pred_bricks, int F, int C, int X, int Y,
                        int Z, const float* rays, int64_t R, float res, const float* thresholds, uint64_t* counts, double* ws, int64_t ws_doubles,
                        double* depth, void* stream);

/* ---- rendered first-hit depth loss of the voxel head along rays (render.hip; an extension) -------------
 * OUR DEFINITION; tests/render_reference.py restates it.  logits (F, C, X, Y, Z) fp32, 2 <= C <= 16, V = X Y Z; rays (R, 7) fp32
 * on the device, the rows of muvo_raycast, one table for all F frames; sizes as muvo_raycast: F in 1..65535, every axis in 1..2048,
 * V < 2^30, R in 1..2^24.
 * Per cell, fp32: m = max_c z_c, e_c = expf(z_c - m), occ = e_1 + ... + e_{C-1} (ascending c), s = e_0 + occ; the free probability
 *   is q = e_0 / s and the occupied probability a = occ / s (this sum, never 1 - q: it keeps small a).
 * Per ray, the cell sequence: the march of muvo_raycast above, steps 1 - 3 word for word, through a grid in which no cell is
 *   occupied - the slabs, the clamped start cell, fresh boundaries with strict < and ties x, y, z, at most X + Y + Z + 3
 *   iterations, the end at best > t1 or on leaving the grid.  It gives cells k = 0..n-1 with entry depths t_k (fp32, the bits
 *   muvo_raycast reports as t for a hit in that cell) and the exit depth t_exit = t1.  A ray that muvo_raycast calls a miss before
 *   its step 2 (a NaN, a zero direction, missing the box) is INVALID: it contributes nothing and has zero gradient.
 * Rendered depth: T_0 = 1, T_{k+1} = T_k q_k, w_k = T_k a_k (fp32 products), D = sum_k w_k t_k + T_n t_exit (fp64 products and
 *   sum, in the order of k): the expectation of the first-hit depth RayIoU measures on the prediction side when every cell is
 *   occupied independently with probability a; a ray through nothing renders at the exit.  The march may stop where T is exactly
 *   0 (all later terms are exactly 0); there is no approximate cut-off.
 * Target: label_hit / label_t (F, R) are muvo_raycast's hit and t of the same rays through the label grid; t* = label_t where
 *   label_hit >= 0, t_exit otherwise.
 * loss[0] = weight / F * sum_f 1 / N * sum_{valid rays} |D - t*| with N = n_valid, the number of valid rays of the table (a
 *   property of the table and the grid size, not of the data: the caller counts it once); N = 0: loss 0, gradient 0.  fp64
 *   partial sums per workgroup, added by one workgroup in a fixed order; one fp32 device scalar, no host read.
 * Outputs: depth (F, R) fp64 = D and target (F, R) fp32 = t*, both 0 at invalid rays (kept for the backward pass); optional, for
 *   tests, NULL otherwise: t_last (F, R) fp32 = T_n, cells (F, R) int32 = n (-1: invalid), t_exit (F, R) fp32.  With one of them
 *   given the march does not stop at T == 0, so n is the full count; the loss has the same bits with and without them.
 * ws: muvo_render_ws_bytes(F, V, R) bytes (-1 for sizes the entries refuse) of 16-byte aligned scratch, written then read (q, a,
 *   the accumulator, the partials); one size serves both entries, nothing in it is kept between them.
 * Backward: with P_k = sum_{j<k} w_j t_j and Q_k = D - P_k - w_k t_k,  dD/dz_{k,c} = (T_{k+1} t_k - Q_k) (p_c - [c == 0]) - no
 *   division.  q and a are recomputed; every valid ray is marched again with D from the forward pass (P and D in fp64) and
 *   sign(D - t*) (T_{k+1} t_k - Q_k), sign(0) = 0, is added into a per-frame (F, V) accumulator of 64-BIT INTEGERS IN FIXED POINT
 *   with 26 fraction bits, rounded to nearest: the largest power of two for which R t_max scale < 2^62 with R <= 2^24 and
 *   t_max = 2048 sqrt(3), the longest unit-direction path through the largest grid (a contribution is clamped to +-4096 before
 *   the conversion, so the sum cannot overflow whatever the directions' lengths).  Integer atomics are order-free: loss and
 *   gradient have the same bits on every call, in both modes of muvo_set_deterministic.  A wave first sums neighbouring lanes that
 *   sit in the same cell.  One dense pass then writes every element of dlogits (F, C, V) = accumulator 2^-26 x gout weight /
 *   (F N) x (p_c - [c == 0]) (class 0: -a), zeros where no ray passed; gout = the upstream gradient of the scalar, on the device. */
int64_t muvo_render_ws_bytes(int64_t F, int64_t V, int64_t R);
int muvo_render_fwd(const float* logits, int64_t F, int C, int X, int Y, int Z, const float* rays, int64_t R, int64_t n_valid, const int32_t* label_hit,
                    const float* label_t, float weight, void* ws, int64_t ws_bytes, double* depth, float* target, float* t_last, int32_t* cells,
                    float* t_exit, float* loss, void* stream);
int muvo_render_bwd(const float* logits, int64_t F, int C, int X, int Y, int Z, const float* rays, int64_t R, int64_t n_valid, const double* depth,
                    const float* target, float weight, const float* gout, void* ws, int64_t ws_bytes, float* dlogits, void* stream);

/* ---- rendered first-hit class loss of the voxel head along rays (render_class.hip; an extension) ---------
 * OUR DEFINITION; tests/render_class_reference.py restates it.  Inputs as muvo_render_fwd: logits (F, C, X, Y, Z) fp32,
 * 2 <= C <= 16, V = X Y Z; labels (F, X, Y, Z) uint8; rays (R, 7) fp32 on the device, the rows of muvo_raycast, one table for all F
 * frames; F in 1..65535, every axis in 1..2048, V < 2^30, R in 1..2^24.
 * Per cell, fp32: m, e_c, occ and s = e_0 + occ as muvo_render_fwd has them; p_c = e_c / s, q = p_0.
 * Per ray: the cell sequence k = 0..n-1 and the validity rule of muvo_render_fwd (the march of muvo_raycast, steps 1 - 3, through a
 *   grid in which nothing is occupied).  An INVALID ray contributes nothing and has zero gradient.  T_0 = 1, T_{k+1} = T_k q_k (fp32
 *   products).
 * Target class y: label_hit (F, R) is muvo_raycast's hit of the same rays through the label grid; y = the class byte of the label
 *   at the hit cell, y = 0 where the label ray misses.  A class byte >= C at a hit cannot be refused without reading device memory
 *   on the host, so such a ray is IGNORED: it is reported as y = -1 and contributes nothing, like an invalid ray (it still counts
 *   in N).
 * Rendered mass: y >= 1: S_y = sum_k T_k p_{k,y}; y = 0: S_0 = T_n, the ray leaves the grid unhit.  Products and sum in fp64, in the
 *   order of k.  sum_c S_c = 1 by telescoping.  The march may stop where T is exactly 0 (all later terms are exactly 0); there is no
 *   approximate cut-off.
 * Loss of a ray: l = -log((S_y + eps) / (1 + eps)), eps = 2^-10, fp64: log(1025) = 6.93 without mass on the class, 0 for a perfect ray.
 * loss[0] = weight / F * sum_f 1 / N * sum_{valid rays} l with N = n_valid as for muvo_render_fwd; N = 0: loss 0, gradient 0.  fp64
 *   partial sums per workgroup, added by one workgroup in a fixed order; one fp32 device scalar, no host read.
 * Outputs: mass (F, R) fp64 = S_y and target (F, R) int32 = y - mass 0 and target -1 at invalid and ignored rays - kept for the backward pass;
 *   optional, for tests, NULL otherwise: t_last (F, R) fp32 = T_n (0: invalid), cells (F, R) int32 = n (-1: invalid).  With one of
 *   them given the march does not stop at T == 0, so n is the full count; the loss has the same bits with and without them.
 * ws: muvo_render_class_ws_bytes(F, C, V, R) bytes (-1 for sizes the entries refuse) of 16-byte aligned scratch, written then read
 *   (the probabilities cell-major (F, V, C) fp32, the accumulator (F, C, V) int64, the partials); one size serves both entries,
 *   nothing in it is kept between them.
 * Backward: A_j = T_j p_{j,y} and B_j = S_y - sum_{k<=j} A_k for y >= 1 (the exact tail of the forward's own fp64 sum: the ray is
 *   marched again with S_y from the forward pass); A_j = 0 and B_j = T_n = S_0 for y = 0.
 *   dS_y/dz_{j,c} = A_j [c = y] + B_j [c = 0] - p_{j,c} (A_j + B_j) and dl/dS_y = -r, r = 1 / (S_y + eps) in fp64, once per ray.
 *   A visit adds -A_j r to slot y and -B_j r to slot 0 of a per-cell vector of C slots, an (F, C, V) accumulator of 64-BIT INTEGERS
 *   IN FIXED POINT with 37 fraction bits, rounded to nearest (at most 2^-38 per add): every contribution has magnitude below 1
 *   (A_j <= S_y, B_j <= S_y), and 37 is the largest number of bits for which R x 1 x 2^37 < 2^62 with R <= 2^24 - the sum of a slot,
 *   and of the C slots of a cell (at most two adds per visit: < 2^63), cannot overflow.  A contribution is clamped to +-1 and a NaN
 *   becomes 0 before the conversion.  Integer atomics are order-free: loss and gradient have the same bits on every call, in both
 *   modes of muvo_set_deterministic.  A wave first sums neighbouring lanes with the same destination.  One dense pass then writes
 *   every element of dlogits (F, C, V): dz_{j,c} = (acc_c - p_c sum_c' acc_c') 2^-37 x gout weight / (F N), the sum over the slots
 *   in integers; zeros where no ray passed; gout = the upstream gradient of the scalar, on the device. */
int64_t muvo_render_class_ws_bytes(int64_t F, int C, int64_t V, int64_t R);
int muvo_render_class_fwd(const float* logits, const uint8_t* labels, int64_t F, int C, int X, int Y, int Z, const float* rays, int64_t R, int64_t n_valid,
                          const int32_t* label_hit, float weight, void* ws, int64_t ws_bytes, double* mass, int32_t* target, float* t_last,
                          int32_t* cells, float* loss, void* stream);
int muvo_render_class_bwd(const float* logits, int64_t F, int C, int X, int Y, int Z, const float* rays, int64_t R, int64_t n_valid, const double* mass,
                          const int32_t* target, float weight, const float* gout, void* ws, int64_t ws_bytes, float* dlogits, void* stream);

/* ---- Euclidean distance transform of voxel grids, boundary loss and voxel Chamfer counts (edt.hip; extensions)
 * OUR DEFINITIONS; tests/edt_reference.py restates them.
 * Grid: a class grid is (F, X, Y, Z) uint8, z fastest.  A cell is OCCUPIED iff 1 <= v <= 254; 0 is free, 255 is "unknown" and never
 *   occupied.  The class grid of a prediction is what muvo_raycast_bricks_logits writes (the first maximum over C: a tie with
 *   class 0 is free).
 * Transform: edt2(grid, cap)[f, v] = min(cap, min over the occupied cells u of frame f of |v - u|^2), an int32; distances in cells,
 *   cap >= 1.  A frame without an occupied cell is `cap` everywhere; cap >= X^2 + Y^2 + Z^2 is the untruncated transform.  Exact in
 *   integers.  Sizes: F in 1..65535, every axis >= 1 with X^2 + Y^2 + Z^2 < 2^31, F X Y Z < 2^36; everything else is refused before
 *   the device is touched.  Three separable min-plus passes d(i) = min_j (i - j)^2 + d(j), z, y, x, capped after each; with
 *   r^2 < cap only offsets |o| <= r are visited.  ws: muvo_voxel_edt_ws_bytes(F, X, Y, Z) bytes (-1 for refused sizes), 4-byte
 *   aligned, the intermediate of the y pass; out (F, X, Y, Z) int32. */
int64_t muvo_voxel_edt_ws_bytes(int64_t F, int X, int Y, int Z);
int muvo_voxel_edt(const uint8_t* grid, int64_t F, int X, int Y, int Z, int32_t cap, void* ws, int64_t ws_bytes, int32_t* out, void* stream);
/* Boundary loss: logits (F, C, X, Y, Z) fp32, 2 <= C <= 16, labels (F, X, Y, Z) uint8, truncation T >= 1 cells; the sizes of the
 *   rendered losses (every axis in 1..2048, V = X Y Z < 2^30).  Per frame f: g = label occupied, k = label is 255, P = the
 *   prediction's class grid occupied (a constant of the backward pass); q = s_0 = e_0 / sum_c e_c (fp32, e_c = exp(z_c - max),
 *   the sum in ascending c), p = 1 - q; edt_label = edt2(label, T^2), edt_pred = edt2(P, T^2), dG = sqrt(edt_label) / T and
 *   dP = sqrt(edt_pred) / T in fp32, both in [0, 1]; n_G = the occupied label cells.
 *   L_f = (sum_{v: !g, !k} p dG + sum_{v: g} q dP) / n_G, the terms fp32 products, the sums fp64.
 *   loss[0] = weight x the mean of L_f over the frames with n_G > 0, 0 without such a frame.  Both sums are divided by n_G: at
 *   n_P = n_G and hard predictions the term is the truncated Chamfer distance in units of T.
 *   Forward: per-workgroup fp64 partials, then one workgroup adds them in a fixed order: the same bits on every call in both modes
 *   of muvo_set_deterministic.  n_g (F + 1) int32: n_G per frame, then the number of frames with n_G > 0 - kept for the backward.
 *   ws: muvo_voxel_boundary_ws_bytes(F, V) bytes (-1 for refused sizes), 16-byte aligned, written then read.
 *   Backward: elementwise, no atomics, every element of dlogits (F, C, X, Y, Z) written: w dp/dz_c with dp/dz_0 = -q p,
 *   dp/dz_c = q s_c and w = gout weight / (frames n_G) x (dG where !g and !k, -dP where g, 0 where k): exactly 0 on 255 cells and
 *   on frames with n_G = 0.  gout = the upstream gradient of the scalar, on the device. */
int64_t muvo_voxel_boundary_ws_bytes(int64_t F, int64_t V);
int muvo_voxel_boundary_forward(const float* logits, const uint8_t* labels, const int32_t* edt_label, const int32_t* edt_pred, int64_t F, int C, int X, int Y, int Z,
                                int truncate, float weight, void* ws, int64_t ws_bytes, int32_t* n_g, float* loss, void* stream);
int muvo_voxel_boundary_backward(const float* logits, const uint8_t* labels, const int32_t* edt_label, const int32_t* edt_pred, const int32_t* n_g, int64_t F, int C,
                                 int X, int Y, int Z, int truncate, float weight, const float* gout, float* dlogits, void* stream);
/* Voxel Chamfer / F-score counts of label grids G and prediction grids P (both (F, X, Y, Z) uint8, the sizes of the boundary loss)
 *   from their UNTRUNCATED transforms edt_label = edt2(G, cap) and edt_pred = edt2(P, cap), cap >= X^2 + Y^2 + Z^2.  A frame where
 *   either set is empty (its transform reaches X^2 + Y^2 + Z^2 at cell 0) is skipped and counted.  Every other frame adds to the
 *   device accumulators counts (10) int64: [0] frames, [1] skipped frames, [2] n_P, [3] n_G, [4..6] hits_P[i] = #{v in P :
 *   edt_label(v) <= thresholds2[i]}, [7..9] hits_G[i] = #{v in G : edt_pred(v) <= thresholds2[i]}, and sums (2) fp64:
 *   sum_PG = sum_{v in P} sqrt((double)edt_label(v)), sum_GP = sum_{v in G} sqrt((double)edt_pred(v)).  thresholds2: 3 squared
 *   distances in cells, integers >= 0, on the host.  Integer counts by 64-bit atomics after a combine per wave and workgroup, the
 *   fp64 sums by per-workgroup partials that one wave adds in a fixed order.  ws: muvo_voxel_cd_ws_bytes(F, V) bytes, 8-byte aligned. */
int64_t muvo_voxel_cd_ws_bytes(int64_t F, int64_t V);
int muvo_voxel_cd_counts(const uint8_t* label, const uint8_t* pred, const int32_t* edt_label, const int32_t* edt_pred, int64_t F, int X, int Y, int Z,
                         const int32_t* thresholds2, uint64_t* counts, double* sums, void* ws, int64_t ws_bytes, void* stream);

/* ---- BEV instances from the centre / offset heads and their panoptic quality (bev_instance.hip; extensions)
 * OUR DEFINITIONS (the post-processing of Panoptic-DeepLab / FIERY, which the reference does not carry);
 * tests/bev_instance_reference.py restates them and the kernels equal that restatement exactly.
 * Inputs per frame: a centre map c (H, W) fp32; offsets o (2, H, W) fp32, channel 0 = centre_y - y, channel 1 = centre_x - x (the
 *   convention of muvo_instance_labels); and EITHER logits (C, H, W) fp32, 2 <= C <= 32, with a 32-bit set `things` (bit k: class k
 *   is a thing) OR a foreground mask (H, W) uint8 (non-zero = foreground); the other pointer is null.  F in 1..65535 frames along a
 *   grid dimension, H and W in 1..4096, H W <= 2^24; everything else is refused before the device is touched.
 * Foreground: a pixel is foreground iff its argmax class is a thing.  The argmax starts at class 0, scans upward and replaces on
 *   strictly greater: the first maximum wins, a NaN never replaces the running maximum (and a NaN at class 0 is never replaced).
 * Peaks: p is a peak iff c[p] > threshold and no in-bounds q of the (2 radius + 1)^2 window has c[q] > c[p]; radius in 1..3.  Every
 *   pixel of a plateau of equal maxima is a peak; a NaN is never a peak and never suppresses a neighbour.  threshold is not NaN.
 * Selection: the K peaks with the highest score, 1 <= K <= 254, among equal scores (-0 = +0) the lower row-major index; the kept
 *   centres are numbered 1..n in that order (score descending, then index ascending).  centres (F, K, 2) int32 holds (y, x) of centre
 *   k at row k - 1 and (-1, -1) in the rows past n; n (F) int32; capped (F) int32 is 1 where the frame had more than K peaks, else 0.
 * Grouping: for a foreground pixel (y, x), in fp32 and in this order (the library is built with -ffp-contract=off):
 *     ty = (float)y + o0;  tx = (float)x + o1;  d_k = (ty - cy_k) * (ty - cy_k) + (tx - cx_k) * (tx - cx_k)
 *   its id is the k (1-based) of the smallest d_k, the lowest k on equal d_k; a non-finite d_k never wins.  Background pixels, pixels
 *   whose d_k are all non-finite and every pixel of a frame without a centre get id 0.  ids (F, H, W) uint8.
 * ws: muvo_bev_instance_ws_bytes(F, H, W) bytes (-1 for refused sizes), 8-byte aligned: a counter and H W candidate keys per frame.
 *   One memset and three launches whatever F; no host synchronisation, nothing is copied to the host.  The candidate list is filled
 *   through an integer atomic; its order is arbitrary and no output depends on it. */
int64_t muvo_bev_instance_ws_bytes(int64_t F, int H, int W);
int muvo_bev_instance_decode(const float* center, const float* offset, const float* logits, int C, uint32_t things, const uint8_t* foreground, int64_t F,
                             int H, int W, float threshold, int radius, int K, void* ws, int64_t ws_bytes, uint8_t* ids, int32_t* centres, int32_t* n,
                             int32_t* capped, void* stream);
/* Panoptic-quality counts of label ids g and predicted ids q, both (F, H, W) uint8 with 0 = none (sizes as above).  Per frame: the
 *   areas a_i = #{g = i}, b_j = #{q = j} and the intersections n_ij; segments i, j > 0 MATCH iff 3 n_ij > a_i + b_j (IoU > 1/2 in
 *   integers: a match is unique); TP = matches, FP = predicted segments (b_j > 0) without a match, FN = label segments (a_i > 0)
 *   without one; the frame's IoU sum = sum over the matches of n_ij / (a_i + b_j - n_ij) in fp64.  ADDED TO the device accumulators
 *   counts (7) int64 - [0] frames, [1] frames whose capped[f] != 0 (capped (F) int32 of the decode; may be null), [2] label
 *   segments, [3] predicted segments, [4] tp, [5] fp, [6] fn - by integer atomics, and iou_sum (1) fp64: each frame's sum is added in
 *   a fixed order into a slot of its own and one wave adds the slots in a fixed order (the same bits on every call).
 *   ws: muvo_bev_pq_ws_bytes(F) bytes (-1 for refused F), 8-byte aligned: a 256 x 256 table of 32-bit counters per frame, filled by
 *   integer atomics, and the slots: 256 KB a frame whatever the ids are, so the workspace, not the ABI's F <= 65535, bounds a call in
 *   practice (1 GB at 4000 frames); a caller with more frames than its memory allows splits them over calls - the accumulators add up.
 *   One memset and three launches whatever F; nothing is read back. */
int64_t muvo_bev_pq_ws_bytes(int64_t F);
int muvo_bev_pq_counts(const uint8_t* label, const uint8_t* pred, const int32_t* capped, int64_t F, int H, int W, uint64_t* counts, double* iou_sum, void* ws,
                       int64_t ws_bytes, void* stream);

/* ---- sensor-visibility mask of the voxel labels (visibility.hip; an extension) ----------------------------
 * OUR DEFINITION (the reference has no visibility mask; its SemScal / GeoScal losses carry ignore_index = 255 and nothing writes
 * one); tests/visibility_reference.py restates it and the kernels equal that restatement bit for bit.
 * Inputs: a label grid (F, X, Y, Z) uint8, its bricks from muvo_raycast_bricks_grid (occupied is what that entry calls occupied:
 *   class != 0) and a ray table (R, 7) fp32 on the device, the rows of muvo_raycast, one table for all F frames; sizes as
 *   muvo_raycast: F in 1..65535, every axis in 1..2048, fewer than 2^30 voxels, R in 1..2^24.
 * Marking: for every ray that passes step 1 of muvo_raycast, walk the cells of its steps 1 - 3, the same fp32 statements in the
 *   same order, and mark each visited cell SEEN; stop after marking the first occupied cell, or where step 3 ends the walk
 *   (best > t1, no axis, leaving the grid).  A ray that is a miss before step 2 (a NaN, a zero or infinite direction, missing the
 *   box, t0 >= t1) marks nothing.  The loop runs at most X + Y + Z + 3 iterations, carried as an explicit trip count.
 * seen: one uint64 per 4 x 4 x 4 brick and frame in the layout and bit order of the occupancy bricks (word ((x>>2) BY + (y>>2)) BZ
 *   + (z>>2) of the frame, bit (x&3) 16 + (y&3) 4 + (z&3)); `words` >= muvo_raycast_brick_words(F, X, Y, Z), 8-byte aligned.
 *   muvo_visibility_mark clears it on the caller's stream and sets it with 64-bit integer OR atomics: a ray collects the bits of
 *   consecutive cells of one brick in a register and issues one atomic when the brick changes and at its end - unless the word,
 *   read first, already holds those bits (bits are only set during a call: a stale read costs an atomic, never a bit).  OR is
 *   order-free: the same inputs give the same bits on every call, in both modes of muvo_set_deterministic.
 * Masked label (muvo_visibility_apply): out (F, X, Y, Z) uint8 = label where label != 0; 0 where the cell is free and SEEN; 255
 *   where it is free and not SEEN.  Occupied cells are never masked: a sensor point put them there, whatever the discretised march
 *   does.  counts (2,) uint64 on the device, ADDED TO by integer atomics: [0] the free-and-seen cells, [1] the unknown cells of
 *   the call.  out may not alias label. */
int muvo_visibility_mark(const uint8_t* grid, const uint64_t* bricks, int F, int X, int Y, int Z, const float* rays, int64_t R, uint64_t* seen,
                         int64_t words, void* stream);
int muvo_visibility_apply(const uint8_t* label, const uint64_t* seen, int F, int X, int Y, int Z, uint8_t* out, uint64_t* counts, void* stream);

/* ---- calibration and uncertainty of a sample ensemble (calibration.hip; an extension) ----------------------
 * OUR DEFINITION (the reference scores every imagined sample's argmax on its own and has none of this);
 * tests/calibration_reference.py restates it in float64.
 * Inputs: logits = a HOST array of K device pointers, K in 1..8, each a contiguous (F, C, X, Y, Z) fp32 tensor (one sample each;
 *   K = 1: a reconstruction or a single sample), C in 2..16; label (F, X, Y, Z) uint8, 255 = ignore; F * X * Y * Z <= 2^40.  The
 *   entry only needs columns of Z contiguous cells: a 2-D head (F, C, H, W) goes in as X = H, Y = W, Z = 1.
 * Per voxel, in fp32, classes in ascending order (the library is built with -ffp-contract=off):
 *   p_k   = softmax(z_k): e_c = exp(z_c - max_c z_c), p_c = e_c * (1 / sum_c e_c); a logit of -inf is an ordinary input, p_c = 0
 *   pbar  = (sum_k p_k) / K
 *   yhat  = the first maximum of pbar over the classes (strict >: the lowest index wins a tie, the rule of muvo_voxel_rows_logits);
 *           at K = 1 the first maximum of the logits themselves - exp is monotone, so that class is a maximum of pbar too, and the
 *           prediction is the one of muvo_ssc_counts even where rounding made two probabilities equal
 *   conf  = pbar[yhat];  correct = (yhat == y);  bin = min(B - 1, floor(conf * B))
 *   A decision fp32 rounding could turn - the two largest pbar closer than 1e-5, or conf * B within 1e-5 B of an integer - is taken
 *   again with pbar in fp64 (a rare branch that re-reads the voxel's logits): yhat, correct and bin, hence every integer output, equal
 *   a float64 evaluation of these formulae unless that evaluation itself is within its own rounding of a tie.  Values stay fp32.
 *   H     = -sum_c pbar_c ln pbar_c (0 ln 0 = 0);  Ebar = (sum_k H(p_k)) / K;  MI = max(0, H - Ebar)   (MI is exactly 0 at K = 1)
 *   brier = sum_c (pbar_c - [y == c])^2;  nll = -ln max(pbar_y, 1e-12)
 * Which voxels count.  label == 255: counted in `ignored`, nothing else (its logits are not even read unless a map is asked for).
 *   Otherwise NON-FINITE - in any sample the maximum logit is +inf or -inf (every logit -inf: the softmax is undefined) or any logit
 *   is NaN: counted in `skipped_nonfinite`, nothing else.  Otherwise scored: voxels + ignored + skipped_nonfinite = F X Y Z.
 *   A scored voxel whose label is >= C goes the way of muvo_ssc_counts: it is never correct, it counts in the completion counts as
 *   occupied, its prediction gets a false positive and no class gets the false negative; here also [y == c] is 0 for every c
 *   (brier = sum pbar_c^2) and pbar_y = 0 (nll = -ln 1e-12).
 * Accumulators: caller-owned, caller-zeroed device buffers that are ADDED TO (two calls into the same buffers add up), all
 *   integers, all by 64-bit integer atomics - order-free, the same bits on every call and in both modes of muvo_set_deterministic:
 *   table (B, 3) int64, B in 1..32 equal-width confidence bins, bin = min(B - 1, floor(conf * B)): n, n_correct, FIX(conf)
 *   counts (4) int64: voxels (scored), ignored, skipped_nonfinite, correct
 *   ssc (3 + 3 C) uint64: layout and counting rule of muvo_ssc_counts, taken on yhat; at K = 1 and finite logits equal to it
 *   sums (6) int64: FIX(brier), FIX(nll), FIX(H) over correct voxels, FIX(H) over wrong, FIX(MI) over correct, FIX(MI) over wrong
 *   FIX(v) = round-to-nearest-even(v * 2^24), an integer: the real sum is word / 2^24.  Rounding a voxel's value to 2^-24 costs at
 *   most 2^-25 a voxel, below the fp32 error of the value itself.  OVERFLOW: a value is < 2^5 (nll <= 27.7, H and MI <= ln 16,
 *   brier <= 2, conf <= 1), its FIX < 2^29, so a word cannot overflow before 2^34 scored voxels (1.7e10: 364 calls of 20 frames of
 *   192 x 192 x 64) even if every voxel had the worst nll; the conf, brier, H and MI words hold 2^38 voxels.
 * Optional outputs (NULL = not written; written, not added to):
 *   ens (F, X, Y, Z) uint8: yhat; 255 where the label is 255 or the voxel is non-finite
 *   top_entropy, top_mi (F, X, Y) uint8: the maximum over z of q(H), q(MI), q(v) = round-to-nearest-even(255 * min(1, v * (1 / ln C)))
 *   with ln C in fp32, over ALL finite voxels of the column, labelled or ignored (they describe the forecast, not the score); a
 *   non-finite voxel contributes 0.
 * One launch, no workspace, no host synchronisation, nothing is copied to the host. */
int muvo_voxel_calibration(const float* const* logits, int K, const uint8_t* label, int64_t F, int C, int X, int Y, int Z, int B,
                           int64_t* table, int64_t* counts, uint64_t* ssc, int64_t* sums, uint8_t* ens, uint8_t* top_entropy, uint8_t* top_mi,
                           void* stream);

/* ---- voxel labels filled from neighbouring frames (voxel_aggregate.hip; an extension) -----------------------
 * OUR DEFINITION (the reference has neither the visibility mask nor this); tests/voxel_aggregate_reference.py restates it in
 * numpy float64 and muvo_voxel_aggregate equals that restatement byte for byte.
 * Frames: F = B * S, frame f = i S + t is time t of sequence i.  State of cell c of frame f (the masked label of
 *   muvo_visibility_apply): S(f, c) = the class v >= 1 if the cell is occupied (its occupancy bit is set; v = grid byte), 0 if it is
 *   free and SEEN, UNK if it is free and not SEEN.
 * Poses: link t (1 <= t < S) of sequence i is row i (S - 1) + t - 1 of T (B (S - 1), 4, 4) fp64, the rigid motion with
 *   p_{t-1} ~ T_t p_t in RANGE-VIEW coordinates r = the x, y, z planes of range_view_label_1 times LIDAR_RE.SCALE (what
 *   muvo_icp_* returns for the pair t -> t - 1): metres in the ego frame, x forward, y mirrored as convert_coor_lidar leaves it,
 *   z up, origin at the ego vehicle's reference point (the lidar's offset is already added: input_dev.h range_point stores
 *   raw + POINTS.LIDAR_POSITION).  A link is VALID iff its status is none of MUVO_ICP_FEW_INLIERS / _EMPTY / _BAD_FRAME, its
 *   fitness >= min_fitness (a NaN fitness is invalid) and the 12 entries of its top three rows are finite.  fitness and status
 *   (fp64, int64: the tensors of the ICP result) may both be NULL: then only finiteness decides.
 * Frame map: a point r lies in grid coordinates g_a = map[a] r_a + map[3 + a] (a = x, y, z; cell j = floor(g)).  For the labels of
 *   scale k in {1, 2, 4}: map = (1 / (VOXEL.RESOLUTION k)) for all three axes - the grid axes ARE the ego axes, no sign flips - and
 *   (VOXEL.EV_POSITION) / k: voxelize.hip bins the ego-frame point e into cell (e + off) / res with off = VOXEL.EV_POSITION res,
 *   and voxel_view.lidar_rays puts the lidar at EV_POSITION + (px, -py, pz) / res, the ego-frame position of raw point 0.
 * Chain (muvo_voxel_pose_chain): M(t' <- t) for t' = t - d: M_d = T_{t-d+1} M_{d-1}; for t' = t + d: M_d = inv(T_{t+d}) M_{d-1},
 *   M_0 = I, inv([R, tau]) = [R^T, -R^T tau] (the rigid inverse; -R^T tau as -((R_0a tau_0 + R_1a tau_1) + R_2a tau_2)), products
 *   as ((a_0 b_0 + a_1 b_1) + a_2 b_2) [+ tau].  The pair is USABLE iff t' is in [0, S) and every link between t and t' is valid.
 *   Conjugated into cells: R'_ab = (map[a] R_ab) / map[b], tau'_a = (map[a] tau_a + map[3+a]) - ((R'_a0 o_0 + R'_a1 o_1) + R'_a2 o_2)
 *   with o = map[3..5].  Slot 2 (d - 1) holds t' = t - d, slot 2 (d - 1) + 1 holds t' = t + d, d = 1 .. window: the walk order.
 *   mats (F, 2 window, 12) fp64 row-major 3 x 4, usable (F, 2 window) uint8; a slot that is not usable holds zeros.  All fp64, one
 *   workgroup, nothing read back.  window in 1..64, S in 1..65535, map[0..2] non-zero and finite.
 * Fill (muvo_voxel_aggregate): A(f, c) = S(f, c) where that is not UNK - own observations are never overridden and come out as
 *   muvo_visibility_apply writes them.  Otherwise the slots are walked in order (nearest in time first, past before future); a
 *   slot that is not usable is skipped; q = M (c + 1/2) in fp64, every row ((m0 cx + m1 cy) + m2 cz) + m3 in that order without
 *   contraction; j = floor(q) per axis; if j is inside the grid (a NaN is outside) and S(f', j) != UNK for the slot's frame
 *   f' = f -+ d then A = S(f', j) and the walk stops.  No value at the end: A = 255.
 *   grid (F, X, Y, Z) uint8, bricks / seen: the words of muvo_raycast_bricks_grid / muvo_visibility_mark for it; out may not alias
 *   grid.  counts (3,) int64 on the device, ADDED TO by integer atomics (one per workgroup and counter): [0] cells filled
 *   occupied, [1] cells filled free, [2] cells still unknown; [0] + [1] + [2] = the unknown count of muvo_visibility_apply.
 *   A pure gather: the same bytes on every call and in both modes of muvo_set_deterministic.  F a multiple of S, sizes as
 *   muvo_visibility_apply. */
int muvo_voxel_pose_chain(const double* T, const double* fitness, const int64_t* status, int B, int S, double min_fitness, int window,
                          const double* map, double* mats, uint8_t* usable, void* stream);
int muvo_voxel_aggregate(const uint8_t* grid, const uint64_t* bricks, const uint64_t* seen, int F, int S, int X, int Y, int Z, int window,
                         const double* mats, const uint8_t* usable, uint8_t* out, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUVO_HIP_H */
