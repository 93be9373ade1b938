/* libdanhip — C ABI of the MI355X-native detector hot path (drop-in boundary).
 *
 * What it replaces in the reference (HiKapok/DAN; paths relative to the reference checkout):
 *   - the TF custom-op plugin loaded by utility/custom_op.py:33-63 (tf.load_op_library of
 *     cpp/Deform/build/libdeform.so and cpp/ExtraLib/build/libextra_lib.so):
 *       DeformConvOp / DeformConvBackpropOp   cpp/Deform/deform_conv.cc:51,170
 *       SmallMiningMatch                      cpp/ExtraLib/small_mining_match.cc:31
 *       DynamicAnchorRouting                  cpp/ExtraLib/dynamic_anchor_routing.cc:32
 *   - the TF built-in kernels the graphs in net/<model>.py call (conv2d, pools, resize_bilinear, softmax-CE,
 *     top_k, non_max_suppression, Momentum) whose source is not in the reference tree.
 *
 * Conventions (all entry points):
 *   - extern "C"; returns 0 (DANHIP_OK) or a negative DANHIP_E* code; never throws / aborts;
 *     danhip_last_error() returns a thread-local message for the last failure.
 *   - every tensor pointer is a caller-owned DEVICE pointer (16-byte aligned); nothing is allocated
 *     inside; scratch comes from a caller-supplied workspace where a *_workspace_bytes() query exists.
 *   - every call takes a hipStream_t (passed as void*) and is asynchronous on it; no host sync.
 *   - re-entrant and thread-safe.  The ONE piece of process-wide mutable state is the table of kernel-FORM switches behind
 *     danhip_set_option (below): filled from the environment exactly once, every value an atomic, read once per call by a launcher;
 *     whatever it says, results agree up to fp32 summation order.  (Bound once and read-only afterwards: the RCCL entry points of
 *     danhip_comm_*.)  Nothing else outlives a call.
 *   - activations are NHWC, 16-bit, passed as raw uint16.  The 16-bit type is a property of the library build:
 *     libdanhip.so = bf16 (default; every "bf16" below), libdanhip_f16.so = IEEE fp16 (same entry points, same layouts,
 *     v_mfma_f32_16x16x32_f16; BASELINE.json configs[4] "fp16 + MFMA").  danhip_act_dtype() tells which one is loaded;
 *     wherever an out_dtype argument says DANHIP_BF16 it means "the build's 16-bit type" (DANHIP_F16 is accepted as an
 *     alias in the fp16 build).  Accumulation, master weights, gradients of weights and all box / loss arithmetic are fp32.
 */
#ifndef DANHIP_H_
#define DANHIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DANHIP_OK 0
#define DANHIP_EINVAL (-1)   /* bad argument / unsupported shape            */
#define DANHIP_ELAUNCH (-2)  /* kernel launch failed                        */
#define DANHIP_EWORKSPACE (-3) /* workspace too small                        */

#define DANHIP_F32 0
#define DANHIP_BF16 1
#define DANHIP_F16 2
#define DANHIP_SPLIT3 3      /* out_dtype of danhip_conv2d_fwd[_ws] in the fp16 build: y = the [hi | lo | hi] half-limb map [N,Ho,Wo,3*Cout] (split_infer.hip) */

const char* danhip_last_error(void);
int danhip_version(void);
/* Process-wide kernel-FORM switches (A/B and test hooks; defaults from the environment variables in brackets, read once; values are
 * atomics and a launcher reads a switch once per call):
 *   "splitk"     [DANHIP_SPLITK, 1]      0: never split K (danhip_conv2d_workspace_bytes answers 0)
 *   "wgrad_slab" [DANHIP_WGRAD_SLAB, 1]  0: weight-gradient partial sums always by fp32 atomics; 2: always stores + combine pass; 1: by launch length
 *   "halo_b2"    [DANHIP_HALO_B2, 0]     1: a second workgroup barrier per step in csrc/conv_halo.hip (the round-2 form; timing A/B only)
 *   "wgrad_b2"   [DANHIP_WGRAD_B2, 0]    1: the same for csrc/conv_wgrad_rows.hip and csrc/conv_wgrad_pw.hip
 *   "deform_bwd_form" [DANHIP_DEFORM_BWD_FORM, 0]  deformable backward: 0 form by the offsets' statistics (on the device), 1 always the
 *                                           gather form with a +-2 px window, 2 always the fp32-atomics scatter form, 3 gather form, +-1 px
 *   "deform_dx_untiled" [DANHIP_DEFORM_DX_UNTILED, 0]  1: the +-1 px gather of the deformable backward as the wave-per-input-pixel kernel instead
 *                                           of the LDS-staged tile kernel (same candidates, weights and summation order)
 *   "halo_general_epilogue" [DANHIP_HALO_GENERAL_EPILOGUE, 0]  1: csrc/conv_halo.hip always takes its general epilogue (A/B of the lean one)
 *   "wgrad_c8"   [DANHIP_WGRAD_C8, 1]    0: the first layer's weight gradient (3x3, 8-channel image, 64 outputs) on the general kernel instead of
 *                                           csrc/conv_wgrad_c8.hip
 *   "pw_dgrad_ld_bn" [DANHIP_PW_DGRAD_LD_BN, 128]  256: csrc/conv_pointwise.hip's data gradient with a ReLU mask / accumulation may take 256-wide tiles
 *   "deterministic" [DANHIP_DETERMINISTIC, 0]  1: deterministic mode, see below
 *   "crc_table"  [DANHIP_CRC_TABLE, 1]   0: danhip_crc32c_batch walks with the table-free shift form instead of the slicing-by-4 table in LDS (same bits)
 * Results agree up to fp32 summation order whatever the setting.  danhip_set_option returns DANHIP_EINVAL for an unknown name. */
int danhip_set_option(const char* name, int value);
int danhip_get_option(const char* name);
int danhip_act_dtype(void);   /* DANHIP_BF16 or DANHIP_F16 */

/* ------------------------------------------------------------------------------------------------
 * Deterministic mode (option "deterministic" = 1; default 0 changes nothing: same launches, same bytes, no workspace asked for).
 * Every fp32 sum of the S3FD training step that crosses workgroups - weight / bias / gamma gradients, the loss sums, the optimizer's L2 term -
 * leaves its workgroup as a plain store into a caller-provided workspace (one row of partial sums per workgroup) and is finished in a FIXED
 * order, so two runs of the same call on the same inputs return the same bits.  Float atomics are not used (global or LDS).
 *
 * THE ORDER CONTRACT - danhip_ordered_reduce_f32(part [P][C], P, C, out [C], accumulate), the kernel every site hands its rows to:
 *   P <= DANHIP_ORDERED_REDUCE_SEQ_MAX (64):  S[c] = (((part[0][c] + part[1][c]) + part[2][c]) + ...) + part[P-1][c]       (fp32, ascending p)
 *   P >  DANHIP_ORDERED_REDUCE_SEQ_MAX:       G = ceil(P / 4);  S_k[c] = that sequential sum over the rows k G <= p < min(P, (k+1) G), k = 0..3;
 *                                             S[c] = ((S_0[c] + S_1[c]) + S_2[c]) + S_3[c]
 *   out[c] = S[c], or with accumulate != 0 out[c] = out[c] + S[c]: ONE add onto the old value.
 * The grouping is a function of P alone - never of the grid size or the CU count.  (The combine kernels of the weight-gradient slab form,
 * csrc/conv_wgrad_rows.hip / conv_wgrad_pw.hip, keep their own fixed order: wave w sums the splits w, w + 4, ... in rounds of eight, the
 * four wave sums are added as (0 + 1) + (2 + 3), then one add onto dw.)
 *
 * Scope of "same bits": the NUMBER of partial rows of the weight-gradient kernels derives from the device's CU count, so results are
 * reproducible per (library build, CU count) - not across devices with different CU counts, library versions, or more than one rank.
 *
 * In deterministic mode:
 *   - danhip_conv2d_bwd_weight_workspace_bytes(d) > 0 for EVERY descriptor (the size includes the bias-gradient rows), and
 *     danhip_conv2d_bwd_weight, or _ws / _strided with ws == NULL or too small, return DANHIP_EINVAL (no silent fall-back to atomics);
 *   - danhip_conv2d_bwd_data_first_supported answers 0 (callers take danhip_conv2d_bwd_data_bits + danhip_conv2d_bwd_weight_ws);
 *   - danhip_relu_bwd_bias_grad (db != NULL), danhip_l2norm_bwd, danhip_l2norm_bwd_pool_scatter, danhip_detection_loss_fwd and
 *     danhip_sgd_momentum_flat[_dynamic] (l2_out != NULL) return DANHIP_EINVAL: call their _ws forms (declared next to them);
 *   - danhip_deform_sample_bwd and danhip_deform_conv_bwd* run their ordered form for ONE shape class (below) and need its larger workspace;
 *   - out of scope, DANHIP_EINVAL: danhip_conv2d_bwd_data_bits_first, danhip_batchnorm_fwd_train, danhip_batchnorm_bwd, danhip_bn_act_*, the deformable backward
 *     of every other shape class, danhip_deform_psroi_pool_bwd (their float atomics have no ordered form).
 * With the option at 0 the _ws forms behave exactly as the plain calls (the workspace is ignored).
 *
 * Deformable backward in deterministic mode (ABI version 17).  Shape class: 3 x 3 taps, stride 1, dilation 1, SAME padding of 1,
 * C / deformable_group == 64 - what DAN-Deform uses; any other shape returns DANHIP_EINVAL with a message that says the shape class has no
 * ordered form.  dOffset and the gather part of dX come from the tile kernels of default mode, which were ordered already (candidates in
 * ascending index, fixed shuffle trees).  The all-atomics scatter form is never chosen (option "deform_bwd_form" = 2 is DANHIP_EINVAL in
 * the mode, as is "deform_dx_untiled"); the gather window is +-1 while at most 1 / 128 of the offset pairs leave [-1, 1), else +-2 - the
 * integer statistic of default mode, a function of the offsets alone ("deform_bwd_form" = 3 / 1 still pins it).  No float atomic runs.
 * FAR CORNERS (bilinear corners more than R pixels from their tap's nominal position, R = the window) leave through records, not atomics:
 *   record       one far corner: source row m * 9 + t of dS (m = output pixel, t = tap) and corner index k of corner_set (0..3);
 *                key = (m * 9 + t) * 4 + k.  Corners that coincide under the high-edge clamp are separate records: k is part of the key.
 *   destination  (n, h, w, group): the 64 fp32 sums of the side buffer far_dx the corner lands on.
 * THE ORDER CONTRACT for one far_dx element:  F = ((0 + c_1) + c_2) + ... in fp32, c_i = w_i * dS_i over the destination's far records in
 * ASCENDING (m, t, k), w = the weight corner_set gives the corner (the weights default mode's atomics add).  Each step is one fused
 * multiply-add F <- fma(w_i, dS_i, F) in this build.  far_dx is stored plainly (zeros where no record lands) and the dX tile kernel reads
 * it as before: ONE add onto the gather sum, then the ReLU mask, the accumulate and the 16-bit store.  The result is a function of the
 * inputs alone - not of the grid size, the CU count or timing.
 * Mechanism (csrc/deform_far.hip): count per destination (integer atomics), exclusive prefix sum, fill (a segment's order is arbitrary
 * here), then per destination repeated selection of the smallest key not yet taken - that removes the fill order - and the sum.  Six launches
 * whatever the offsets are, no host synchronisation: the step stays capturable.  Segments of any length are summed correctly; the selection
 * costs L^2 / 8 loads for a segment of L records, short segments are the fast case.
 * Workspace, sized from the shape alone (worst case: four records per (pixel, tap, group), a count and a start word per destination; about
 * 250 MB at 160 x 160 x 256, batch 16): danhip_deform_sample_bwd_ordered_workspace_bytes = the default workspace + that region, 0 outside the
 * shape class; danhip_deform_conv_bwd_ordered_workspace_bytes = 2 column buffers + that + the weight gradient's partial rows
 * (danhip_conv2d_bwd_weight_workspace_bytes of the GEMM: ask with the option SET).  A smaller buffer is DANHIP_EWORKSPACE.  Shapes with
 * N * H * W * deformable_group * 9 >= 2^30 are refused (32-bit record ids).
 * danhip_deform_far_ordered runs the far path alone into the workspace's first N*H*W*C floats (zeros where nothing lands; window: 0 by the
 * statistic, 1, 2) and danhip_deform_far_ordered_emulate is the same computation on the host - the per-record routines are one header
 * (csrc/deform_far.h) compiled for both sides - with every index checked (*range_errors, NULL allowed; DANHIP_EINVAL when any) and the
 * sums formed in the contract's order: the two far_dx agree bit for bit.  *records_out (NULL allowed) = the number of far records. */
size_t danhip_deform_sample_bwd_ordered_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t deformable_group);
size_t danhip_deform_conv_bwd_ordered_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                                                      int32_t deformable_group);
int danhip_deform_far_ordered(const uint16_t* offsets, const uint16_t* dS, int32_t N, int32_t H, int32_t W, int32_t C, int32_t deformable_group,
                              int32_t window, float* workspace, size_t workspace_bytes, void* stream);
int danhip_deform_far_ordered_emulate(const uint16_t* offsets, const uint16_t* dS, float* far_dx, int64_t far_dx_elems, int32_t N, int32_t H, int32_t W,
                                      int32_t C, int32_t deformable_group, int32_t window, int64_t* records_out, int64_t* range_errors);
#define DANHIP_ORDERED_REDUCE_SEQ_MAX 64
int danhip_ordered_reduce_f32(const float* part, int32_t P, int64_t C, float* out, int accumulate, void* stream);
/* Workspace of the _ws forms of danhip_relu_bwd_bias_grad / danhip_l2norm_bwd / danhip_l2norm_bwd_pool_scatter over M pixels (N*H*W) of C channels:
 * one row of C partial sums per workgroup of the largest grid any of them launches (a function of M and C alone). */
size_t danhip_reduce_workspace_bytes(int64_t M, int32_t C);
#define DANHIP_LOSS_WS_BYTES 2048      /* danhip_detection_loss_fwd_ws: 128 workgroups x 4 sums */
#define DANHIP_SGD_WS_BYTES 16640      /* danhip_sgd_momentum_flat_ws: 4096 workgroup sums + 64 column sums */
size_t danhip_loss_workspace_bytes(void);   /* the two sizes above, for callers that bind the library without this header */
size_t danhip_sgd_workspace_bytes(void);

/* ------------------------------------------------------------------------------------------------
 * Dense convolution (tf.layers.conv2d, padding='same'; net/sfd_net.py:81-89 conv_relu and every
 * tf.layers.conv2d call in net/<model>.py).  bf16 NHWC activations, fp32 accumulate on MFMA.
 *
 * Weight packing: the TF kernel variable is HWIO fp32 [kh,kw,Cin,Cout].  The forward kernel consumes
 * wf = bf16 [Cout_pad][Kpad] with k = (i*kw+j)*Cin_pad + c (K-contiguous per output channel); the data
 * gradient consumes wb = bf16 [Cin_pad][Kpad_b] with k = (i*kw+j)*Cout_pad8 + co.  Both are produced by
 * danhip_pack_conv_weight (sizes via danhip_conv_packed_elems).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int32_t N, H, W, Cin;      /* input  [N,H,W,Cin]   (Cin multiple of 8: pad the tensor otherwise)     */
  int32_t Ho, Wo, Cout;      /* output [N,Ho,Wo,Cout]                                                  */
  int32_t kh, kw, stride;    /* Ho/Wo = ceil(in/s): TF 'same' (pad_before = max((Ho-1)*s+kh-H,0)/2 derived);
                                Ho/Wo = floor((in-k)/s)+1: 'valid' (no padding)                          */
} danhip_conv_desc;

/* rows/cols of the packed forward (which=0) or data-gradient (which=1) weight matrix */
int danhip_conv_packed_dims(const danhip_conv_desc* d, int which, int64_t* rows, int64_t* cols);
/* w_hwio fp32 [kh,kw,CinReal,Cout] (CinReal <= d->Cin; extra input channels get zero weights) */
int danhip_pack_conv_weight(const danhip_conv_desc* d, const float* w_hwio, int32_t cin_real,
                            uint16_t* wf_packed, uint16_t* wb_packed, void* stream);

/* All conv weights of a model packed by ONE launch (after each optimizer update).  The caller fills a host array of
 * entries with danhip_pack_entry_init (which also returns how many workgroups the entry gets; first_block is the running
 * sum), copies it to the device and passes it here with the total.  Same packing as danhip_pack_conv_weight. */
typedef struct {
  const float* w_hwio;
  uint16_t* wf_packed;
  uint16_t* wb_packed;       /* NULL: forward packing only */
  int32_t kh, kw, cin, cin_real, cout, rows_f, cols_f, rows_b, cols_b, co8, first_block, pad_;
} danhip_pack_entry;
int danhip_pack_entry_init(danhip_pack_entry* e, const danhip_conv_desc* d, const float* w_hwio, int32_t cin_real,
                           uint16_t* wf_packed, uint16_t* wb_packed, int32_t first_block, int32_t* blocks);
int danhip_pack_conv_weights_batched(const danhip_pack_entry* table_dev, int32_t n, int32_t total_blocks, void* stream);

/* y = act(conv(x, w) + bias).  x bf16; y bf16 (out_dtype=DANHIP_BF16) or fp32; bias fp32[Cout] or NULL.
 * Pointwise (1x1, stride 1) convolutions with channel counts that are multiples of 64 run on the streaming GEMM kernel
 * (csrc/conv_pointwise.hip; bias / ReLU, or mask / accumulate for danhip_conv2d_bwd_data, in its epilogue).  No vendor GEMM or
 * convolution library is linked.
 * relu: 0/1.  residual: optional bf16 tensor of y's shape added AFTER the activation (DAN context modules,
 * net/danet.py:912-918) or NULL. */
int danhip_conv2d_fwd(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* wf_packed, const float* bias,
                      void* y, int out_dtype, int relu, const uint16_t* residual, void* stream);

/* conv_relu + the 2x2 / stride-2 'same' max-pool that follows every VGG block (net/sfd_net.py:128-143) in one call:
 * y = relu(conv(x, w) + bias) [N,Ho,Wo,Cout] and pool_y = maxpool2x2(y) [N,ceil(Ho/2),ceil(Wo/2),Cout], both in the build's
 * 16-bit type.  3x3 kernels that own whole row pairs per wave pool in their epilogue; other shapes run the pool kernel. */
int danhip_conv2d_fwd_pool(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* wf_packed, const float* bias, uint16_t* y,
                           uint16_t* pool_y, void* stream);
/* The same calls that ALSO write the pool's 2-bit arg-max codes (pool_arg: [N*ceil(Ho/2)*ceil(Wo/2)][Cout/4] bytes, channel c in bits
 * 2(c%4).. of byte c/4, code = 2*dh + dw of the FIRST maximum of the window in row-major order - TF's MaxPoolGrad rule), from the epilogue
 * registers where the kernel pools there, from the pool kernel otherwise.  danhip_maxpool2x2_bwd_arg scatters the pooled gradient through
 * the codes: it reads a quarter-size gradient and 2 bits per element instead of the full-resolution activation (1.28 instead of 2.25
 * map-sized HBM passes).  pool_arg == NULL: the plain calls. */
int danhip_conv2d_fwd_pool_arg(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* wf_packed, const float* bias, uint16_t* y,
                               uint16_t* pool_y, uint8_t* pool_arg, void* stream);
int danhip_conv2d_fwd_relu_bits_arg(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* wf_packed, const float* bias, uint16_t* y,
                                    uint8_t* y_bits, uint16_t* pool_y, uint8_t* pool_bits, uint8_t* pool_arg, void* stream);
/* 1 when danhip_conv2d_fwd_pool may be called with y == NULL for this descriptor: only the pooled map is produced and the full-resolution
 * activation is never written (inference: nothing but the pool reads conv1_2's / conv2_2's output - 839 + 419 MB of stores per batch of
 * 16 at 640 x 640).  0: the pool is a separate kernel for this shape, y is needed. */
int danhip_conv2d_fwd_pool_only(const danhip_conv_desc* d);

/* dx = conv_transpose(dy, w) (* (relu_mask > 0) if relu_mask != NULL: fuses the ReLU backward of the layer
 * that produced x).  dy bf16 [N,Ho,Wo,Cout_pad8]; dx bf16 [N,H,W,Cin]. accumulate: dx += instead of = . */
int danhip_conv2d_bwd_data(const danhip_conv_desc* d, const uint16_t* dy, const uint16_t* wb_packed,
                           const uint16_t* relu_mask, uint16_t* dx, int accumulate, void* stream);

/* The same two calls with a caller-provided scratch buffer.  Maps with too few output tiles to fill the chip (the 40x40 ... 5x5 pyramid
 * levels; every level at 2-4 images per GPU, the per-rank shape of an 8-GPU strong-scaling run) otherwise walk K = kh*kw*Cin serially in a
 * handful of workgroups: with >= danhip_conv2d_workspace_bytes(d, which) bytes (which: 0 forward, 1 data gradient; 0 = the shape does not
 * split) K is split over workgroups, the fp32 partial outputs go to the scratch buffer and a second small kernel sums them and applies
 * the epilogue.  Results equal the single-pass form up to fp32 summation order.  ws == NULL behaves as the plain call. */
size_t danhip_conv2d_workspace_bytes(const danhip_conv_desc* d, int which);
int danhip_conv2d_fwd_ws(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* wf_packed, const float* bias, void* y,
                         int out_dtype, int relu, const uint16_t* residual, void* ws, size_t ws_bytes, void* stream);
int danhip_conv2d_bwd_data_ws(const danhip_conv_desc* d, const uint16_t* dy, const uint16_t* wb_packed, const uint16_t* relu_mask,
                              uint16_t* dx, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* The ReLU mask as one bit per element: bits[m][j] bit i = x[m][8j + i] > 0, rows of C/8 bytes (C % 8 == 0).  A data-gradient kernel that
 * keeps its tile's mask in LDS reads 1/16 of the bytes, and not from its epilogue: danhip_conv2d_bwd_data_takes_bits(d) says whether the
 * kernel chosen for descriptor d does (then call danhip_conv2d_bwd_data_bits with the bits of the conv's INPUT activation). */
int danhip_relu_bits(const uint16_t* x, uint8_t* bits, int64_t M, int32_t C, void* stream);
/* conv_relu (+ the block's fused 2x2 max-pool when pool_y != NULL) that also writes those bit masks for y (and pool_y) from its epilogue
 * registers, so the next convolution's data gradient needs no pass over the activation: danhip_conv2d_fwd_emits_bits(d, with_pool) == 1
 * where the forward kernel of descriptor d can (3x3 / stride-1 'same' on the 128-wide halo tiles, Cout % 128 == 0). */
int danhip_conv2d_fwd_emits_bits(const danhip_conv_desc* d, int with_pool);
int danhip_conv2d_fwd_relu_bits(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* wf_packed, const float* bias, uint16_t* y,
                                uint8_t* y_bits, uint16_t* pool_y, uint8_t* pool_bits, void* stream);
int danhip_conv2d_bwd_data_takes_bits(const danhip_conv_desc* d);
/* The data gradient of the SECOND layer (conv1_2: 3x3, 64 -> 64) with the FIRST layer's weight / bias gradient folded into it (round 6).  conv1_1 has
 * no data gradient (its input is the image), so the dX this call would store is read by nothing but conv1_1's weight gradient: the kernel keeps each
 * dX tile in LDS, multiplies it with the tile's patch of the 8-channel image x8 ([N,H,W,8], cin_real <= 4 real channels) and ADDS the result to
 * dw8 [3,3,cin_real,64] / db8 [64] (fp32, may be NULL) — dX never reaches HBM and the first layer's own weight-gradient launch disappears
 * (train_sfd.py's graph: net/sfd_net.py:128 conv1 block).  relu_bits = the bit mask of conv1_1's output (danhip_conv2d_bwd_data_bits).
 * danhip_conv2d_bwd_data_first_supported(d) == 1 where the kernel takes descriptor d (else: danhip_conv2d_bwd_data_bits + danhip_conv2d_bwd_weight). */
int danhip_conv2d_bwd_data_first_supported(const danhip_conv_desc* d);
int danhip_conv2d_bwd_data_bits_first(const danhip_conv_desc* d, const uint16_t* dy, const uint16_t* wb_packed, const uint8_t* relu_bits,
                                      const uint16_t* x8, int32_t cin_real, float* dw8, float* db8, void* stream);
int danhip_conv2d_bwd_data_bits(const danhip_conv_desc* d, const uint16_t* dy, const uint16_t* wb_packed, const uint8_t* relu_bits,
                                uint16_t* dx, int accumulate, void* stream);

/* Forward 1x1 / stride-1 convolution over the CHANNEL CONCATENATION of two NHWC tensors that is never written:
 *   y = relu([x1 | x2] . W + b),  d->Cin = c1 + c2,  wf_packed = the forward packing of the [1, 1, c1 + c2, Cout] kernel.
 * Replaces tf.concat + conv2d where the reference feeds a 1x1 from two maps; with a block-diagonal kernel it is two 1x1 convolutions of
 * different inputs written side by side into one map - DAN's stage-2 input mix (/root/reference/net/danet.py:944-950:
 * concat([conv1x1(stop_gradient(stage1), C/3), conv1x1(feature, C - C/3)]), whose ragged 85 / 171 column counts no tile fits).
 * x1 holds c1 channels, x2 holds Cin - c1, both with pixel pitch src_pitch elements; c1, Cin - c1 and Cout multiples of 64.
 * _supported(): 1 when the streaming GEMM takes this shape (else concatenate on the host side and call danhip_conv2d_fwd). */
int danhip_conv2d_fwd_concat2_supported(const danhip_conv_desc* d, int32_t c1, int32_t src_pitch);
int danhip_conv2d_fwd_concat2(const danhip_conv_desc* d, const uint16_t* x1, const uint16_t* x2, int32_t c1, int32_t src_pitch,
                              const uint16_t* wf_packed, const float* bias, uint16_t* y, int relu, void* stream);

/* Channel-slice views (round 4; net/danet.py:842-918: every branch of the context block is a channel slice of a wider tensor - the fused
 * input 1x1's output, the concat buffer).  A slice [.., c0 : c0 + C] of an NHWC tensor whose pixels are `ld` elements apart is its base
 * pointer + c0 and pitch ld: x_pitch / y_pitch are the pitches of the call's input / output operand (forward: x, y; data gradient: dy,
 * dx; weight gradient: x, dy), aux_pitch that of the data gradient's relu_mask (0 = dx's channel count).  Multiples of 8 elements.
 * These calls run on the streaming GEMM / flat-M kernels and, for 3x3 / stride-1 64 -> 64 on maps the 8 x 32 tiles cover well, on the
 * register-resident 64 -> 64 kernel (the halo kernel addresses dense tensors); the weight gradient also on the row-streaming kernel;
 * 16-bit output, no residual.
 * relu_channels (forward): ReLU applies to output channels < relu_channels only (a fused block of 1x1 convolutions whose last columns
 * stay linear); pass Cout for a plain conv_relu, anything with relu = 0 for none. */
typedef struct { int32_t x_pitch, y_pitch, aux_pitch; } danhip_conv_pitch;
int danhip_conv2d_fwd_strided(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* wf_packed, const float* bias, uint16_t* y,
                              int relu, int32_t relu_channels, const danhip_conv_pitch* pitch, void* ws, size_t ws_bytes, void* stream);
int danhip_conv2d_bwd_data_strided(const danhip_conv_desc* d, const uint16_t* dy, const uint16_t* wb_packed, const uint16_t* relu_mask,
                                   uint16_t* dx, int accumulate, const danhip_conv_pitch* pitch, void* ws, size_t ws_bytes, void* stream);
int danhip_conv2d_bwd_weight_strided(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* dy, float* dw_hwio, float* db,
                                     int32_t cin_real, const danhip_conv_pitch* pitch, void* ws, size_t ws_bytes, void* stream);

/* dw_hwio fp32 [kh,kw,Cin,Cout] += sum_pixels x (x) dy   (atomic fp32 accumulation: zero it first).
 * db (optional) fp32 [Cout] += sum_pixels dy  (bias gradient, computed by the same kernel: no extra pass over dy).
 * cin_real: number of leading input channels that exist in dw (dw is [kh,kw,cin_real,Cout]). */
int danhip_conv2d_bwd_weight(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* dy, float* dw_hwio, float* db,
                             int32_t cin_real, void* stream);
/* The same with a caller-provided scratch buffer: where danhip_conv2d_bwd_weight_workspace_bytes(d) > 0 and `ws` holds at least that many
 * bytes, the split partial sums leave the kernel as plain coalesced stores and a second small kernel combines them into dw_hwio (+=),
 * instead of fp32 atomics (4-5x the bytes per second; the atomic tail dominated the launch at <= 4 images per GPU).  ws == NULL: atomics
 * (deterministic mode: every descriptor has a workspace size, and a call without that workspace is DANHIP_EINVAL).
 * Limitation: the query sees the descriptor alone and answers for DENSE pitches (x_pitch = Cin, y_pitch = Cout rounded up to 8).  In
 * deterministic mode a danhip_conv2d_bwd_weight_strided call whose pitches make the selection fall to another kernel family (a pitch above
 * 65535 elements declines the row-streaming kernel, a first-layer image that is not dense declines its kernel and changes the generic
 * kernel's split count) may need a different size, which cannot be asked for: such a call returns DANHIP_EINVAL (every launcher checks
 * ws_bytes against its own need; nothing is overrun).  Pitches of channel-slice views of tensors up to 65535 channels wide are unaffected. */
size_t danhip_conv2d_bwd_weight_workspace_bytes(const danhip_conv_desc* d);
int danhip_conv2d_bwd_weight_ws(const danhip_conv_desc* d, const uint16_t* x, const uint16_t* dy, float* dw_hwio, float* db,
                                int32_t cin_real, void* ws, size_t ws_bytes, void* stream);

/* In place: dy *= (y > 0) (ReLU backward) when y != NULL; db[c] += sum over pixels of the masked dy.
 * dy bf16 [M, C]; y bf16 [M, C] or NULL; db fp32 [C] or NULL. */
int danhip_relu_bwd_bias_grad(uint16_t* dy, const uint16_t* y, float* db, int64_t M, int32_t C, void* stream);
/* Deterministic mode: db through ws (>= danhip_reduce_workspace_bytes(M, C) bytes; may be NULL when db is). */
int danhip_relu_bwd_bias_grad_ws(uint16_t* dy, const uint16_t* y, float* db, int64_t M, int32_t C, void* ws, size_t ws_bytes, void* stream);

/* Kernel-instance label a forward (which=0) / data-gradient (which=1; which=5 when relu_mask is passed) / forward-with-fused-pool
 * (which=4, danhip_conv2d_fwd_pool) call of this descriptor launches (the demangled name rocprofv3 reports) — lets bench.py attribute
 * measured time to a kernel.  The answer is for the *_ws calls given their scratch buffer; which | 16: for the plain calls (no split-K). */
const char* danhip_conv_kernel_label(const danhip_conv_desc* d, int which);
/* Same for the weight-gradient call of this descriptor. */
const char* danhip_conv_wgrad_kernel_label(const danhip_conv_desc* d);
/* Label of the convolution kernel instance (forward, data gradient or weight gradient) most recently launched on the calling thread;
 * "" before the first launch.  The two functions above predict it from a descriptor; this one reports what ran. */
const char* danhip_conv_last_launch_label(void);

/* ------------------------------------------------------------------------------------------------
 * HBM-bound layer kernels (bf16 NHWC, 16-byte vectors, wave reductions).
 * ------------------------------------------------------------------------------------------------ */
/* tf.layers.max_pooling2d([2,2],[2,2],'same') — net/sfd_net.py:132.  y [N,ceil(H/2),ceil(W/2),C]; C % 8 == 0.
 * Backward: the gradient goes to the FIRST maximal element in window order (TF CPU kernel). */
int danhip_maxpool2x2_fwd(const uint16_t* x, uint16_t* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int danhip_maxpool2x2_bwd(const uint16_t* x, const uint16_t* dy, uint16_t* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                          int accumulate, void* stream);
/* The 2 x 2 max-pool with its arg-max codes (layout: danhip_conv2d_fwd_pool_arg) and the backward through them: dx (+)= scatter(dy, arg). */
int danhip_maxpool2x2_fwd_arg(const uint16_t* x, uint16_t* y, uint8_t* arg, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int danhip_maxpool2x2_bwd_arg(const uint8_t* arg, const uint16_t* dy, uint16_t* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                              int accumulate, void* stream);
/* VGG16Backbone.l2_normalize — net/sfd_net.py:68-79: y = x * rsqrt(max(sum_c x^2, 1e-10)) * gamma_c.
 * x,y bf16 [M,C], gamma fp32 [C], C in {64,128,256,512,1024}.  bwd: dgamma += (atomic fp32), dx (=|+= if accumulate);
 * relu_mask: x is a ReLU output, so dx is also multiplied by (x > 0) (the producer's ReLU backward folded in). */
int danhip_l2norm_fwd(const uint16_t* x, const float* gamma, uint16_t* y, int64_t M, int32_t C, void* stream);
int danhip_l2norm_bwd(const uint16_t* x, const float* gamma, const uint16_t* dy, uint16_t* dx, float* dgamma, int64_t M,
                      int32_t C, int accumulate, int relu_mask, void* stream);
/* Deterministic mode: dgamma through ws (>= danhip_reduce_workspace_bytes(M, C) bytes); dx is bit-identical to the plain call in both modes. */
int danhip_l2norm_bwd_ws(const uint16_t* x, const float* gamma, const uint16_t* dy, uint16_t* dx, float* dgamma, int64_t M,
                         int32_t C, int accumulate, int relu_mask, void* ws, size_t ws_bytes, void* stream);
/* Gradient junction of a tapped map x [N,H,W,C] (C in {64,128,256,512}) that feeds an L2 norm AND a 2 x 2 max-pool: one pass that equals
 * danhip_l2norm_bwd(x, gamma, dy, dx, dgamma, N*H*W, C, accumulate, relu_mask) followed by danhip_maxpool2x2_bwd_arg(arg, pooled_dy, dx, ...,
 * accumulate = 1) - or, with pool_first, the scatter (accumulate) followed by the L2 norm (accumulate = 1) - with dx written once.  dx is
 * bit-identical to the two calls (the 16-bit rounding between them is reproduced); dgamma agrees up to fp32 summation order. */
int danhip_l2norm_bwd_pool_scatter(const uint16_t* x, const float* gamma, const uint16_t* dy, const uint8_t* arg, const uint16_t* pooled_dy,
                                   uint16_t* dx, float* dgamma, int32_t N, int32_t H, int32_t W, int32_t C, int accumulate, int relu_mask,
                                   int pool_first, void* stream);
/* Deterministic mode: dgamma through ws (>= danhip_reduce_workspace_bytes(N*H*W, C) bytes). */
int danhip_l2norm_bwd_pool_scatter_ws(const uint16_t* x, const float* gamma, const uint16_t* dy, const uint8_t* arg, const uint16_t* pooled_dy,
                                      uint16_t* dx, float* dgamma, int32_t N, int32_t H, int32_t W, int32_t C, int accumulate, int relu_mask,
                                      int pool_first, void* ws, size_t ws_bytes, void* stream);
/* tf.image.resize_bilinear(up, size(lateral)) (TF1 legacy mapping src = dst*(in/out), align_corners=False) fused with the
 * LFPN lateral add: out = lateral + resize(up) (lateral may be NULL) — net/pb_net.py:209-217, net/danet.py:363-371.
 * up bf16 [N,Hi,Wi,C], lateral/out bf16 [N,Ho,Wo,C], C % 8 == 0.  bwd: d_up (=|+= if accumulate) from d_out (the lateral's
 * gradient is d_out itself). */
int danhip_resize_bilinear_add_fwd(const uint16_t* up, const uint16_t* lateral, uint16_t* out, int32_t N, int32_t Hi, int32_t Wi,
                                   int32_t Ho, int32_t Wo, int32_t C, void* stream);
int danhip_resize_bilinear_add_bwd(const uint16_t* dout, uint16_t* dup, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                   int32_t C, int accumulate, void* stream);
/* tf.layers.average_pooling2d((2,2), 1, 'same') — net/danet.py:854: pad (0,1), divisor = number of valid taps. */
int danhip_avgpool2x2s1_same_fwd(const uint16_t* x, uint16_t* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* x_mask (may be NULL): the pooled tensor when it is a ReLU output — dx is then multiplied by (x > 0). */
int danhip_avgpool2x2s1_same_bwd(const uint16_t* dy, const uint16_t* x_mask, uint16_t* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                 int accumulate, void* stream);
/* The residual sum of the DAN context block (net/danet.py:913-918), y = relu(conv(hyper)) + features: out = a + b over n 16-bit elements
 * (n % 8 == 0), and its backward in ONE pass over dy: dr = dy * (r > 0) (the conv's ReLU backward, materialised for its two gradient
 * kernels) and, when dx != NULL, dx (+)= dy * (x_mask > 0, or all when x_mask == NULL) (the skip path into the producer's gradient). */
int danhip_add16(const uint16_t* a, const uint16_t* b, uint16_t* out, int64_t n, void* stream);
int danhip_residual_bwd(const uint16_t* dy, const uint16_t* r, const uint16_t* x_mask, uint16_t* dr, uint16_t* dx, int accumulate, int64_t n,
                        void* stream);
/* The same pool on channel-slice views (pitches in elements, multiples of 8), optionally followed by ReLU, and its backward (dy -> dx,
 * overwritten; a ReLU's backward is the caller's: dy arrives masked).  The DAN context block (net/danet.py:854-861) runs branch 2's 1x1
 * convolution IN FRONT of the (linear) pool, on the 64 output channels instead of the C input channels. */
int danhip_avgpool2x2s1_same_fwd_strided(const uint16_t* x, int32_t x_pitch, uint16_t* y, int32_t y_pitch, int32_t N, int32_t H, int32_t W,
                                         int32_t C, int relu, void* stream);
int danhip_avgpool2x2s1_same_bwd_strided(const uint16_t* dy, int32_t y_pitch, uint16_t* dx, int32_t x_pitch, int32_t N, int32_t H, int32_t W,
                                         int32_t C, void* stream);
/* Backward of tf.concat(axis=-1) / of a residual add (net/danet.py:911-918), one input at a time:
 *   out[m][c] (+)= (mask == NULL || mask[m*ldm + c] > 0) ? dy[m*ldy + c0 + c] : 0      for c < C,   out[m][c] = 0 for C <= c < Cpad (first write)
 * out rows have Cpad (>= C, multiple of 8) elements: the channel-padded gradient layout danhip_conv2d_bwd_* take for a ragged Cout. */
int danhip_slice_deliver(const uint16_t* dy, int32_t ldy, int32_t c0, int32_t C, const uint16_t* mask, int32_t ldm, uint16_t* out, int32_t Cpad,
                         int accumulate, int64_t M, void* stream);
/* tf.layers.batch_normalization over the channel axis of [M,C] (M = N*H*W) — the conv_bn_relu / bn_relu / conv_bn surface of
 * net/sfd_net.py:91-119 (momentum 0.997, eps 1e-5).  Training: batch statistics (biased variance), optional moving-average
 * update, optional fused ReLU; workspace = 2*C doubles (4*C floats, 8-byte aligned).  Inference: caller passes mean and rstd = rsqrt(var + eps).
 * Backward: dgamma, dbeta are overwritten. */
int danhip_batchnorm_fwd_train(const uint16_t* x, const float* gamma, const float* beta, uint16_t* y, float* save_mean,
                               float* save_rstd, float* moving_mean, float* moving_var, int64_t M, int32_t C, float eps,
                               float momentum, int relu, float* workspace, void* stream);
int danhip_batchnorm_fwd_infer(const uint16_t* x, const float* gamma, const float* beta, const float* mean, const float* rstd,
                               uint16_t* y, int64_t M, int32_t C, int relu, void* stream);
int danhip_batchnorm_bwd(const uint16_t* x, const uint16_t* dy, const float* gamma, const float* save_mean, const float* save_rstd,
                         uint16_t* dx, float* dgamma, float* dbeta, int64_t M, int32_t C, void* stream);
/* preprocess_for_eval arithmetic (preprocessing/dan_preprocessing.py:55-57,755-758): uint8 RGB [npix,3] ->
 * bf16 [npix,8] = (B-103.94, G-116.78, R-123.68, 0,0,0,0,0). */
int danhip_preprocess_u8(const uint8_t* img_rgb, uint16_t* out, int64_t npix, void* stream);
/* fp32 [rows,c_src] -> bf16 [rows,c_dst] zero padded (gradient of the fp32 head outputs / of ragged-Cout convs).
 * relu_y (optional, bf16 [rows,c_src]): the layer's ReLU output — elements where it is <= 0 are zeroed (ReLU backward applied on
 * the unpadded layout, before the channel padding). */
int danhip_cast_pad_f32_to_bf16(const float* src, const uint16_t* relu_y, uint16_t* dst, int64_t rows, int32_t c_src, int32_t c_dst,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Detection heads glue, hard-negative mining, losses, optimizer (fp32 / int32).
 * ------------------------------------------------------------------------------------------------ */
/* Max-out + reshape_pred for one level with one anchor per cell (net/sfd_net.py:175-216; train_sfd.py:293-304):
 * h fp32 [B*HW, Ch], channels [loc(4) | neg(nneg) | pos(npos)] -> loc [B,A,4], cls [B,A,2] rows [off, off+HW). */
int danhip_head_split_fwd(const float* h, float* loc, float* cls, int32_t B, int32_t HW, int32_t Ch, int32_t nneg, int32_t npos,
                          int32_t A, int32_t anchor_offset, void* stream);
int danhip_head_split_bwd(const float* h, const float* dloc, const float* dcls, float* dy, int32_t B, int32_t HW, int32_t Ch,
                          int32_t nneg, int32_t npos, int32_t A, int32_t anchor_offset, void* stream);
/* ABI version 9: all pyramid levels of the detection heads in ONE launch each way.  The level table travels by value as a kernel
 * argument (nothing is copied to the device per call), at most DANHIP_HEADS_MAX_LEVELS entries.  The launchers refuse
 * (DANHIP_EINVAL) more levels than that, Ch != 4 + nneg + npos, anchor ranges [off, off + HW) that do not tile [0, A) without
 * overlap, a null or misaligned pointer (h, dy, loc, dloc: 16 bytes; cls, dcls: 8 bytes - what a batch slice of them keeps) and, for
 * the gradient, co_pad < Ch or co_pad % 8 != 0.
 *   danhip_heads_split_fwd: per level exactly danhip_head_split_fwd (same max-out arithmetic, same destinations).
 *   danhip_heads_grad_pad:  per level the composition danhip_head_split_bwd -> danhip_cast_pad_f32_to_bf16 (no ReLU operand):
 *     reads h, dloc [B,A,4], dcls [B,A,2]; writes the level's channel-padded 16-bit dY [B*HW, co_pad] (pad columns zero),
 *     bit-identical to the two calls; the fp32 dY exists in registers only. */
#define DANHIP_HEADS_MAX_LEVELS 8
typedef struct danhip_head_level {
  const float* h;  /* head map of the level, fp32 [B*HW, Ch] */
  uint16_t* dy;    /* danhip_heads_grad_pad: destination, 16 bit [B*HW, co_pad]; ignored by danhip_heads_split_fwd */
  int32_t HW, Ch, nneg, npos;
  int32_t off;     /* anchor offset of the level in [0, A) */
  int32_t co_pad;  /* danhip_heads_grad_pad: channels per row of dy */
} danhip_head_level;
int danhip_heads_split_fwd(const danhip_head_level* levels, int32_t nlevels, float* loc, float* cls, int32_t B, int32_t A, void* stream);
int danhip_heads_grad_pad(const danhip_head_level* levels, int32_t nlevels, const float* dloc, const float* dcls, int32_t B, int32_t A,
                          void* stream);
/* Per-image hard-negative mining (train_sfd.py:350-384, train_dan.py:286-324): score = label==0 ? -softmax(cls)[0] : -1;
 * k = min(int(ratio*n_pos), n_neg) (at_least_one: max(k,1)); thr[b] = exact k-th largest score of row b (radix select),
 * +inf when k == 0.  cls fp32 [B,A,2], labels int32 [B,A] in {1,0,-1}; score [B,A], counts int32 [B,2], thr [B], k_out [B]. */
int danhip_hard_neg_select(const float* cls, const int32_t* labels, float* score, int32_t* counts, float* thr, int32_t* k_out,
                           int32_t B, int32_t A, float negative_ratio, int at_least_one, void* stream);
/* acc4 = [sum CE over selected, #selected, sum smooth-L1 over positives, #positives]; sel uint8 [B,A] (0/1 neg/2 pos)
 * (train_sfd.py:386-417).  bwd: dcls = (softmax-onehot)*ce_scale/#selected, dloc = dSmoothL1*loc_scale/#positives. */
int danhip_detection_loss_fwd(const float* cls, const float* loc, const int32_t* labels, const float* loc_targets,
                              const float* score, const float* thr, uint8_t* sel, float* acc4, int32_t B, int32_t A,
                              void* stream);
/* Deterministic mode: the four sums through ws (>= DANHIP_LOSS_WS_BYTES). */
int danhip_detection_loss_fwd_ws(const float* cls, const float* loc, const int32_t* labels, const float* loc_targets,
                                 const float* score, const float* thr, uint8_t* sel, float* acc4, int32_t B, int32_t A,
                                 void* ws, size_t ws_bytes, void* stream);
int danhip_detection_loss_bwd(const float* cls, const float* loc, const float* loc_targets, const uint8_t* sel,
                              const float* acc4, float* dcls, float* dloc, float ce_scale, float loc_scale, int32_t B,
                              int32_t A, void* stream);
/* Streaming classification accuracy, the reference's tf.metrics.accuracy over final_mask (train_sfd.py:383-395, train_dan.py:454-462):
 * over the anchors with sel != 0 (as danhip_detection_loss_fwd wrote them), counts[0] += #(argmax(cls, -1) == clip(label, 0, 2)) and
 * counts[1] += their number.  argmax takes the first index on equal logits (tf.argmax).  counts int64 [2] is ADDED to, never cleared: the
 * metric is a running total over all steps; the caller zeroes it once.  Integer sums, so the result has the same bits in deterministic
 * mode and out of it; no host read-back, no synchronisation.  B * A must not exceed 2^31 - 1 (32-bit indices): DANHIP_EINVAL.
 * Launch shape: workgroups of DANHIP_CLS_ACCURACY_THREADS, at most DANHIP_CLS_ACCURACY_MAX_BLOCKS of them (beyond their product a
 * workgroup loops). */
#define DANHIP_CLS_ACCURACY_THREADS 256
#define DANHIP_CLS_ACCURACY_MAX_BLOCKS 1024
int danhip_cls_accuracy(const float* cls, const int32_t* labels, const uint8_t* sel, int64_t* counts, int32_t B, int32_t A, void* stream);
/* Fused multi-tensor momentum SGD over flat fp32 buffers (train_sfd.py:419-447): for element i of segment s
 * (seg_starts[s] <= i < seg_starts[s+1]): g' = (g*grad_scale + wd_coef[s]*w) * gmult[s]; v = m*v + g'; w -= lr*v.
 * l2_out (optional) += sum 0.5*wd_coef[s]*w^2 (the L2 loss term at the pre-update weights).
 * Layout contract: buffers 16-byte aligned, every seg_starts[s] and total a multiple of 4 (the trainer pads each variable to 64
 * elements with zeros, which stay zero), so the kernel moves float4s that never straddle two variables. */
int danhip_sgd_momentum_flat(float* w, const float* g, float* v, const int64_t* seg_starts, const float* gmult,
                             const float* wd_coef, int32_t nseg, int64_t total, float lr, float momentum, float grad_scale,
                             float* l2_out, void* stream);
/* Deterministic mode: l2_out through ws (>= DANHIP_SGD_WS_BYTES): the workgroup sums (grid rounded up to a multiple of 64, idle workgroups
 * store 0) are reduced as [rows][64] -> 64 column sums -> one sum, both by the ordered reduction.  w and v are elementwise: same bits in both modes. */
int danhip_sgd_momentum_flat_ws(float* w, const float* g, float* v, const int64_t* seg_starts, const float* gmult,
                                const float* wd_coef, int32_t nseg, int64_t total, float lr, float momentum, float grad_scale,
                                float* l2_out, void* ws, size_t ws_bytes, void* stream);
/* The same update under a DYNAMIC loss scale kept on the device (fp16 build; no host round trip, capturable in a hipGraph).
 * loss_scale_state: 4 floats {scale, clean steps so far, growth interval, scratch flag}.  One call = non-finite check of g; the
 * update with g / scale, skipped entirely (w, v untouched) when the check fired; then torch.cuda.amp.GradScaler's rule: scale x0.5
 * after a skipped step, x2 after `interval` clean ones.  The loss terms multiply their gradients by state[0] on the device. */
int danhip_sgd_momentum_flat_dynamic(float* w, const float* g, float* v, const int64_t* seg_starts, const float* gmult,
                                     const float* wd_coef, int32_t nseg, int64_t total, float lr, float momentum,
                                     float* loss_scale_state, float* l2_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Anchor / box index-compare kernels (fp32 + int32, bit-exact vs the oracle; utility/anchor_manipulator.py).
 * ------------------------------------------------------------------------------------------------ */
/* generate_anchors_by_offset + center2point (anchor_manipulator.py:125-127,163-198) for one level, order (y,x,depth). */
int danhip_anchors_generate(float* ymin, float* xmin, float* ymax, float* xmax, const float* anchor_h, const float* anchor_w,
                            int32_t depth, int32_t layer_h, int32_t layer_w, float stride, float offset_h, float offset_w,
                            int32_t out_offset, void* stream);
/* iou_matrix (anchor_manipulator.py:24-52), optionally multiplied by inside_mask[a] (encode_anchors :287). [A,G]. */
int danhip_iou_matrix(const float* ymin, const float* xmin, const float* ymax, const float* xmax, const uint8_t* inside_mask,
                      const float* gt_boxes, float* overlaps, int32_t A, int32_t G, void* stream);
size_t danhip_match_workspace_bytes(int32_t A, int32_t G);
/* do_dual_max_match (anchor_manipulator.py:54-105, gt_max_first=True). */
int danhip_dual_max_match(const float* overlaps, int32_t A, int32_t G, float low_thres, float high_thres, int ignore_between,
                          int32_t* match_indices, float* match_scores, void* workspace, size_t workspace_bytes, void* stream);
/* SmallMiningMatch custom op (cpp/ExtraLib/small_mining_match.cc:31-54,68-222): same inputs, attrs, outputs. */
int danhip_small_mining_match(const float* overlaps, int32_t A, int32_t G, float negative_low_thres, float negative_high_thres,
                              float positive_thres, int32_t min_match, float stop_positive_thres, int32_t* match_indices,
                              float* match_scores, void* workspace, size_t workspace_bytes, void* stream);
/* Tail of encode_anchors / encode_pa_anchors after matching (anchor_manipulator.py:294-326, :358-387). */
int danhip_encode_anchors(const float* ymin, const float* xmin, const float* ymax, const float* xmax, const float* gt_boxes,
                          const int32_t* match_indices, float* targets, int32_t* labels, float* matched_gt, int32_t A,
                          float ps0, float ps1, float ps2, float ps3, float scale, void* stream);
/* anchor_encoder_fn over a whole batch in one call (the reference maps encode_anchors / encode_pa_anchors per image inside tf.data:
 * train_sfd.py:206, train_dan.py:243-249; anchor_manipulator.py:275-387): IoU x inside_mask -> small_mining_match (match_mining=1:
 * negative_low_thres, ignore_thres, positive_thres, min_match, stop_positive_thres as the op's attrs) or do_dual_max_match
 * (match_mining=0: low=ignore_thres, high=positive_thres) -> encode.  gt_boxes [total_gt,4] is the concatenation of the images' gt rows,
 * gt_offsets [B+1] int32 (device) their row ranges; every image needs >= 1 row (the reference substitutes [[0,0,1,1]] for an empty
 * list, anchor_manipulator.py:286 / :347).  match_* = anchors used for matching (NULL: the encode anchors; encode_pa_anchors passes the
 * shrunk set and `scale`).  Outputs targets [B,A,4], labels [B,A] in {1,0,-1}, scores [B,A], matched_gt [B,A,4] or NULL.
 * Images are independent, so the B sequential hard-face compensation passes run side by side (one workgroup each). */
size_t danhip_encode_anchors_batched_workspace_bytes(int32_t B, int32_t A, int32_t total_gt);
int danhip_encode_anchors_batched(const float* ymin, const float* xmin, const float* ymax, const float* xmax, const float* match_ymin,
                                  const float* match_xmin, const float* match_ymax, const float* match_xmax, const uint8_t* inside_mask,
                                  const float* gt_boxes, const int32_t* gt_offsets, int32_t B, int32_t A, int32_t total_gt, int32_t max_gt,
                                  int32_t match_mining, float negative_low_thres, float ignore_thres, float positive_thres,
                                  int32_t min_match, float stop_positive_thres, float ps0, float ps1, float ps2, float ps3, float scale,
                                  float* targets, int32_t* labels, float* scores, float* matched_gt, void* workspace,
                                  size_t workspace_bytes, void* stream);
/* batch_decode_anchors / decode_anchors (anchor_manipulator.py:389-424). pred [B,A,4] -> boxes [B,A,4]. */
int danhip_decode_anchors(const float* pred, const float* ymin, const float* xmin, const float* ymax, const float* xmax,
                          float* boxes, int32_t B, int32_t A, float ps0, float ps1, float ps2, float ps3, void* stream);

/* Face score of two-way logits: score[i] = softmax(cls[i, 0:2])[1] (tf.nn.softmax(cls_pred)[:, -1]: eval_dan.py:356,371, eval_sfd.py:281) and /
 * or the easy-anchor mask (score > threshold) as int32 (train_dan.py:438-439, eval_dan.py:386).  cls fp32 [n, 2]; score / mask [n], either
 * may be NULL. */
int danhip_face_scores(const float* cls, float* score, int32_t* mask, float threshold, int64_t n, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Deformable convolution (cpp/Deform: DeformConvOp deform_conv.cc:51-167,392-535; DeformConvBackpropOp :170-189,635-771;
 * Python names utility/custom_op.py:62-63).  The reference computes, per sample, deformable_im2col + GEMM; here the
 * im2col is danhip_deform_sample_fwd (batched, NHWC bf16, sampling rules of deform_conv.cu:91-126,229-275) and the GEMM is
 * danhip_conv2d_{fwd,bwd_data,bwd_weight} run as a 1x1 convolution over S [N,Ho,Wo,kh*kw*C] with the OIHW filter variable
 * viewed as HWIO [1,1,kh*kw*C,Cout] (k = tap*C + c).  Backward: dS from danhip_conv2d_bwd_data, then
 * danhip_deform_sample_bwd = deformable_col2im_coord (d_offsets) + deformable_col2im (dx; fp32 atomics as the reference).
 * offsets: NHWC [N,Ho,Wo,dg*2*kh*kw], channel (g*kh*kw + tap)*2 + {0: dh, 1: dw} (deform_conv.cu:251-259) — the NHWC
 * transpose of the reference's NCHW offset tensor.  SAME padding from the undilated kernel (deform_conv.cc:473-479).
 * ------------------------------------------------------------------------------------------------ */
int danhip_deform_sample_fwd(const uint16_t* x, const uint16_t* offsets, uint16_t* S, int32_t N, int32_t H, int32_t W, int32_t C,
                             int32_t kh, int32_t kw, int32_t stride, int32_t dilation, int32_t deformable_group, void* stream);
/* workspace: at least (N*H*W*C + 64) * sizeof(float) bytes = danhip_deform_sample_bwd_workspace_bytes (fp32 scatter target + the
 * far-corner statistic that selects the gather or the scatter form on the device).  ABI version 2 (danhip_version): the call takes
 * workspace_bytes and returns DANHIP_EWORKSPACE for a smaller buffer (version 1 took no size and sized the buffer N*H*W*C floats). */
size_t danhip_deform_sample_bwd_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C);
int danhip_deform_sample_bwd(const uint16_t* x, const uint16_t* offsets, const uint16_t* dS, uint16_t* dx, uint16_t* d_offsets,
                             int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride, int32_t dilation,
                             int32_t deformable_group, int accumulate, float* workspace, size_t workspace_bytes, void* stream);

/* DeformConvOp / DeformConvBackpropOp as single calls (the bindings custom_op.py:62-63 would make): same tensors and attrs as
 * the TF ops (strides / rates collapsed to one int each, num_groups = 1 as every call site uses), NHWC bf16, all samples in
 * one batch.  The im2col buffer lives in the workspace for the duration of the call only (deform_conv.cc:497-503
 * allocate_temp); the backward re-runs im2col as the reference does (:744-748) instead of keeping it from the forward.
 *   filter : the OIHW variable [Cout,C,kh,kw] viewed as HWIO [1,1,kh*kw*C,Cout] (k = tap*C + c) and packed with
 *            danhip_pack_conv_weight for the 1x1 descriptor {N,Ho,Wo,kh*kw*C -> Cout}: wf_packed (forward), wb_packed (backward).
 *   dw     : fp32 [kh*kw*C, Cout] in that same view, ACCUMULATED (zero it first); db fp32 [Cout] accumulated, or NULL.
 *   dy     : bf16 [N,Ho,Wo,Cout] gradient w.r.t. the op's output (after the caller's ReLU backward if relu was fused), Cout % 8 == 0.
 *   dx = | += (accumulate_dx) bf16 [N,H,W,C]; d_offsets bf16 like offsets (overwritten). */
size_t danhip_deform_conv_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride, int backward);
/* 1 when danhip_deform_conv_fwd runs this shape as ONE kernel (csrc/deform_fused.hip: 3x3 taps, C / deformable_group == 64, Cout in
 * {64, 128, 256}) — sampling feeds the GEMM through LDS.  The forward then takes workspace = NULL (no column buffer exists at all:
 * inference), or a workspace of danhip_deform_conv_workspace_bytes(.., 0) into which the kernel ALSO writes the column buffer for a caller
 * that keeps it for danhip_deform_conv_bwd_with_col.  Other shapes: sampling kernel + GEMM, workspace required. */
int danhip_deform_conv_fused(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride, int32_t deformable_group);
int danhip_deform_conv_fwd(const uint16_t* x, const uint16_t* wf_packed, const float* bias, const uint16_t* offsets, uint16_t* y,
                           int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                           int32_t dilation, int32_t deformable_group, int relu, void* workspace, size_t workspace_bytes, void* stream);
int danhip_deform_conv_bwd(const uint16_t* x, const uint16_t* wb_packed, const uint16_t* offsets, const uint16_t* dy, uint16_t* dx,
                           uint16_t* d_offsets, float* dw, float* db, int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout,
                           int32_t kh, int32_t kw, int32_t stride, int32_t dilation, int32_t deformable_group, int accumulate_dx,
                           void* workspace, size_t workspace_bytes, void* stream);
/* Same, with the im2col buffer that danhip_deform_conv_fwd left at the start of ITS workspace (kept alive by the caller; same x and
 * offsets): skips the reference's re-im2col (deform_conv.cc:744-748) — on a 288 GB part the 9x-activation buffer is cheaper to keep
 * than to regenerate.  col_saved = NULL behaves as danhip_deform_conv_bwd. */
int danhip_deform_conv_bwd_with_col(const uint16_t* x, const uint16_t* wb_packed, const uint16_t* offsets, const uint16_t* dy,
                                    const uint16_t* col_saved, uint16_t* dx, uint16_t* d_offsets, float* dw, float* db, int32_t N,
                                    int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                                    int32_t dilation, int32_t deformable_group, int accumulate_dx, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* Same, with the input gradient handed over the way the convolutions hand theirs to the layer below: relu_x != 0 multiplies it by (x > 0)
 * - x is then a ReLU output (DAN-Deform: the 1x1 'down' convolution, /root/reference/net/danet_deform.py:267-290) and its ReLU backward is
 * folded into this call - before accumulate_dx adds what dx already holds (the offset convolution's contribution). */
int danhip_deform_conv_bwd_deliver(const uint16_t* x, const uint16_t* wb_packed, const uint16_t* offsets, const uint16_t* dy,
                                   const uint16_t* col_saved, uint16_t* dx, uint16_t* d_offsets, float* dw, float* db, int32_t N,
                                   int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                                   int32_t dilation, int32_t deformable_group, int accumulate_dx, int relu_x, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DynamicAnchorRouting custom op (cpp/ExtraLib/dynamic_anchor_routing.cc:32-65 op def, :188-518 kernel; Python name
 * utility/custom_op.py:52) — same tensors / scalars / attrs as the TF op, plus a leading batch B (the reference maps the op
 * over the batch with tf.map_fn, train_dan.py:382): every array carries B images of N = feat_height*feat_width*anchor_depth
 * rows.  img_height / img_width of the TF op are unused by its kernel and therefore not taken.
 *   eval  (trainging=false, :328-408): mask_out in {0,1}, decode_out = stage-2 boxes decoded against the routed stage-1 box.
 *   train (trainging=true,  :203-327): mask_out in {1,0,-1}, decode_out = stage-2 regression targets.  The reference draws
 *          from std::mt19937(std::random_device) (not reproducible); here u(b,i) = splitmix64(seed, counter0 + b*N + i).
 *          counter_dev (nullable): device uint64 added to counter0 at run time, so a launch recorded in a hipGraph draws a
 *          fresh stream on every replay (the caller advances it with a device-side add).
 * ------------------------------------------------------------------------------------------------ */
size_t danhip_routing_workspace_bytes(int64_t N, int32_t B, int training);
int danhip_dynamic_anchor_routing_eval(const float* anchors, const float* gt_targets, const float* labels, const int32_t* mask_in,
                                       int64_t N, int32_t feat_height, int32_t feat_width, int32_t anchor_depth, int32_t feat_strides,
                                       int32_t B, int32_t* mask_out, float* decode_out, void* workspace, size_t workspace_bytes,
                                       void* stream);
int danhip_dynamic_anchor_routing_train(const float* anchors, const float* gt_targets, const float* labels, const int32_t* mask_in,
                                        int64_t N, int32_t feat_height, int32_t feat_width, int32_t anchor_depth, int32_t feat_strides,
                                        int32_t B, float thres, float ignore_thres, uint64_t seed, uint64_t counter0,
                                        const uint64_t* counter_dev, int32_t* mask_out, float* decode_out, void* workspace,
                                        size_t workspace_bytes, void* stream);

/* tf.image.non_max_suppression as used by utility/bbox_util.py:75-91: greedy over candidates already ordered by descending
 * score (stable), suppress when IoU > iou_threshold (raw areas, no +1, corners normalised by min/max).
 * boxes_sorted fp32 [B,K,4]; keep_idx int32 [B,max_out] = kept positions (-1 padded); num_keep int32 [B]. */
int danhip_nms(const float* boxes_sorted, int32_t B, int32_t K, int32_t max_out, float iou_threshold, int32_t* keep_idx,
               int32_t* num_keep, void* stream);

/* Stable descending arg-sort of one fp32 vector (the ordering step of utility/bbox_util.py:61-73 tf.nn.top_k and :75-91 ahead of
 * tf.image.non_max_suppression; eval_dan.py:255 `argsort()[::-1]` with ties_high_index_first = 1): idx_out int32 [n] = positions by
 * descending score, equal scores (+0 == -0) by ascending index (descending with ties_high_index_first).  Bitonic network on unique
 * 64-bit (score, index) keys; workspace = danhip_argsort_workspace_bytes(n) bytes (8 per element of the next power of two >= 8192). */
size_t danhip_argsort_workspace_bytes(int64_t n);
int danhip_argsort_desc_f32(const float* scores, int64_t n, int32_t ties_high_index_first, int32_t* idx_out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* DeformPSROIPool / DeformPSROIPoolGrad (cpp/Deform/deform_psroi_pooling_op.cc:37-97; utility/custom_op.py:93-126):
 * the TF op's tensors and attributes as they are — data fp32 NCHW [B,C,H,W], rois fp32 [R,5] (batch index, x1, y1, x2, y2), trans fp32
 * [R,2*num_classes,part_size,part_size] (NULL allowed when no_trans) -> top_data, mapping_channel (sample count) fp32
 * [R,output_dim,pooled_size,pooled_size]; num_classes = no_trans ? 1 : trans.dim(1)/2.  The backward zeroes data_diff [B,C,H,W] /
 * trans_diff and scatters with fp32 atomics like the reference.  Buffers 16-byte aligned. */
int danhip_deform_psroi_pool_fwd(const float* data, const float* rois, const float* trans, float* top_data, float* mapping_channel, int32_t R,
                                 int32_t C, int32_t H, int32_t W, int32_t output_dim, int32_t group_size, int32_t pooled_size, int32_t part_size,
                                 int32_t sample_per_part, float spatial_scale, float trans_std, int32_t no_trans, int32_t num_classes, void* stream);
int danhip_deform_psroi_pool_bwd(const float* top_diff, const float* mapping_channel, const float* data, const float* rois, const float* trans,
                                 float* data_diff, float* trans_diff, int32_t B, int32_t R, int32_t C, int32_t H, int32_t W, int32_t output_dim,
                                 int32_t group_size, int32_t pooled_size, int32_t part_size, int32_t sample_per_part, float spatial_scale,
                                 float trans_std, int32_t no_trans, int32_t num_classes, void* stream);

/* tf.layers.max_pooling2d([3,3],[2,2],'same') — the ResNet stem's pool_1 (net/resnet_danet.py:129).
 * y [N,ceil(H/2),ceil(W/2),C]; backward routes each window's gradient to its first maximum (gather form, dx overwritten). */
int danhip_maxpool3x3s2_same_fwd(const uint16_t* x, uint16_t* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int danhip_maxpool3x3s2_same_bwd(const uint16_t* x, const uint16_t* dy, uint16_t* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                 void* stream);

/* --------------------------------------------------------------------------------------------------
 * Test-time pipeline of eval_dan.py / eval_sfd.py
 *   resize_u8_linear : cv2.resize(image, None, None, fx, fy, INTER_LINEAR) of eval_dan.py:96-97 on an 8-bit HWC image
 *                      (generic fixed-point path of OpenCV); Ho/Wo = round-half-even(H*fy / W*fx), computed by the caller.
 *   bbox_vote        : eval_dan.py:201-241.  det float64 [B,Nmax,5] rows (xmin,ymin,xmax,ymax,score) in the order of
 *                      det[:,4].argsort()[::-1] (:202-203), counts int32 [B]; IoU with +1, merge when >= iou_threshold,
 *                      clusters of one dropped, float64 sums, float32 results.  out fp32 [B,max_out,5], num_out int32 [B].
 * ------------------------------------------------------------------------------------------------ */
int danhip_resize_u8_linear(const uint8_t* src, int32_t H, int32_t W, uint8_t* dst, int32_t Ho, int32_t Wo, int32_t C, double fx,
                            double fy, void* stream);
size_t danhip_bbox_vote_workspace_bytes(int32_t B, int32_t Nmax);
int danhip_bbox_vote(const double* det, const int32_t* counts, int32_t B, int32_t Nmax, double iou_threshold, int32_t max_out,
                     float* out, int32_t* num_out, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------------------
 * WIDER FACE evaluation (csrc/wider_eval_exact.hip; ABI 5): from the detections write_to_txt (eval_dan.py:243-261) would print to the
 * easy / medium / hard average precision, on the device.  The protocol (dan_amd/wider_eval.py states it in full), IEEE double in the
 * order written, no FMA contraction:
 *   1 scores -> (score - lo) / (hi - lo), lo / hi over every detection of every image (hi == lo: all 0);
 *   2 per image, detections by descending score, equal scores by ascending index;
 *   3 per image and subset: count_face += kept boxes; an image without detections or without boxes adds nothing else (its detections are
 *     NOT false positives); else each detection h takes the FIRST box j of maximum overlap (corners x + w, y + h; +1 convention); overlap
 *     >= iou_threshold: j not kept -> proposal[h] = -1, else the first such h turns recall[j] to 1 (a later one stays a false positive);
 *     pred_recall[h] = #{recall == 1} after h;
 *   4 thresholds t = 0..T-1, thr = 1 - (t+1)/T, r = last detection with score >= thr: curve[s][t] += (#{h <= r: proposal == 1},
 *     pred_recall[r]), summed over the images in integers;
 *   5 precision = curve[.][1] / curve[.][0] (0 where curve[.][0] == 0), recall = curve[.][1] / count_face, mrec = [0, recall, 1],
 *     mpre = [0, precision, 0] made non-increasing from the back, AP = sum over the steps of mrec, ascending; count_face == 0: AP = 0.
 * Layouts.  Ground truth as CSR: gt_offsets int32 [I+1], gt_boxes double [G,4] rows (x, y, w, h), gt_keep uint8 [G] with bit s = kept in
 * subset s (S <= DANHIP_WIDER_MAX_SUBSETS).  Detections for steps 1-5 as CSR too: det_offsets int32 [I+1], det_rows double [D,5] rows
 * (x, y, w, h, score), at most DANHIP_WIDER_MAX_DETS rows per image; scores and boxes are finite, w, h >= 0.
 *   danhip_wider_quantize    : the text route + compaction.  dets [B,Nmax,5] (in_dtype DANHIP_F32, or DANHIP_WIDER_F64 with quantize = 0),
 *                              num int32 [B] (clamped to [0, Nmax]), image_index int32 [B].  quantize != 0: rows are fp32 (xmin, ymin, xmax,
 *                              ymax, score); bw = xmax - xmin + 1, bh = ymax - ymin + 1 in fp32; a row stays iff ceil(bh) >= 10 and bw > 1
 *                              and score > 0.01f; it becomes (floor xmin, floor ymin, ceil bw, ceil bh, rint(double(score) * 1000) / 1000) -
 *                              the doubles that parsing write_to_txt's text gives.  quantize == 0: rows are (x, y, w, h, score), all kept.
 *                              Image image_index[b]'s rows go, in order, to store_rows double [I,cap,5] at [image_index[b]], their number to
 *                              store_counts int32 [I] (the caller fills it with -1 = "not added" first).  Nmax <= cap <= DANHIP_WIDER_MAX_DETS.
 *   danhip_wider_score_range : step 1's lo, hi -> range double [2] (D == 0: 0, 0).  Two launches, no atomics.
 *   danhip_wider_eval        : steps 1-4 for all S subsets in one launch (a persistent grid; one workgroup per image at a time; rank sort,
 *                              boxes through LDS tiles, an LDS atomicMin per box, a block prefix sum, a binary search per threshold); the
 *                              curve goes to the workspace as per-workgroup uint32 partial sums.  max_dets = the caller's bound on an image's
 *                              detections: above DANHIP_WIDER_MAX_DETS -> DANHIP_EINVAL.  I <= 2^20, T <= DANHIP_WIDER_MAX_THRESHOLDS.
 *   danhip_wider_ap          : the same workspace -> curves int64 [S,T,2], count_face int64 [S] (every box of gt_keep counts, whether or not
 *                              its image had detections), precision / recall double [S,T], ap double [S] (step 5).  Two launches.
 * status int32 [1] (zeroed by the caller, OR-ed by the kernels, read by the caller after the evaluation): DANHIP_WIDER_EINDEX an
 * image_index outside [0, I) (that image is skipped), _ETWICE an image stored twice, _ECOUNT more detections in an image than the bound
 * (skipped), _EOFFSETS offsets that leave [0, D] / [0, G] or decrease (skipped).  Nothing is ever written or read out of bounds.
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_WIDER_MAX_DETS 2048
#define DANHIP_WIDER_MAX_SUBSETS 8
#define DANHIP_WIDER_MAX_THRESHOLDS 2046
#define DANHIP_WIDER_F64 4
#define DANHIP_WIDER_EINDEX 1
#define DANHIP_WIDER_ETWICE 2
#define DANHIP_WIDER_ECOUNT 4
#define DANHIP_WIDER_EOFFSETS 8
int danhip_wider_quantize(const void* dets, int in_dtype, const int32_t* num, const int32_t* image_index, int32_t B, int32_t Nmax,
                          int32_t quantize, double* store_rows, int32_t* store_counts, int32_t I, int32_t cap, int32_t* status, void* stream);
size_t danhip_wider_score_range_workspace_bytes(void);
int danhip_wider_score_range(const double* det_rows, int64_t D, double* range, void* workspace, size_t workspace_bytes, void* stream);
size_t danhip_wider_eval_workspace_bytes(int32_t I, int32_t S, int32_t T);
int danhip_wider_eval(const int32_t* det_offsets, const double* det_rows, int64_t D, const int32_t* gt_offsets, const double* gt_boxes,
                      const uint8_t* gt_keep, int64_t G, const double* range, int32_t I, int32_t S, int32_t T, int32_t max_dets,
                      double iou_threshold, void* workspace, size_t workspace_bytes, int32_t* status, void* stream);
int danhip_wider_ap(const void* workspace, size_t workspace_bytes, const uint8_t* gt_keep, int64_t G, int32_t I, int32_t S, int32_t T,
                    int64_t* curves, int64_t* count_face, double* precision, double* recall, double* ap, void* stream);

/* --------------------------------------------------------------------------------------------------
 * On-device training input pipeline: the image half of preprocess_for_train
 * (preprocessing/dan_preprocessing.py:677-733) in one pass from the decoded uint8 image [H,W,3] (RGB) to the network input
 * [out_h,out_w,8] (16-bit, B-mean, G-mean, R-mean, 0 x5):  [0,1] conversion -> distort_color (:98-150) -> crop window with
 * mean-colour fill (:410-565; the window may leave the image) -> legacy bilinear resize -> flip -> uint8 saturate -> means -> BGR.
 * op_codes: 0 brightness (value = delta), 1 saturation (factor), 2 hue (delta), 3 contrast (factor; at most one), applied in
 * the given order; the random draws themselves are the caller's (dan_amd/preprocessing/dan_preprocessing.py).
 * ------------------------------------------------------------------------------------------------ */
size_t danhip_augment_workspace_bytes(void);
int danhip_augment_preprocess(const uint8_t* src, int32_t H, int32_t W, int32_t nops, const int32_t* op_codes, const float* op_values,
                              int32_t win_y, int32_t win_x, int32_t win_h, int32_t win_w, int32_t flip, uint16_t* dst, int32_t out_h,
                              int32_t out_w, void* workspace, size_t workspace_bytes, void* stream);

/* The batched form (ABI version 11): B decoded images of DIFFERENT sizes -> one network input [B, out_h, out_w, 8] (same 16-bit layout), every
 * image with exactly the arithmetic of danhip_augment_preprocess (the kernels share its device functions).  As with danhip_pack_entry_init /
 * danhip_pack_conv_weights_batched, the caller fills a host array of fixed-size items with danhip_augment_item_init, copies it to the device
 * with one copy and passes the device table here; the call itself touches no host memory, so it is stream-ordered and can be captured.
 *   danhip_augment_item_init validates what it is given (DANHIP_EINVAL: null pointer, H / W <= 0, more than 4 ops, more than one contrast op,
 *   an unknown op code, a non-positive window size, flip outside 0..2) and returns in *mean_blocks how many workgroups of the contrast-mean
 *   launch the item owns (0 without a contrast op); first_mean_block is the running sum of those counts over the items before it and
 *   total_mean_blocks of the call the sum over all items.  The window may leave the image.
 *   flip: 0 none; 1 the resized image is flipped (dan / pb_preprocessing.py:707-714); 2 the window is flipped BEFORE the resize
 *   (sfd_preprocessing.py:522-531, where the flip precedes tf.image.resize_images).  danhip_augment_preprocess keeps its 0 / non-zero meaning.
 * KERNEL LAUNCHES PER CALL, whatever B is: 1 when total_mean_blocks == 0 (no item has a contrast op), otherwise 3 - the workspace zero-fill,
 * one segmented fp64 reduction for the contrast means of all items that have the op (a workgroup's pixels belong to one image; the other items
 * take no part), and the image pass (one workgroup = a 32 x 8 tile of one output image, grid z = image; the mean's final division is folded in).
 * Items without a contrast op equal danhip_augment_preprocess bit for bit; with one, up to the fp64 summation order of the mean.
 * workspace: danhip_augment_batch_workspace_bytes(B) bytes, 16-byte aligned, zeroed inside the call when it is used.  DANHIP_EINVAL for a null
 * table / dst, B <= 0 (or > 65535), a non-positive output size; the CONTENTS of the table are on the device and are not validated by the call. */
typedef struct {
  const uint8_t* src;                      /* uint8 [H, W, 3] RGB, any byte alignment (views into a decoder's buffer) */
  int32_t H, W;
  int32_t nops, contrast_at;               /* contrast_at: index of the contrast op in the chain, -1 = none */
  int32_t op[4];
  float val[4];
  int32_t win_y, win_x, win_h, win_w;
  int32_t flip;
  int32_t first_mean_block, mean_blocks, pad_;
} danhip_augment_item;
size_t danhip_augment_item_bytes(void);    /* sizeof(danhip_augment_item), for callers that bind the library without this header */
int danhip_augment_item_init(danhip_augment_item* item, const uint8_t* src, int32_t H, int32_t W, int32_t nops, const int32_t* op_codes,
                             const float* op_values, int32_t win_y, int32_t win_x, int32_t win_h, int32_t win_w, int32_t flip,
                             int32_t first_mean_block, int32_t* mean_blocks);
size_t danhip_augment_batch_workspace_bytes(int32_t B);
int danhip_augment_preprocess_batch(const danhip_augment_item* table_dev, int32_t B, int32_t total_mean_blocks, uint16_t* dst, int32_t out_h,
                                    int32_t out_w, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------------------
 * Test-time pipeline for images of DIFFERENT sizes (ABI version 12; dan_amd/eval_dan.py:detect_image_list; csrc/evalpipe_ragged_exact.hip).
 *
 * danhip_resize_u8_linear_batch: every resized and / or mirrored copy of every image in ONE launch.  All sources lie in one source buffer
 * and all results in one destination buffer; an item names a source view uint8 [H, W, 3] (src + src_offset, any byte alignment, rows `pitch`
 * bytes apart) and its result uint8 [Ho, Wo, 3] (dst + dst_offset, dense).  The arithmetic is danhip_resize_u8_linear's, pixel for pixel
 * (the kernels share one device function); mirror = 1 reads source column W-1-x, i.e. the item is the resize of image.flip(1); fx = fy = 1
 * with mirror = 1 is the plain mirrored copy.  As with danhip_augment_item_init, the caller fills a host array of items with
 * danhip_resize_item_init (first_tile = the running sum of the *tiles it returned for the items before), uploads it with one copy and passes
 * BOTH tables: the host table is validated before anything is launched, the kernel reads the device table.  A workgroup's pixels belong to
 * one item; the grid is the flat list of all items' tiles, so items of very different sizes leave no workgroup idle.
 * DANHIP_EINVAL with a message, before any launch - from danhip_resize_item_init: a non-positive size, Ho / Wo that are not rint(H * fy) /
 * rint(W * fx) in double, pitch < 3 * W, fx / fy not positive and finite, mirror outside 0 / 1, a negative offset or first_tile; from the
 * batch call in addition: an item init did not fill, a tile prefix that does not add up, a source range that leaves [0, src_bytes), a
 * destination range that leaves [0, dst_bytes) or overlaps another item's.
 *
 * danhip_detect_select: the tail of one detection pass - detect_face's order and cut (eval_dan.py:107-116), the size filter of
 * multi_scale_test / multi_scale_test_pyramid and flip_test's mirror map - written straight into the voting buffer.
 *   boxes fp32 [A,4] rows (ymin, xmin, ymax, xmax), scores fp32 [A]; K <= min(A, 2048) (the pipeline's K = min(A - 1, int(max_per_image * 1.5)));
 *   rows double [K,5] = (xmin, ymin, xmax, ymax, score), valid uint8 [K].
 *   Row r is element r of the descending arg-sort of the scores with equal scores taken HIGHER index first (danhip_argsort_desc_f32 with
 *   ties_high_index_first: numpy's argsort()[::-1]; -0 = +0).  Coordinates are box / shrink in fp32, correctly rounded (a true division:
 *   __fdiv_rn; the build passes no flag that relaxes fp32 division and compiles the file with -ffp-contract=off), then widened to double.
 *   mirror_width >= 0 (the width w of the image flip_test mirrored): xmin' = (w - xmax) - 1, xmax' = (w - xmin) - 1 in fp32; < 0: none.
 *   filter 0: valid = 1; 1 "big": max(w, h) > 30; 2 "small": min(w, h) < 100, with w = (xmax - xmin) + 1, h = (ymax - ymin) + 1 in fp32 on
 *   the row BEFORE the mirror map.
 *   Precondition: the scores are finite.  With NaNs nothing is read or written out of bounds, but which rows come out is not promised.
 *   No sort of the A scores: a radix select (11 + 11 + 10 bits of the order-preserving key) finds the K-th key, the keys above it and the
 *   highest-index ties of it are collected, and those K are ordered in LDS.  KERNEL LAUNCHES PER CALL: DANHIP_DETECT_SELECT_LAUNCHES = 7,
 *   whatever A is (zero-fill, three histograms, tie count, collect, emit); *launches (may be NULL) receives the number the call issued.
 *   workspace: danhip_detect_select_workspace_bytes(A) bytes, 16-byte aligned.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int64_t src_offset, dst_offset;          /* bytes from the call's src / dst */
  int32_t H, W, pitch;                     /* source rows are `pitch` bytes apart (>= 3 * W) */
  int32_t Ho, Wo;
  int32_t mirror;
  int32_t first_tile, tiles;               /* the item's workgroups: [first_tile, first_tile + tiles) of the grid */
  double fx, fy;
  double scale_x, scale_y;                 /* 1 / fx, 1 / fy, what the kernel computes with */
} danhip_resize_item;
size_t danhip_resize_item_bytes(void);     /* sizeof(danhip_resize_item), for callers that bind the library without this header */
int danhip_resize_item_init(danhip_resize_item* item, int64_t src_offset, int32_t H, int32_t W, int32_t pitch, int64_t dst_offset, int32_t Ho,
                            int32_t Wo, double fx, double fy, int32_t mirror, int32_t first_tile, int32_t* tiles);
int danhip_resize_u8_linear_batch(const danhip_resize_item* table_host, const danhip_resize_item* table_dev, int32_t n, const uint8_t* src,
                                  int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, void* stream);
#define DANHIP_DETECT_SELECT_LAUNCHES 7
size_t danhip_detect_select_workspace_bytes(int64_t A);
int danhip_detect_select(const float* boxes, const float* scores, int32_t A, int32_t K, float shrink, int32_t filter, float mirror_width,
                         double* rows, uint8_t* valid, void* workspace, size_t workspace_bytes, int32_t* launches, void* stream);

/* --------------------------------------------------------------------------------------------------
 * Baseline JPEG decode in front of the input pipeline (ABI version 6): a record's 'image/encoded' bytes -> the uint8 [H,W,3] RGB device
 * image danhip_augment_preprocess reads, equal bit for bit to what Pillow (libjpeg-turbo, JDCT_ISLOW, fancy upsampling) decodes.
 * The serial half - marker parsing, Huffman decoding - runs on host threads (csrc/jpeg_entropy.cpp, no HIP call: these entry points work in
 * a process without a GPU); dequantisation, the islow IDCT, fancy chroma upsampling and YCbCr -> RGB are two launches per BATCH
 * (csrc/jpeg_exact.hip: jpeg_idct_kernel, jpeg_upsample_rgb_kernel), each a grid over (image, tile) through the descriptor table.
 * Accepted: SOF0 / SOF1, 8 bit, Huffman, ONE interleaved scan; 1 component (grey), or 3 components Y Cb Cr with luma sampling 1x1 (4:4:4),
 * 2x1 (4:2:2) or 2x2 (4:2:0) and chroma 1x1; up to 4 quantisation tables of 8 or 16 bit; any DHT set; DRI / RSTn; FF00 stuffing; JFIF
 * APP0 / EXIF / COM segments skipped; 1x1 up to DANHIP_JPEG_MAX_DIM per side (checked before anything is sized from the header).
 * Everything else is refused ON THE HOST with one of the reason codes below (the caller then decodes that image some other way); so is a
 * block whose dequantised coefficients have a sum of squares above DANHIP_JPEG_MAX_BLOCK_ENERGY: up to there no 16-bit intermediate of
 * libjpeg-turbo's vector IDCT wraps or saturates and no 32-bit one of the kernel overflows (an 8-bit image's own blocks stay below 1024^2
 * plus their quantisation error), beyond it the two need not agree.
 * Coefficients: int16, per image at coef_offset (a multiple of 64 elements), the component planes one after the other, a plane's 8x8
 * blocks in raster order of the component's block grid (padded to whole MCUs), a block's 64 values de-zigzagged and COLUMN-major
 * (element col*8 + row), so that a lane's one 16-byte load is a column of the first IDCT pass.
 * No index the device uses is taken from the file: the kernels see descriptors that danhip_jpeg_entropy_decode_batch computed, and
 * danhip_jpeg_reconstruct_batch re-derives every field from (width, height, mode) and checks it against the buffer sizes before a launch.
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_JPEG_MAX_DIM 16384
#define DANHIP_JPEG_MAX_BLOCK_ENERGY 2073600      /* 1440^2 */
#define DANHIP_JPEG_MAX_THREADS 16
#define DANHIP_JPEG_GREY 0
#define DANHIP_JPEG_444 1
#define DANHIP_JPEG_422 2
#define DANHIP_JPEG_420 3
/* reason codes (info.reason, status_out[i], desc.status); 0 = decoded / decodable on the device */
#define DANHIP_JPEG_ENOTJPEG 1       /* no SOI, or no marker where one must be */
#define DANHIP_JPEG_ETRUNCATED 2     /* the stream ends (or meets a marker) before the header / the scan is complete */
#define DANHIP_JPEG_EPROGRESSIVE 3   /* SOF2 */
#define DANHIP_JPEG_EARITHMETIC 4    /* SOF9..SOF15 */
#define DANHIP_JPEG_EPRECISION 5     /* sample precision other than 8 (12 bit) */
#define DANHIP_JPEG_EMULTISCAN 6     /* a scan that does not carry every component */
#define DANHIP_JPEG_ECOMPONENTS 7    /* 4 components (CMYK / YCCK), or any count but 1 and 3 */
#define DANHIP_JPEG_EADOBE 8         /* Adobe APP14 with transform != 1 */
#define DANHIP_JPEG_ERGBIDS 9        /* component ids 'R' 'G' 'B' */
#define DANHIP_JPEG_ESAMPLING 10     /* sampling factors other than 4:4:4 / 4:2:2 / 4:2:0 (4:1:1, 4:4:0, ...) */
#define DANHIP_JPEG_EHUFFMAN 11      /* a code no table holds, a run past coefficient 63, a DC value outside int16 */
#define DANHIP_JPEG_ETOOLARGE 12     /* a side above DANHIP_JPEG_MAX_DIM */
#define DANHIP_JPEG_ETABLE 13        /* a malformed or missing DQT / DHT, a malformed SOF / SOS / DRI */
#define DANHIP_JPEG_EUNSUPPORTED 14  /* lossless / hierarchical frames, DNL, a second frame */
#define DANHIP_JPEG_ERESTART 15      /* the expected RSTn is not where the restart interval puts it */
#define DANHIP_JPEG_ECOEFRANGE 16    /* a block above DANHIP_JPEG_MAX_BLOCK_ENERGY */
#define DANHIP_JPEG_ECAPACITY 17     /* coef_out has no room for this image */
typedef struct danhip_jpeg_info {
  int32_t width, height, ncomp, mode; /* mode: DANHIP_JPEG_GREY .. DANHIP_JPEG_420 */
  int32_t reason, reserved;
  int64_t coef_count;                 /* int16 elements danhip_jpeg_entropy_decode_batch writes for this image (0 when refused) */
} danhip_jpeg_info;
typedef struct danhip_jpeg_desc {
  int32_t width, height, ncomp, mode;
  int32_t blocks_w[3], blocks_h[3];   /* block grid of each component (whole MCUs); a plane's pitch is blocks_w * 8 bytes */
  int32_t comp_w[3], comp_h[3];       /* the component's own size ceil(width * h / hmax) x ceil(height * v / vmax): the upsampling edges */
  int32_t quant_index[3];
  int32_t status;                     /* reason code; != 0: every count and offset below is 0, the image takes no device work */
  int32_t idct_groups, rgb_groups;    /* workgroups of launch 1 (32 blocks each) and launch 2 (256 lanes x 8 pixels each) */
  int32_t reserved[2];
  int64_t coef_offset, coef_count;    /* int16 elements */
  int64_t plane_offset[3];            /* bytes into the workspace, multiples of 256 */
  int64_t out_offset;                 /* bytes into out, a multiple of 256; the image is width * height * 3 bytes there */
  uint16_t quant[4][64];              /* row-major (de-zigzagged) */
} danhip_jpeg_desc;
/* header only: dims, mode, coefficient count, reason (also returned).  info may not be NULL. */
int danhip_jpeg_inspect(const uint8_t* data, int64_t n, danhip_jpeg_info* info);
/* B streams on min(threads, B, DANHIP_JPEG_MAX_THREADS) host threads (threads < 1: 1).  Image i's coefficients go to
 * coef_out[descs_out[i].coef_offset ...]: offsets are handed out in order to the images whose header is accepted; an image that is refused
 * later (a truncated scan, a bad code) keeps its slot and nothing outside that slot is written.  status_out[i] = reason code, 0 = decoded.
 * The device offsets (planes, output, workgroup counts) are handed out afterwards to the decoded images alone.  Returns DANHIP_EINVAL for bad
 * arguments, else DANHIP_OK whatever the per-image statuses are. */
int danhip_jpeg_entropy_decode_batch(const uint8_t* const* datas, const int64_t* sizes, int32_t B, int32_t threads, int16_t* coef_out,
                                     int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out);
size_t danhip_jpeg_workspace_bytes(const danhip_jpeg_desc* descs, int32_t B);     /* host descriptors; 0 when none is decodable or one is malformed */
int64_t danhip_jpeg_output_bytes(const danhip_jpeg_desc* descs, int32_t B);       /* likewise */
/* The two launches.  descs_host / descs_dev: the same B descriptors in host and in device memory (the host copy is validated and sizes the
 * grids, the kernels read the device copy); coef_dev: int16 [coef_count], 16-byte aligned; out: uint8 [out_bytes].  launches (may be NULL)
 * receives the number of kernels launched: 2, or 0 when no descriptor is decodable.  B <= 65535. */
int danhip_jpeg_reconstruct_batch(const int16_t* coef_dev, int64_t coef_count, const danhip_jpeg_desc* descs_host,
                                  const danhip_jpeg_desc* descs_dev, int32_t B, uint8_t* out, int64_t out_bytes, void* workspace,
                                  size_t workspace_bytes, int32_t* launches, void* stream);

/* --------------------------------------------------------------------------------------------------
 * Huffman decoding on the device (ABI version 7): the entropy stage of the decoder above as a self-synchronising parallel Huffman decoder
 * (Klein & Wiseman; Weissenberger & Schmidt 2018), opt-in.  The host keeps what is O(header): danhip_jpeg_scan_prepare_batch parses the
 * same headers, makes ONE pass over the scan that looks for FF only (the end of the scan, every RSTn when DRI is set), and packs into one
 * staging buffer: per-image geometry, one SEGMENT per restart interval, one work item per SUBSEQUENCE (DANHIP_JPEG_SUBSEQ_BYTES stuffed
 * bytes of a segment), the workgroups (at most DANHIP_JPEG_SUBSEQ_PER_GROUP items whose bytes fit one LDS window), the chunks of the DC
 * prefix sum, the Huffman tables the scans use and the scan bytes, left stuffed.  The upload is that buffer: about the streams themselves.
 * csrc/jpeg_huffman_exact.hip then writes the SAME int16 coefficient buffer danhip_jpeg_entropy_decode_batch writes, bit for bit, in
 * 5 + DANHIP_JPEG_SYNC_ROUNDS launches whatever the data and the batch size are:
 *   zero the buffer | speculate: every lane decodes its subsequence from state (block 0 of the MCU, coefficient 0) and the group iterates
 *   "decode from the predecessor's exit" to its fixed point | DANHIP_JPEG_SYNC_ROUNDS times the same step, a group's first lane seeded with
 *   the previous group's last exit of the launch before | write: prefix sum of completed blocks, one more decode from the final entry that
 *   stores the coefficients and VERIFIES that it reproduces the stored exit | two launches of DC prefix sum, int16 range and block energy.
 * A chain of exits that reproduces itself from a segment's true start is the serial decode; an image where it does not (more group seams in
 * one restart interval than rounds can carry), or whose scan the device finds malformed, gets a non-zero word in status_dev and the caller
 * hands it to danhip_jpeg_entropy_decode_batch, which stays the authority for reason codes.  The descriptors are the ones the host stage
 * fills, so danhip_jpeg_reconstruct_batch runs unchanged behind either.
 * No index the device uses leaves a range that the host derived from the header: stream reads are bounded by the segment and the staged
 * window (zero bits beyond), coefficient writes by the segment's block count and the image's slot, loops by constants; no workgroup waits
 * for another inside a launch; danhip_jpeg_huffman_decode_batch re-derives and checks every table of the staging buffer before a launch.
 * danhip_jpeg_entropy_emulate_batch runs the same phases through the same routines (csrc/jpeg_huffman.h) on the host with checked indexing.
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_JPEG_SUBSEQ_BYTES 128
#define DANHIP_JPEG_SUBSEQ_PER_GROUP 256
#define DANHIP_JPEG_SYNC_ROUNDS 2
#define DANHIP_JPEG_DEV_NOTSYNC 1     /* status bits of the device stage: the exits did not reach their fixed point */
#define DANHIP_JPEG_DEV_ERROR 2       /* a bad code, run or category; bits beyond a segment; a DC value or a block energy out of range */
#define DANHIP_JPEG_HOSTONLY (-1)     /* prepare status: a decodable header whose scan (1 GiB or more) is left to the host stage */
/* upper bound of the staging bytes danhip_jpeg_scan_prepare_batch needs for these streams (headers only; 0: bad arguments) */
size_t danhip_jpeg_scan_staging_bytes(const uint8_t* const* datas, const int64_t* sizes, int32_t B);
/* status_out[i]: 0 = prepared for the device; a reason code = refused, with the code the host stage gives (a header it refuses, an RSTn
 * that is missing or out of sequence); DANHIP_JPEG_HOSTONLY.  descs_out as danhip_jpeg_entropy_decode_batch fills them: coefficient slots in
 * order to every accepted header, device offsets to the prepared images.  staging: 16-byte aligned. */
int danhip_jpeg_scan_prepare_batch(const uint8_t* const* datas, const int64_t* sizes, int32_t B, void* staging, size_t staging_bytes,
                                   int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out);
size_t danhip_jpeg_scan_device_bytes(const void* staging);       /* the prefix of a prepared staging buffer that the device needs */
size_t danhip_jpeg_scan_workspace_bytes(const void* staging);    /* device workspace of danhip_jpeg_huffman_decode_batch */
/* The launches.  staging_host / staging_dev: the same prepared bytes in host and device memory (the host copy is validated, the kernels
 * read the device copy); coef_dev: int16 [coef_count], 16-byte aligned, written whole; status_dev: int32 [B] in device memory, 0 = decoded.
 * launches (may be NULL) receives the number of kernels launched: 5 + DANHIP_JPEG_SYNC_ROUNDS, or 0 when no image is prepared. */
int danhip_jpeg_huffman_decode_batch(const void* staging_host, const void* staging_dev, size_t staging_bytes, int32_t B, int16_t* coef_dev,
                                     int64_t coef_count, const danhip_jpeg_desc* descs_host, const danhip_jpeg_desc* descs_dev,
                                     void* workspace, size_t workspace_bytes, int32_t* status_dev, int32_t* launches, void* stream);
/* The same phases on the host.  sync_rounds < 0: DANHIP_JPEG_SYNC_ROUNDS (another value is for tests of the verify step).  coef_out: the
 * slots of the prepared images are written, nothing else.  range_errors (may be NULL) receives the number of indices the checked accessors
 * refused: 0 unless the decoder is wrong. */
int danhip_jpeg_entropy_emulate_batch(const void* staging, size_t staging_bytes, int32_t B, const danhip_jpeg_desc* descs, int16_t* coef_out,
                                      int64_t coef_count, int32_t sync_rounds, int32_t* status_out, int64_t* range_errors);

/* --------------------------------------------------------------------------------------------------
 * Progressive streams (ABI version 8), opt-in: with DANHIP_JPEG_ALLOW_PROGRESSIVE in `flags` the host entropy stage also takes SOF2 frames
 * (8 bit, Huffman, the component counts and sampling factors of the baseline path) and leaves the SAME coefficient array and descriptors
 * behind, so that danhip_jpeg_reconstruct_batch - which re-derives everything from (width, height, mode) - runs unchanged: a progressive
 * file that is complete gives libjpeg the same kind of coefficient array as a baseline file, and the same dequantisation, islow IDCT, fancy
 * upsampling and colour conversion follow.  Without the flag (and through the entry points above, which pass flags = 0) SOF2 stays
 * DANHIP_JPEG_EPROGRESSIVE.
 * Accepted: any number of scans, DHT between scans (tables are latched per scan), DRI between scans, every scan obeying T.81 G.1.1.1.1 as
 * libjpeg's start_pass_phuff_decoder checks it - Ss = 0 implies Se = 0; an AC scan has ONE component and 1 <= Ss <= Se <= 63; Al <= 13;
 * Ah = 0 on the first scan of a coefficient, afterwards Ah = that coefficient's previous Al and Al = Ah - 1; a component's DC before any of
 * its AC bands; no coefficient twice at the same precision - and, at EOI, COMPLETE: every coefficient 0..63 of every component sent down to
 * Al = 0.  Anything else is DANHIP_JPEG_EPROGRESSION (libjpeg's "warn and go on" is not reproduced).  The completion rule exists because
 * libjpeg decodes an incomplete progression through another path - inter-block smoothing of the coefficients not yet refined, coarse
 * coefficients left as they are - for which the device kernels have no counterpart: such a file differs from its complete version by tens
 * of grey levels and stays with the caller's fallback.  A DQT after the first SOS is DANHIP_JPEG_ETABLE (libjpeg latches a component's
 * quantisation table at its first scan); a stream that ends before EOI or meets a marker inside a scan's data is DANHIP_JPEG_ETRUNCATED.
 * The DC range and block energy checks of the baseline path are applied to the finished coefficients, with the same reason codes.
 * The device Huffman stage does not take progressive scans: danhip_jpeg_scan_prepare_batch_ex hands an accepted progressive header its
 * coefficient slot, no device segments and the status DANHIP_JPEG_HOSTONLY (the caller sends it through the host stage), or the reason
 * code the host stage gives.
 * An accepted progressive frame is marked by info.reserved = 1 and desc.reserved[0] = 1 (0 otherwise); the launcher does not read them.
 * Unknown bits in flags: DANHIP_EINVAL.  flags = 0: exactly the entry point without _ex.
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_JPEG_ALLOW_PROGRESSIVE 1
#define DANHIP_JPEG_EPROGRESSION 18  /* a progressive frame whose scan script is not taken: a scan against T.81 G.1.1.1.1, or incomplete at EOI */
int danhip_jpeg_inspect_ex(const uint8_t* data, int64_t n, uint32_t flags, danhip_jpeg_info* info);
int danhip_jpeg_entropy_decode_batch_ex(const uint8_t* const* datas, const int64_t* sizes, int32_t B, int32_t threads, uint32_t flags,
                                        int16_t* coef_out, int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out);
int danhip_jpeg_scan_prepare_batch_ex(const uint8_t* const* datas, const int64_t* sizes, int32_t B, uint32_t flags, void* staging,
                                      size_t staging_bytes, int64_t coef_capacity, danhip_jpeg_desc* descs_out, int32_t* status_out);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange (csrc/comm.cpp): the all-reduce(sum) of tf_replicate_model_fn.py:633-645
 * (_compute_sum_on_device: add_n over the towers' gradients, after _scale_loss :615-631 put 1/N into every tower's loss) issued
 * straight on RCCL (rccl.h: ncclCommInitRank / ncclAllReduce / ncclReduceScatter / ncclAllGather) from this library, on the caller's
 * stream — no framework process group, no watchdog / heartbeat thread, so the calls can be recorded into a hipGraph like any kernel
 * (RCCL's collectives are stream-ordered device work; SURVEY 8b: "directly via rccl.h from C++ for the overlapped bucket path").
 * librccl is NOT a link-time dependency: it is dlopen'ed at the first danhip_comm_* call (danhip_comm_load names the file, e.g. the
 * copy PyTorch ships; NULL = the copy already in the process, else librccl.so[.1] on the loader path).  One communicator = one rank =
 * one GPU (the device current at danhip_comm_create); the 128-byte unique id is produced by rank 0 and carried to the other ranks by
 * the caller (any host channel: a TCP store, a file, MPI).  A communicator must be used by one thread at a time (RCCL's rule).
 * dtype: DANHIP_F32 | DANHIP_BF16 | DANHIP_F16 (here DANHIP_BF16 means bf16 whatever the build's activation type is).
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_ECOMM (-4)      /* RCCL missing / an RCCL call failed (danhip_last_error carries ncclGetErrorString) */
#define DANHIP_COMM_ID_BYTES 128
int danhip_comm_load(const char* librccl_path);                        /* optional; idempotent once a copy is bound */
int danhip_comm_rccl_version(int* version);                            /* ncclGetVersion: e.g. 22606 */
int danhip_comm_unique_id(void* id128);                                /* host buffer of DANHIP_COMM_ID_BYTES (rank 0) */
/* collective over the nranks callers; device >= 0: hipSetDevice(device) first (RCCL binds a communicator to the calling thread's
 * current device), -1: the current device */
int danhip_comm_create(const void* id128, int32_t nranks, int32_t rank, int32_t device, void** comm_out);
int danhip_comm_destroy(void* comm);                                   /* after the streams that carry its collectives have drained */
int danhip_comm_info(void* comm, int32_t* nranks, int32_t* rank, int32_t* device);
/* Failure detection (ncclCommGetAsyncError / ncclCommAbort; ProcessGroupNCCL's watchdog did this from a background thread, here the
 * CALLER polls): *err = 0 while the communicator is healthy, else the RCCL error code of a collective that failed asynchronously (a
 * peer died, a link dropped) with its text in danhip_last_error().  danhip_comm_abort tears a communicator down WITHOUT waiting for
 * its outstanding collectives (the only way out when a peer is gone; danhip_comm_destroy would wait for ever). */
int danhip_comm_async_error(void* comm, int32_t* err);
int danhip_comm_abort(void* comm);
/* buf[i] = sum over ranks of buf[i], in place, asynchronous on stream */
int danhip_comm_allreduce_sum(void* comm, void* buf, int64_t count, int dtype, void* stream);
/* recv[0:recvcount] = sum over ranks of send[rank*recvcount : (rank+1)*recvcount]   (send holds nranks*recvcount elements; recv may be
 * the caller's own slice of send: in place) */
int danhip_comm_reduce_scatter_sum(void* comm, const void* send, void* recv, int64_t recvcount, int dtype, void* stream);
/* recv[r*sendcount : (r+1)*sendcount] = rank r's send   (send may be the caller's slice of recv: in place) */
int danhip_comm_allgather(void* comm, const void* send, void* recv, int64_t sendcount, int dtype, void* stream);

/* ---- split-operand inference (csrc/split_infer.hip): fp32-accurate evaluation at the 16-bit MFMA rate, for the same north-star bound as the
 * fp32 path below (eval_dan.py:299-404 box outputs within 1e-4).  An fp32 map [M, C] is carried as IEEE-half limbs in a 3C-channel NHWC
 * map X3 = [hi | lo | hi] (hi = half(x), lo = half(x - hi)), C3 = 3C rounded up to 8; with weights W3 = [hi | hi | lo] along Cin the
 * ordinary 16-bit convolution of the fp16 build (libdanhip_f16.so: danhip_conv2d_fwd with Cin = C3, fp32 output) computes
 * hi.hi + lo.hi + hi.lo with exact products and fp32 accumulation.  These entry points are identical in both builds (always IEEE half).
 * relu != 0: max(x, 0) first.  danhip_maxpool2x2_split3: tf.layers.max_pooling2d([2,2],[2,2],'same') on the 3C layout (C % 8 == 0).
 *
 * Exponents: a limb map may hold x * 2^e instead of x (e = its exponent; exp / in_exp / out_exp below are such powers of two, applied exactly):
 * the split path keeps every map and weight tensor inside half's range this way.  A limb writer that meets a value hi cannot hold (|x * 2^e|
 * >= 65520, or NaN) sets the int32 device flag registered with danhip_split_set_range_flag (NULL = no flag); the caller reads it after the
 * evaluation and fails - the limbs of such a value are inf / -inf, which the next convolution turns into NaN and a ReLU into 0. */
int danhip_split_set_range_flag(int32_t* flag);
int danhip_split3_f32(const float* x, uint16_t* y3, int64_t M, int32_t C, int32_t C3, int relu, int32_t exp, void* stream);
int danhip_unsplit3_f32(const uint16_t* x3, float* y, int64_t M, int32_t C, int32_t C3, void* stream);
int danhip_unsplit3_scaled_f32(const uint16_t* x3, float* y, int64_t M, int32_t C, int32_t C3, int32_t exp, void* stream);     /* y = (hi + lo) * 2^exp */
int danhip_maxpool2x2_split3(const uint16_t* x3, uint16_t* y3, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);     /* keeps the exponent */
/* l2_normalize (net/sfd_net.py:68-79) on the limb layout -> limb layout; the arithmetic of unsplit -> danhip_l2norm_fwd_f32 -> split in one pass */
int danhip_l2norm_split3(const uint16_t* x3, const float* gamma, uint16_t* y3, int64_t M, int32_t C, int32_t in_exp, int32_t out_exp, void* stream);
/* The first layer of the split-operand path (conv1_1: 3x3 / stride 1 / 'same', x fp32 [N,H,W,3], w HWIO fp32 [3,3,3,64]) as an exact fp32 FMA chain,
 * stored straight in the next convolution's limb layout y3 [N,H,W,192] with exponent out_exp; bias may be NULL. */
int danhip_conv3x3_c3_f32_split3(const float* x, const float* w_hwio, const float* bias, uint16_t* y3, int32_t N, int32_t H, int32_t W, int32_t Cout,
                                 int relu, int32_t out_exp, void* stream);
/* fp16 build: danhip_conv2d_fwd_ws over a limb map x3 (Cin = C3) with limb weights that carry a power-of-two exponent: v = acc * 2^acc_exp + bias
 * (acc_exp in [-126, 127]; the caller folds the output map's exponent into acc_exp and bias), relu?; out_dtype DANHIP_F32 stores v,
 * DANHIP_SPLIT3 v's limbs (Cout % 8 == 0).  The bf16 build refuses it. */
int danhip_conv2d_fwd_split(const danhip_conv_desc* d, const uint16_t* x3, const uint16_t* wf_packed, const float* bias, void* y, int out_dtype,
                            int relu, int32_t acc_exp, void* ws, size_t ws_bytes, void* stream);

/* ---- fp32 inference path (csrc/f32_infer.hip): the evaluation graphs of eval_sfd.py:232-283 / eval_pb.py / eval_dan.py:299-404 with fp32
 * storage and arithmetic end to end, for the north-star tolerance "eval box outputs within 1e-4 of the reference".  NHWC fp32
 * activations, the TF variables as they are (HWIO fp32 kernel, no packing; Cin need not be padded), forward only.  Same semantics as
 * the 16-bit entry points above: TF 'same' / 'valid' sizes through the descriptor, optional bias / ReLU / residual-after-activation. */
int danhip_conv2d_fwd_f32(const danhip_conv_desc* d, const float* x, const float* w_hwio, const float* bias, float* y, int relu,
                          const float* residual, void* stream);
int danhip_maxpool2x2_fwd_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
int danhip_l2norm_fwd_f32(const float* x, const float* gamma, float* y, int64_t M, int32_t C, void* stream);
int danhip_resize_bilinear_add_fwd_f32(const float* up, const float* lateral, float* out, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                       int32_t Wo, int32_t C, void* stream);
int danhip_avgpool2x2s1_same_fwd_f32(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);
/* deformable im2col of DeformConvOp (cpp/Deform/deform_conv.cu:229-275) in fp32: S[N,Ho,Wo,kh*kw*C]; the GEMM is a 1x1
 * danhip_conv2d_fwd_f32 over S */
int danhip_deform_sample_fwd_f32(const float* x, const float* offsets, float* S, int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh,
                                 int32_t kw, int32_t stride, int32_t dilation, int32_t deformable_group, void* stream);

/* --------------------------------------------------------------------------------------------------
 * CRC-32C (Castagnoli; ABI version 14): the checksum of TF-V2 checkpoint tensors, index blocks and TFRecord frames
 * (csrc/crc32c.cpp on the host, csrc/crc32c_exact.hip on the device; the arithmetic both share is csrc/crc32c.h).
 * Polynomial 0x82F63B78 (reflected), init and final xor 0xFFFFFFFF.
 *
 * danhip_crc32c_host: the CRC of data[0, n) continued from `crc` (0 to start; (data, 0, crc) returns crc, so (.., 0, 0) is 0) - the
 *   semantics of utility/checkpoint.py:crc32c.  Slicing-by-8 tables; on x86-64 with SSE4.2 (asked at run time) the crc32 instruction, same
 *   bits.  danhip_crc32c_host_form(.., form): 0 the same, 1 always the tables (tests compare the two).  No GPU call, no error state.
 * danhip_crc32c_combine: the CRC of A || B from crc(A), crc(B) and len(B): crc_a * x^(8 len_b) mod P, xor crc_b, the power by
 *   square-and-multiply over all 64 bits of len_b.  The device path combines its pieces with this arithmetic.
 *
 * danhip_crc32c_batch: the CRCs of n DEVICE byte ranges of any length and byte alignment -> crc_out_dev uint32 [n] (masked != 0: TensorFlow's
 *   crc32c::Mask, ((c >> 15) | (c << 17)) + 0xa282ead8).  An empty range gives 0 (masked: the mask of 0); n == 0 succeeds and launches nothing.
 *   Table hand-over, as with danhip_resize_u8_linear_batch: the caller fills a host array of danhip_crc_segment and uploads it with ONE
 *   copy - to the FRONT of the workspace, ordered before the call on `stream`.  table_host is validated before anything is launched and sizes
 *   the grid; the kernels read the copy in the workspace; the call itself touches no other host memory, copies nothing and does not
 *   synchronise.  Nothing outside a range is read.
 *   KERNEL LAUNCHES PER CALL: DANHIP_CRC32C_BATCH_LAUNCHES = 3 whatever n and the sizes are (plan, walk, finish;
 *   danhip_crc32c_batch_last_launches() returns what the calling thread's last call issued).  Pieces are combined by integer XOR (an ordinary
 *   vector atomic on the range's word): the same bits in any order, deterministic mode is not concerned.
 *   A lane walks danhip_crc32c_chunk_bytes() bytes, a workgroup danhip_crc32c_group_bytes() (of 16-byte aligned lines, so a range that starts
 *   off alignment takes its windows from its pointer rounded down).
 *   workspace: danhip_crc32c_batch_workspace_bytes(n, total_bytes) bytes, 16-byte aligned (total_bytes = the sum of the ranges' sizes; the
 *   present form keeps one word per range, so the answer depends on n alone).
 *   DANHIP_EINVAL: n < 0 or > 2^22, a null table / output / workspace, a range with bytes > 0 and a null pointer, more than 2^31 windows;
 *   DANHIP_EWORKSPACE: a short workspace.  Option "crc_table" [DANHIP_CRC_TABLE]: the walk's form (csrc/crc32c_exact.hip).
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  const void* ptr;                           /* device pointer, any alignment; may be NULL when bytes == 0 */
  uint64_t bytes;
} danhip_crc_segment;
#define DANHIP_CRC32C_BATCH_LAUNCHES 3
uint32_t danhip_crc32c_host(const void* data, size_t n, uint32_t crc);
uint32_t danhip_crc32c_host_form(const void* data, size_t n, uint32_t crc, int32_t form);
uint32_t danhip_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
size_t danhip_crc_segment_bytes(void);       /* sizeof(danhip_crc_segment), for callers that bind the library without this header */
int32_t danhip_crc32c_chunk_bytes(void);
int32_t danhip_crc32c_group_bytes(void);
int32_t danhip_crc32c_batch_last_launches(void);
size_t danhip_crc32c_batch_workspace_bytes(int32_t n, uint64_t total_bytes);
int danhip_crc32c_batch(const danhip_crc_segment* table_host, int32_t n, uint32_t* crc_out_dev, int32_t masked, void* ws, size_t ws_bytes,
                        void* stream);

/* --------------------------------------------------------------------------------------------------
 * Baseline JPEG encode (ABI version 15): uint8 [H,W,3] RGB -> a JFIF file that is byte for byte what Pillow (libjpeg-turbo) writes with
 * Image.save(f, "JPEG", quality=q, subsampling=s) - the mirror of the decoder above, made for the debug images of the evaluation
 * command.  The pixel stage runs on the device (csrc/jpeg_encode_exact.hip), the Huffman stage and the file writer on host threads
 * (csrc/jpeg_encode.cpp, no HIP call); the integer arithmetic both share is csrc/jpeg_encode.h, which also says where libjpeg-turbo
 * parts from the textbook (edges and dummy blocks, the reciprocal quantiser, the quality scaling, APP0).
 *
 * Scope: quality 1 .. 100; mode DANHIP_JPEG_420 (Pillow's default, subsampling=2) or DANHIP_JPEG_444 (subsampling=0); sides 1 ..
 * DANHIP_JPEG_MAX_DIM; optimize=True through the calls of "JPEG encode: optimised Huffman tables" below; no progressive.  The file is SOI,
 * JFIF APP0, two DQT, SOF0, four DHT (the standard tables of T.81 K.3, or the image's own), SOS, the stuffed scan padded with 1 bits, EOI.
 * Grey input, 4:2:2, restart intervals and progressive files are not made.
 *
 * danhip_jpeg_encode_prepare: one descriptor per image from (width, height) and the call's (mode, quality): geometry by the rules of the
 *   decoder (whole MCUs), reciprocal quantisation tables, and offsets handed out in order into the coefficient buffer (int16 elements), the
 *   device workspace (bytes) and the file buffer (bytes; file_capacity is a bound no image can exceed).  srcs[i] is image i's first byte -
 *   a device pointer for danhip_jpeg_encode_pixels_batch, a host pointer for danhip_jpeg_encode_pixels_host; rows are width * 3 bytes
 *   apart (views into one buffer, the decoder's, or separate tensors).  srcs may be NULL for descriptors that only feed the entropy stage.
 *   totals_out[3] = {coefficients, workspace bytes, file bytes}.
 * danhip_jpeg_encode_pixels_batch: the device pixel stage, DANHIP_JPEG_ENCODE_LAUNCHES launches whatever B and the sizes are, each a
 *   (workgroup, image) grid through the descriptor table (the host copy is re-derived from (width, height, mode) and checked against the
 *   buffer sizes before a launch; the kernels read the device copy).
 *     1 colour and downsample: RGB -> YCbCr, planar component planes in the workspace (pitch = block-grid width * 8), edges replicated;
 *       4:2:0 chroma by (a + b + c + d + bias) >> 2, bias 1, 2 alternating along the row.
 *     2 forward DCT and quantisation: eight lanes own a block - level shift, the jfdctint row pass, the transpose through LDS, the column
 *       pass, the reciprocal quantiser.
 *   Coefficients leave as int16 IN THE LAYOUT danhip_jpeg_entropy_decode_batch PRODUCES (component planes, raster blocks over whole MCUs,
 *   de-zigzagged, column-major), so either stage can be tested against the decoder's.
 * danhip_jpeg_encode_pixels_host: the same stage on the host through the same arithmetic (checked indexing, one thread).
 * danhip_jpeg_encode_entropy_batch: coefficients in host memory -> files.  min(threads, B, DANHIP_JPEG_MAX_THREADS) threads; image i's
 *   file is files_out[descs[i].file_offset ...], sizes_out[i] bytes long.
 * danhip_jpeg_encode_host: the whole encoder on the host for one image; *size_out = the file's size.  DANHIP_EWORKSPACE when capacity is
 *   below it (danhip_jpeg_encode_file_bound gives a capacity that always suffices).
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_JPEG_ENCODE_LAUNCHES 2
typedef struct danhip_jpeg_enc_desc {
  const uint8_t* src;                 /* RGB, rows width * 3 bytes apart */
  int32_t width, height, mode, quality;
  int32_t blocks_w[3], blocks_h[3];   /* block grid of each component over whole MCUs: the coefficient layout; a plane's pitch is blocks_w * 8 */
  int32_t comp_w[3], comp_h[3];       /* the component's own size */
  int32_t real_bw, real_bh;           /* luma blocks that carry samples: ceil(width / 8) x ceil(height / 8); the rest are dummy blocks */
  int32_t color_groups, fdct_groups;  /* workgroups of launch 1 (256 lanes x 8 luma columns x 1 | 2 rows) and launch 2 (32 blocks each) */
  int64_t coef_offset, coef_count;    /* int16 elements */
  int64_t plane_offset[3];            /* bytes into the workspace, multiples of 256 */
  int64_t file_offset, file_capacity; /* bytes into the file buffer */
  uint16_t recip[2][64], corr[2][64]; /* luma | chroma quantiser, row-major (de-zigzagged): csrc/jpeg_encode.h dh_jenc_quant */
  uint8_t shift[2][64];
  uint8_t qtable[2][64];              /* the tables the file carries, row-major */
} danhip_jpeg_enc_desc;
size_t danhip_jpeg_enc_desc_bytes(void);                                         /* sizeof(danhip_jpeg_enc_desc) */
int64_t danhip_jpeg_encode_file_bound(int32_t width, int32_t height, int32_t mode);   /* 0: outside the scope */
int danhip_jpeg_encode_prepare(const int32_t* widths, const int32_t* heights, const void* const* srcs, int32_t B, int32_t mode, int32_t quality,
                               danhip_jpeg_enc_desc* descs_out, int64_t* totals_out);
int danhip_jpeg_encode_pixels_batch(const danhip_jpeg_enc_desc* descs_host, const danhip_jpeg_enc_desc* descs_dev, int32_t B, int16_t* coef_dev,
                                    int64_t coef_count, void* workspace, size_t workspace_bytes, int32_t* launches, void* stream);
int danhip_jpeg_encode_pixels_host(const danhip_jpeg_enc_desc* descs, int32_t B, int16_t* coef_out, int64_t coef_count);
int danhip_jpeg_encode_entropy_batch(const int16_t* coef, int64_t coef_count, const danhip_jpeg_enc_desc* descs, int32_t B, int32_t threads,
                                     uint8_t* files_out, int64_t files_capacity, int64_t* sizes_out);
int danhip_jpeg_encode_host(const uint8_t* rgb, int32_t width, int32_t height, int32_t mode, int32_t quality, uint8_t* out, int64_t capacity,
                            int64_t* size_out);

/* --------------------------------------------------------------------------------------------------
 * JPEG encode: Huffman stage on the device (ABI version 16), opt-in: the coefficient buffer danhip_jpeg_encode_pixels_batch leaves on the
 * device -> the complete files in ONE device buffer, image i's at descs[i].file_offset, plus int64 sizes[B] and int32 status[B] in device
 * memory.  Every byte of every file is what danhip_jpeg_encode_entropy_batch writes from the same coefficients and descriptors; the scope
 * is that stage's (4:2:0 and 4:4:4, quality 1 .. 100, the tables of T.81 K.3, one interleaved scan, no restart intervals).
 *
 * The host keeps what is O(B) and makes no HIP call: danhip_jpeg_encode_scan_prepare checks the descriptors and packs into one staging
 * buffer, per image, the scan geometry (MCU counts, blocks in scan order), the offsets into the device workspace (workgroup bit sums and
 * bit offsets, the unstuffed bit buffer, the FF counts and offsets), the four code / length tables, and the markers in front of the scan
 * (SOI, APP0, DQT, SOF0, DHT, SOS - a function of (width, height, mode, quality), written by the writer the host stage uses).  An image
 * whose file bound reaches 1 GiB gets the status DANHIP_JPEG_HOSTONLY and is left to the host stage.
 *
 * csrc/jpeg_encode_huffman_exact.hip then runs DANHIP_JPEG_ENCODE_ENTROPY_LAUNCHES launches whatever B, the sizes and the data are; each
 * is a (workgroup, image) grid or one workgroup per image, and no workgroup waits for another inside a launch:
 *   1 length   one lane per block in scan order (MCU-interleaved): the DC difference against the component's previous block, the 63 AC
 *              values in zig-zag order, ZRL for runs of 16 and more, EOB -> the block's bits; a workgroup's sum; the workgroup also zeroes
 *              its share of the unstuffed buffer
 *   2 offsets  one workgroup per image: the prefix sum of the workgroup sums as 64-bit bit offsets, the scan's total, status[i]
 *   3 write    the same walk emits the codes MSB first at the block's bit offset (workgroup prefix sum + the workgroup's offset), whole
 *              32-bit words OR-ed into the zeroed buffer (atomicOr: the bytes do not depend on timing); the last block pads with 1 bits
 *   4 count    the FF bytes of every DANHIP_JPEG_ENCODE_STUFF_LANE_BYTES * 256 bytes of the unstuffed scan
 *   5 finish   one workgroup per image: prefix sum of the counts, the markers copied in front, FF D9 behind, sizes[i]
 *   6 stuff    every byte to file_offset + marker length + its index + the FF bytes in front of it, 00 behind every FF
 * Every index comes from the staging buffer, which danhip_jpeg_encode_huffman_batch re-derives from the host descriptors and compares
 * before a launch.  Coefficient values change counts only: a block counts at most 1658 bits, word indices are checked against the unstuffed
 * buffer and byte indices against the slot's file_capacity (danhip_jpeg_encode_file_bound covers 1658 bits per block, every byte stuffed).
 * A value no baseline code carries (a DC difference of more than 11 bits, an AC value of more than 10) sets DANHIP_JPEG_ENC_DEV_RANGE in
 * status[i], a file that would leave its slot DANHIP_JPEG_ENC_DEV_CAPACITY; sizes[i] is then 0, nothing is written outside image i's slot,
 * and the caller hands the image to danhip_jpeg_encode_entropy_batch, which has the last word (it refuses such a value).
 * danhip_jpeg_encode_entropy_emulate_batch runs the same phases through the same routines (csrc/jpeg_encode_huffman.h) on the host with
 * checked indexing.
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_JPEG_ENCODE_ENTROPY_LAUNCHES 6
#define DANHIP_JPEG_ENCODE_STUFF_LANE_BYTES 16
#define DANHIP_JPEG_ENC_DEV_RANGE 1     /* status bits of the device stage: a coefficient without a baseline code */
#define DANHIP_JPEG_ENC_DEV_CAPACITY 2  /* the file would leave its slot */
size_t danhip_jpeg_encode_scan_staging_bytes(int32_t B);                            /* 0: B outside 1 .. 65535 */
/* descs as danhip_jpeg_encode_prepare fills them (src is not read); coef_count / file_bytes: the sizes of the coefficient and file buffers
 * the launches will be given.  staging: 16-byte aligned, at least danhip_jpeg_encode_scan_staging_bytes(B) bytes.  status_out[i]: 0 =
 * prepared, or DANHIP_JPEG_HOSTONLY.  DANHIP_EINVAL for a descriptor that does not follow from its (width, height, mode, quality) or
 * leaves a buffer. */
int danhip_jpeg_encode_scan_prepare(const danhip_jpeg_enc_desc* descs, int32_t B, int64_t coef_count, int64_t file_bytes, void* staging,
                                    size_t staging_bytes, int32_t* status_out);
size_t danhip_jpeg_encode_scan_workspace_bytes(const void* staging);                /* device workspace of the launches; 0: not a staging buffer */
/* The launches.  staging_host / staging_dev: the same prepared bytes in host and device memory (the host copy is validated against
 * descs_host, the kernels read the device copy); coef_dev: int16 [coef_count]; files_dev: file_bytes bytes; sizes_dev: int64 [B];
 * status_dev: int32 [B], 0 = written, DANHIP_JPEG_HOSTONLY as prepared, else DANHIP_JPEG_ENC_DEV_* bits; workspace: 16-byte aligned.
 * launches (may be NULL) receives the number of kernels launched: DANHIP_JPEG_ENCODE_ENTROPY_LAUNCHES, or 0 when no image is prepared (the
 * caller then knows every status from the prepare call; nothing is written). */
int danhip_jpeg_encode_huffman_batch(const void* staging_host, const void* staging_dev, size_t staging_bytes,
                                     const danhip_jpeg_enc_desc* descs_host, int32_t B, const int16_t* coef_dev, int64_t coef_count,
                                     uint8_t* files_dev, int64_t file_bytes, int64_t* sizes_dev, int32_t* status_dev, void* workspace,
                                     size_t workspace_bytes, int32_t* launches, void* stream);
/* The same phases on the host, everything in host memory.  range_errors (may be NULL) receives the number of indices the checked accessors
 * refused: 0 unless the encoder is wrong (an out-of-range coefficient is a status, not a refused index). */
int danhip_jpeg_encode_entropy_emulate_batch(const void* staging, size_t staging_bytes, const danhip_jpeg_enc_desc* descs, int32_t B,
                                             const int16_t* coef, int64_t coef_count, uint8_t* files_out, int64_t file_bytes,
                                             int64_t* sizes_out, int32_t* status_out, int64_t* range_errors);

/* --------------------------------------------------------------------------------------------------
 * JPEG encode: optimised Huffman tables (ABI version 20), opt-in: the bytes of Pillow's save(..., optimize=True) - the same coefficients,
 * coded with tables made from the image's own symbol statistics by libjpeg's jpeg_gen_optimal_table rule (csrc/jpeg_encode.h
 * dh_jenc_optimal_table says where that is not the textbook Huffman code).  The layout of the file is unchanged; the four DHT segments
 * (DC 0, AC 0, DC 1, AC 1 in front of SOS) carry the image's tables.  Every call above keeps its prototype, its launches and its bytes.
 *
 * danhip_jpeg_optimal_table_host: the table rule alone.  counts[257]: occurrences of symbol 0 .. 255 (entry 256 is not read: the rule gives
 *   the reserved pseudo-symbol the count 1); bits_out[l] = codes of length l, bits_out[0] = 0; vals_out: the symbols in DHT order, 0 behind
 *   the last.  DANHIP_EINVAL when the counts sum to 2^31 - 1 or more or give a code of more than 32 bits before the cut to 16 bits.
 * danhip_jpeg_encode_entropy_batch_ex: danhip_jpeg_encode_entropy_batch with flags; DANHIP_JPEG_ENC_OPTIMIZE makes each thread count its
 *   image's symbols (every block the scan writes, dummy blocks included), build the four tables and write the scan with them.
 * danhip_jpeg_encode_scan_prepare_ex: danhip_jpeg_encode_scan_prepare with flags.  With DANHIP_JPEG_ENC_OPTIMIZE the staging buffer asks
 *   danhip_jpeg_encode_huffman_batch for DANHIP_JPEG_ENCODE_OPTIMIZE_LAUNCHES launches in front of its own, whatever B, the sizes and the
 *   data are (*launches is then the sum), and the workspace grows by danhip_jpeg_encode_optimize_layout's stride per image:
 *     1 clear      one workgroup per image zeroes the image's region
 *     2 histogram  (work item, image): a workgroup counts the symbols of up to out[6] blocks in scan order - a lane per block and round, the
 *                  DC predictor taken as the length launch takes it - into one 4 x 257 uint32 table per wave in LDS (integer LDS atomics),
 *                  then adds the non-zero sums into the image's table (integer global atomics: the result does not depend on the order)
 *     3 tables     one workgroup per image, one wave per table, its first lane runs dh_jenc_optimal_table over LDS; then all lanes write
 *                  bits / vals, the code | length << 16 table the length and write launches read, and the image's markers: the staged
 *                  ones with the four DHT segments replaced
 *   The six launches then read tables, markers and marker length through the image's region.  A symbol that does not occur has no code.
 *   The device's own bounds hold as before: a block of more than 1658 bits - possible only with own tables, at most 1665 - is flagged like
 *   a value without a code (DANHIP_JPEG_ENC_DEV_RANGE) and the image goes to the host stage; the markers are at most as long as the standard
 *   ones when every value has a baseline code (12 DC and 162 AC symbols at most), and their region holds out[7] bytes, four full segments.
 *   danhip_jpeg_encode_entropy_emulate_batch refuses such a staging buffer.
 * danhip_jpeg_encode_optimize_layout: out[8] = {region stride, offsets in a region of: the counts (uint32 [4][257]), the code | length table
 *   (uint32 [4][256]), bits / vals (uint8 [4][17 + 256]), the words (int32 [4], the first the markers' length), the markers; blocks per
 *   work item of the histogram launch; the markers' capacity}.  Image i's region starts at byte i * stride of the workspace.
 * danhip_jpeg_optimal_tables_device: the tables launch alone over n regions in device memory (16-byte aligned, n * stride bytes) whose
 *   counts the caller filled: writes the code | length table and bits / vals of each (the markers are left alone).  For tests of the rule.
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_JPEG_ENCODE_OPTIMIZE_LAUNCHES 3
#define DANHIP_JPEG_ENC_OPTIMIZE 1      /* flags of the _ex calls */
int danhip_jpeg_optimal_table_host(const int32_t counts[257], uint8_t bits_out[17], uint8_t vals_out[256]);
int danhip_jpeg_encode_entropy_batch_ex(const int16_t* coef, int64_t coef_count, const danhip_jpeg_enc_desc* descs, int32_t B, int32_t threads,
                                        int32_t flags, uint8_t* files_out, int64_t files_capacity, int64_t* sizes_out);
int danhip_jpeg_encode_scan_prepare_ex(const danhip_jpeg_enc_desc* descs, int32_t B, int64_t coef_count, int64_t file_bytes, int32_t flags,
                                       void* staging, size_t staging_bytes, int32_t* status_out);
int danhip_jpeg_encode_optimize_layout(int32_t out[8]);                              /* returns the stride; out may be NULL */
int danhip_jpeg_optimal_tables_device(void* regions_dev, int32_t n, void* stream);

/* --------------------------------------------------------------------------------------------------
 * Box drawing on uint8 [H,W,3] device images (ABI version 15; csrc/draw_exact.hip): the rectangles of utility/draw_toolbox.py
 * bboxes_draw_on_img for every image of a list in ONE launch.  The rule is this project's own (no OpenCV to compare with):
 *   box i of an image is skipped when classes[i] < 1 or a coordinate is not finite; corners x1, y1, x2, y2 = the floats bbox[0..3]
 *   truncated toward zero (Python's int(); clamped to +-2^30); skipped when x2 < x1 or y2 < y1;
 *   with t = thickness, a pixel (x, y) of the image is painted (203, 71, 119) when x1 - t/2 <= x <= x2 + t/2 and y1 - t/2 <= y <= y2 + t/2
 *   and it is not in the interior x1 + (t+1)/2 <= x <= x2 - (t+1)/2, y1 + (t+1)/2 <= y <= y2 - (t+1)/2 (integer divisions).  For t = 2 the
 *   band is the two pixels x1 - 1, x1 on the left, x2, x2 + 1 on the right, likewise above and below.
 * One colour, so the result does not depend on the order of the boxes; one lane per pixel tests the image's boxes, staged in LDS in
 * chunks; no atomics.  danhip_draw_boxes_u8 draws these rectangles and nothing else.
 *
 * The score label (ABI version 18; danhip_draw_boxes_labels_u8, csrc/draw_font.h): the reference's '%.1f%%' % (score * 100) in white on a
 * filled tab above each box, by this project's own rule (OpenCV's Hershey font and getTextSize are not matched):
 *   text: v = score * 100 in ONE float32 multiply; tenths = v * 10 rounded to the nearest integer, ties to even, on the exact value
 *   (computed in double, where the product is exact; v * 10 in float32 would round twice).  The string is the decimal digits of
 *   tenths / 10, '.', the digit tenths % 10, '%': what printf("%.1f%%", v) prints.  The label is drawn only when 0 <= tenths <= 9999
 *   (4 to 6 characters; NaN, the infinities, a negative tenths and 1000.0 and above draw the rectangle only); -0.0 and the negatives that
 *   round to it print as 0.0%, without printf's sign.  A skipped box has no label;
 *   font: 5 x 7 bitmap glyphs, advance 6: n characters have text_w = 6 n - 1; text_h = 7, baseline = 2;
 *   tab: (203, 71, 119) for x1 - t/2 <= x <= x1 + text_w and y1 - text_h - t - baseline <= y <= y1 (the reference's arithmetic,
 *   draw_toolbox.py:60-65, with these metrics);
 *   text: (255, 255, 255); the bottom glyph row is y = y1 - text_h + baseline, the top one 6 above it; the left column of character k
 *   is x = x1 + 6 k.  Everything is clipped to the image: a label that leaves the top or the right edge is cut, not moved;
 *   order: the reference's loop.  Box i paints its band, then its tab, then its text, and box i + 1 paints over all of it: a pixel shows
 *   what the highest-index box that touches it paints there, and within that box the text beats the tab beats the band.
 * One lane per pixel walks ALL staged boxes in index order (no early-out) and stores once; the score is formatted once per box.
 * scores float [n] beside boxes and classes, required when n_boxes > 0; everything else is validated as danhip_draw_boxes_u8 does.
 * danhip_draw_glyph: the 7 row bytes of glyph `index` (0 - 9 the digits, 10 '.', 11 '%'), top row first, bit 4 the left column.
 * danhip_draw_format_score (host): the string of a score by the rule above, or "" when no label is drawn - the same inline function the
 * kernel runs.
 * items: one per image, in host memory (validated, sizes the grid) and in device memory (read by the kernel); boxes float [n,4] and
 * classes int32 [n] of all images back to back, an item names its range.  thickness 1 .. 64.
 * ------------------------------------------------------------------------------------------------ */
typedef struct danhip_draw_item {
  uint8_t* image;                     /* device, uint8 [height, width, 3], rows width * 3 bytes apart */
  int32_t width, height;
  int32_t first_box, num_boxes;       /* rows of boxes / classes */
  int32_t groups, reserved;           /* workgroups of 256 pixels: ceil(width * height / 256) */
} danhip_draw_item;
size_t danhip_draw_item_bytes(void);
int danhip_draw_boxes_u8(const danhip_draw_item* items_host, const danhip_draw_item* items_dev, int32_t n_images, const float* boxes_dev,
                         const int32_t* classes_dev, int64_t n_boxes, int32_t thickness, void* stream);
int danhip_draw_boxes_labels_u8(const danhip_draw_item* items_host, const danhip_draw_item* items_dev, int32_t n_images,
                                const float* boxes_dev, const int32_t* classes_dev, const float* scores_dev, int64_t n_boxes,
                                int32_t thickness, void* stream);
int danhip_draw_glyph(int32_t index, uint8_t rows_out[7]);       /* 0-9 digits, 10 '.', 11 '%' */
int danhip_draw_format_score(float score, char out[8]);          /* host: the string, or "" when no label is drawn */

/* --------------------------------------------------------------------------------------------------
 * Transposed convolution 4x4 / stride 2 with the LFPN's lateral add (ABI version 19; csrc/conv_transpose.hip):
 * tf.layers.conv2d_transpose(x, Cout, (4, 4), strides=(2, 2), padding='same') on NHWC, written out:
 *
 *   full[n, oy, ox, co] = b[co] + sum over ky, kx in 0..3 and ci of x[n, iy, ix, ci] * W[ky, kx, co, ci]
 *                         with oy = 2 iy + ky - 1, ox = 2 ix + kx - 1, 0 <= iy < Hi, 0 <= ix < Wi
 *   out [n, oy, ox, co] = lateral[n, oy, ox, co] + full[n, oy, ox, co]        for oy < Ho, ox < Wo
 *
 *   - full is 2 Hi x 2 Wi; Ho is 2 Hi or 2 Hi - 1 and Wo is 2 Wi or 2 Wi - 1: the odd sizes are a top-left crop (a 'same' pool halved an
 *     odd map).  Any other Ho / Wo is DANHIP_EINVAL, not a silent result;
 *   - lateral and bias may be NULL;
 *   - products are accumulated in fp32; ONE rounding to the activation type, at the end, after bias and lateral;
 *   - every output has 1, 2 or 4 contributing taps per input channel (corner, edge, interior);
 *   - the variable is W [4, 4, Cout, Cin] fp32 (TensorFlow's conv2d_transpose layout) and b [Cout] fp32.
 * Cin and Cout: multiples of 64 up to 1024, anything else is DANHIP_EINVAL.  No call here uses float atomics: each result is a fixed
 * function of the call's inputs, in deterministic mode and out of it.
 *
 * danhip_conv_transpose4x4s2_pack_weight: W -> wf (16-bit, [4,4,Cout,Cin], the forward's operand) and, unless NULL, wb (16-bit,
 *   [4,4,Cin,Cout], the data gradient's operand); 16 Cin Cout elements each.
 * danhip_conv_transpose4x4s2_add_fwd: x [N,Hi,Wi,Cin], lateral / out [N,Ho,Wo,Cout], 16-bit activations; on the MFMA, by output parity.
 * danhip_conv_transpose4x4s2_dgrad: dx [N,Hi,Wi,Cin] (+)= the gradient of x for dout [N,Ho,Wo,Cout] (a cropped row / column of full carries
 *   no gradient); accumulate != 0: dx = dx + gradient in fp32, one rounding (the second delivery into a gradient slot).
 * danhip_conv_transpose4x4s2_wgrad: dw [4,4,Cout,Cin] += sum over pixels of dout x; db [Cout] += sum over pixels of dout (fp32; either
 *   may be NULL).  Partial sums over pixel slabs are stored in the workspace (danhip_conv_transpose4x4s2_wgrad_workspace_bytes bytes for the
 *   same shape, 16-byte aligned; a smaller one is DANHIP_EWORKSPACE) and added in slab order by the ordered reduction.
 *   danhip_conv_transpose4x4s2_wgrad_slabs: how many partial sums of dw that is (0 for an unsupported shape, like the byte count).
 * danhip_conv_transpose4x4s2_add_fwd_f32: the same rule on fp32 tensors with the fp32 variable as it is (fp32 inference path; FMA chains).
 * ------------------------------------------------------------------------------------------------ */
int danhip_conv_transpose4x4s2_pack_weight(const float* w, void* wf, void* wb, int32_t Cin, int32_t Cout, void* stream);
int danhip_conv_transpose4x4s2_add_fwd(const void* x, const void* wf, const float* bias, const void* lateral, void* out, int32_t N, int32_t Hi,
                                       int32_t Wi, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout, void* stream);
int danhip_conv_transpose4x4s2_dgrad(const void* dout, const void* wb, void* dx, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                     int32_t Cin, int32_t Cout, int accumulate, void* stream);
size_t danhip_conv_transpose4x4s2_wgrad_workspace_bytes(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout);
int32_t danhip_conv_transpose4x4s2_wgrad_slabs(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout);
int danhip_conv_transpose4x4s2_wgrad(const void* x, const void* dout, float* dw, float* db, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                     int32_t Wo, int32_t Cin, int32_t Cout, void* workspace, size_t workspace_bytes, void* stream);
int danhip_conv_transpose4x4s2_add_fwd_f32(const float* x, const float* w, const float* bias, const float* lateral, float* out, int32_t N,
                                           int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout, void* stream);

/* --------------------------------------------------------------------------------------------------
 * Fused batch-norm tails (ABI version 21; csrc/bn_act.hip): what closes a conv -> BN -> ReLU layer and a ResNet bottleneck unit
 * (net/resnet_danet.py:157-218), over the channel axis of [M,C] 16-bit activations (M = N*H*W), C % 8 == 0, C <= 2048, any M:
 *
 *   y = act(xhat * gamma + beta + shortcut),  xhat = (x - mean) * rstd,  act = ReLU when relu != 0, else the identity
 *
 *   - shortcut ([M,C], 16-bit) may be NULL; the sum is kept in fp32 and rounded to 16 bits ONCE, at the store;
 *   - every activation and per-channel array is 16-byte aligned (DANHIP_EINVAL otherwise).
 * danhip_bn_act_fwd_train: batch statistics and the moving-average update are those of danhip_batchnorm_fwd_train (the same two kernels,
 *   the same launches, workspace = 2*C doubles, 8-byte aligned; moving_mean / moving_var may be NULL), then ONE apply launch.
 * danhip_bn_act_fwd_infer: the apply launch alone with the caller's mean and rstd = rsqrt(var + eps).
 * danhip_bn_act_bwd: y != NULL says the forward had relu != 0; the mask [y > 0] is applied on the fly in both passes (no masked copy of dy):
 *     g = dy * [y > 0];   dbeta = sum g,  dgamma = sum g * xhat   (OVERWRITTEN; fp32 atomics; one clear when dbeta == dgamma + C)
 *     dx = gamma * rstd * (g - dbeta / M - xhat * dgamma / M)     or, frozen != 0 (mean / rstd are constants):  dx = g * gamma * rstd
 *     dshortcut = g                                                (unless NULL; written in the same pass as dx)
 *   Two launches: reduce, apply.
 * With the option "deterministic" set the three calls return DANHIP_EINVAL, as danhip_batchnorm_* do (their float atomics have no ordered form).
 * ------------------------------------------------------------------------------------------------ */
int danhip_bn_act_fwd_train(const uint16_t* x, const uint16_t* shortcut, const float* gamma, const float* beta, uint16_t* y, float* save_mean,
                            float* save_rstd, float* moving_mean, float* moving_var, int64_t M, int32_t C, float eps, float momentum,
                            int relu, float* workspace, void* stream);
int danhip_bn_act_fwd_infer(const uint16_t* x, const uint16_t* shortcut, const float* gamma, const float* beta, const float* mean,
                            const float* rstd, uint16_t* y, int64_t M, int32_t C, int relu, void* stream);
int danhip_bn_act_bwd(const uint16_t* x, const uint16_t* dy, const uint16_t* y, const float* gamma, const float* mean, const float* rstd,
                      uint16_t* dx, uint16_t* dshortcut, float* dgamma, float* dbeta, int64_t M, int32_t C, int frozen, void* stream);

/* --------------------------------------------------------------------------------------------------
 * Face chips (ABI version 22; csrc/face_chips_exact.hip; dan_amd/utility/face_chips.py): every detection of every image of a list cropped
 * and resized to uint8 [S, S, 3] in TWO launches, whatever the number of images and detections; nothing is read back.
 * The rectangle rule is this project's own, integers only (restated by dan_amd/utility/face_chips.py rule).  For row r of image i
 * (H x W), dets[i, r] = (x1, y1, x2, y2, score) fp32, the layout eval_dan.detect_image_list returns:
 *   corners = the floats truncated toward zero (Python's int(); clamped to +-2^30, as danhip_draw_boxes_u8 does); w = x2 - x1 + 1,
 *   h = y2 - y1 + 1;
 *   no chip when r >= num[i], score < score_threshold (an fp32 compare: a score equal to the threshold is kept), a coordinate is NaN or
 *   infinite, or w < 1 or h < 1;
 *   margin: x1 -= mx, x2 += mx with mx = w * margin_pm / 1000, y1 -= my, y2 += my with my = h * margin_pm / 1000 (integer divisions of
 *   non-negative numbers; margin_pm in per mille, 0 .. 4000);
 *   square != 0, after the margin: s = max(w', h') of the grown sides; x1 -= (s - w') / 2, x2 = x1 + s - 1, likewise y: the shorter
 *   side gets (s - side) / 2 in front and the rest behind;
 *   then the rectangle is intersected with [0, W-1] x [0, H-1] (danhip_face_chips_u8 and pad = 0 of danhip_face_chips_u8_ex; pad = 1 is
 *   below): xc1, yc1, xc2, yc2; an empty intersection gives no chip.
 *   Intermediates are 64-bit: |corner| <= 2^30 and margin_pm <= 4000 keep every product below 2^44.
 *   The chip is cv2.resize(image[yc1 : yc2 + 1, xc1 : xc2 + 1], (S, S), INTER_LINEAR): danhip_resize_u8_linear's arithmetic (the kernels
 *   share one device function) with the crop's top-left byte as the source, the image's pitch, the crop's size and scale = crop / S in double.
 * Valid slots are numbered in (image, row) ascending order by a prefix sum inside ONE workgroup that loops over the slots (no atomics,
 * nothing the order could depend on).  *count_out receives the TRUE number of valid slots; the first min(count, max_chips) of them are
 * written, the rest of chips_out / chip_src_out is not touched: count > max_chips tells the caller of the overflow.
 *   images_host / images_dev: one danhip_resize_item per image, in host memory (validated) and in device memory (read by the kernels);
 *     src_offset (from `src`, any byte alignment), H, W and pitch are read, the other fields are not (danhip_resize_item_init with
 *     fx = fy = 1 fills an item);
 *   dets fp32 [n_images, rows_per_image, 5], num int32 [n_images]; n_images * rows_per_image <= 2^24;
 *   chips_out uint8 [max_chips, S, S, 3]; chip_src_out int32 [max_chips, 6] = (image, row, xc1, yc1, xc2, yc2); count_out int32 [1];
 *   1 <= S <= 1024; workspace: danhip_face_chips_workspace bytes (0 today: the query and the arguments are there so that another
 *   numbering scheme needs no new entry point; NULL is accepted when the query answers 0).
 * DANHIP_EINVAL with a message and no launch: S or margin_pm out of range, square outside 0 / 1, a NaN threshold, max_chips < 0, a
 * negative or too large n_images / rows_per_image, a workspace below the query, a NULL pointer, an image whose size is not positive,
 * whose pitch is below 3 * W or whose bytes leave [0, src_bytes).  n_images == 0 or rows_per_image == 0: *count_out = 0, success.
 * ------------------------------------------------------------------------------------------------ */
int danhip_face_chips_workspace(int32_t n_images, int32_t rows_per_image, size_t* bytes);
int danhip_face_chips_u8(const danhip_resize_item* images_host, const danhip_resize_item* images_dev, int32_t n_images, const uint8_t* src,
                         int64_t src_bytes, const float* dets, const int32_t* num, int32_t rows_per_image, int32_t S, int32_t margin_pm,
                         int32_t square, float score_threshold, uint8_t* chips_out, int32_t* chip_src_out, int32_t* count_out,
                         int32_t max_chips, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------------------
 * Face chips, extended (ABI version 23; csrc/face_chips_exact.hip): zero-padded rectangles and an antialiased (area) downscale.
 * danhip_face_chips_u8_ex takes danhip_face_chips_u8's 19 arguments in order, then filter, pad and fill_rgb; danhip_face_chips_u8 itself
 * keeps its kernels and its bytes.  Still TWO launches per call (a select launch of the same single looping workgroup, one resize launch),
 * nothing read back, no atomics.  Everything up to and including squaring is the rule above, unchanged.
 *   pad = 1: the rectangle is NOT intersected with the image: chip_src carries the unclipped (x1, y1, x2, y2), which may be negative or
 *     beyond W-1 / H-1; a rectangle whose intersection with the image is empty still gives no chip; a position of the rectangle outside
 *     the image reads the constant fill_rgb[c] (3 bytes in HOST memory, read before the call returns; NULL = zeros).  pad = 0: the clipping
 *     above.
 *   Side cap: no chip when a side of the rectangle (the unclipped one when pad = 1, the clipped one otherwise) exceeds
 *     DANHIP_FACE_CHIPS_MAX_SIDE = 32768.  It keeps every sum below 2^38 (255 * 2^30) and bounds the work per chip.  (Only here:
 *     danhip_face_chips_u8 has no cap.)
 *   filter = DANHIP_FACE_CHIPS_LINEAR (0): the chip is cv2.resize(crop, (S, S), INTER_LINEAR) bit for bit, crop = the rectangle, padded
 *     when pad = 1: the arithmetic above with a pixel fetch that answers fill outside the image (replication at the border is that of
 *     the RECTANGLE, as cv2.resize of the padded crop does it).  filter = 0, pad = 0 gives danhip_face_chips_u8's bytes.
 *   filter = DANHIP_FACE_CHIPS_AREA (1): this project's own rule, integers only, separable, ONE rounding.  For an axis with n source
 *     positions (the rectangle's side) and S outputs, output j has integer weights over the source positions i and a divisor D:
 *       n > S (the axis shrinks), box filter, D = n: source position i covers [i*S, (i+1)*S), output j covers [j*n, (j+1)*n);
 *         weight(i) = max(0, min((j+1)*n, (i+1)*S) - max(j*n, i*S)), nonzero for i = floor(j*n / S) .. floor(((j+1)*n - 1) / S);
 *         the weights sum to n;
 *       n <= S, exact half-pixel linear, D = 2*S: t = (2*j + 1)*n - S, i0 = floor(t / (2*S)) (toward minus infinity), f = t - 2*S*i0;
 *         weight 2*S - f on clamp(i0, 0, n-1) and f on clamp(i0 + 1, 0, n-1) (the clamp is to the rectangle, not the image); n == S is
 *         the identity.
 *     A chip byte is (sum_y sum_x wy * wx * p(y, x) + (Dx*Dy) / 2) / (Dx*Dy), both divisions integer divisions of non-negative 64-bit
 *     numbers (round half up); p is the image byte, or fill_rgb[c] outside the image.  The two axes choose their form independently
 *     (with pad = 0 a clipped rectangle can shrink on one axis and grow on the other).  No floating point.
 *     The kernel is separable within a workgroup: one (chip, output row, 256 output columns) item per workgroup at a time; bands of
 *     source rows are read with consecutive lanes on consecutive bytes, reduced to exact horizontal sums (uint32, at most 255 * 32768
 *     < 2^23) in LDS, and finished vertically in 64 bits.
 * danhip_face_chips_ex_workspace: 0 bytes today (the band lives in LDS); it validates n_images, rows_per_image, S and filter.
 * DANHIP_EINVAL with a message and no launch: filter outside 0 / 1, pad outside 0 / 1, and everything danhip_face_chips_u8 refuses.
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_FACE_CHIPS_MAX_SIDE 32768
#define DANHIP_FACE_CHIPS_LINEAR 0
#define DANHIP_FACE_CHIPS_AREA 1
int danhip_face_chips_ex_workspace(int32_t n_images, int32_t rows_per_image, int32_t S, int32_t filter, size_t* bytes);
int danhip_face_chips_u8_ex(const danhip_resize_item* images_host, const danhip_resize_item* images_dev, int32_t n_images, const uint8_t* src,
                            int64_t src_bytes, const float* dets, const int32_t* num, int32_t rows_per_image, int32_t S, int32_t margin_pm,
                            int32_t square, float score_threshold, uint8_t* chips_out, int32_t* chip_src_out, int32_t* count_out,
                            int32_t max_chips, void* workspace, size_t workspace_bytes, void* stream, int32_t filter, int32_t pad,
                            const uint8_t fill_rgb[3]);

/* --------------------------------------------------------------------------------------------------
 * Face redaction (ABI version 24; csrc/redact_exact.hip, csrc/redact_walk.h; dan_amd/utility/redact.py): every detection of every image
 * of a list blurred, pixelated or filled, out of place, in DANHIP_REDACT_LAUNCHES launches whatever the number of images, detections and
 * sizes; nothing is read back.  The rule is this project's own, integers only after the corners are truncated, ONE rounding (restated by
 * dan_amd/utility/redact.py rule_pixel / reference).  For image i (H x W, uint8 RGB), row r is dets[i, r] = (x1, y1, x2, y2, score):
 *   Rectangle: the face-chip rectangle above with square = 0, pad = 0 and the side cap: corners = int() of the floats clamped to +-2^30,
 *     w, h >= 1, margin_pm per mille on each side, intersected with the image: (x1, y1, x2, y2), clipped sides wc = x2 - x1 + 1,
 *     hc = y2 - y1 + 1.  No rectangle when r >= num[i], score < score_threshold (fp32 compare: equal is kept), a coordinate is NaN or
 *     infinite, w < 1 or h < 1, the intersection is empty, or a clipped side exceeds DANHIP_FACE_CHIPS_MAX_SIDE.
 *   Extent: e = clamp(max(wc, hc) * strength_pm / 1000, 1, DANHIP_REDACT_MAX_EXTENT) (integer division; strength_pm 1 .. 1000).
 *     DANHIP_REDACT_MAX_EXTENT = 255: a window sum is at most 255 * 511 * 511 < 2^32.
 *   Shape: DANHIP_REDACT_RECT (0): every pixel of the rectangle.  DANHIP_REDACT_ELLIPSE (1): pixel (px, py) of it when
 *     (2*(px-x1)+1-wc)^2 * hc^2 + (2*(py-y1)+1-hc)^2 * wc^2 <= wc^2 * hc^2, in 64 bits (the side cap keeps it below 2^62).
 *   Ownership: a pixel inside the shapes of several valid rows of its image belongs to the one with the HIGHEST row index; a pixel inside
 *     no shape is copied unchanged.
 *   Value: every mode reads the ORIGINAL image only, so the result depends on no execution order.
 *     DANHIP_REDACT_FILL (2): channel c = fill_rgb[c] (3 bytes in HOST memory, read before the call returns).
 *     DANHIP_REDACT_MOSAIC (1): cell side c = max(2, e); cells anchored at (x1, y1), each clipped to the rectangle; every channel is
 *       (S + A / 2) / A, S = the sum of the original bytes of the clipped cell, A = its pixel count, integer divisions.  With the ellipse the
 *       mean is still that of the whole clipped cell; only the pixels inside the ellipse are written.
 *     DANHIP_REDACT_BLUR (0): one box filter of radius e; the window [px-e, px+e] x [py-e, py+e] is intersected with the IMAGE (not the
 *       rectangle: the surroundings bleed in); (S + A / 2) / A with A the number of window pixels inside the image.
 * The launches: redact_select (ONE looping workgroup: the table of valid rectangles with their extents and the running number of work items
 * before each, in (image, row) order; no atomics), redact_copy (every pixel of every image, source to destination) and ONE work launch of the
 * mode.  Work items of blur and fill are tiles of DANHIP_REDACT_BAND output rows x DANHIP_REDACT_STRIP columns of one rectangle; of mosaic,
 * one cell.  A blur item keeps one uint32 vertical running sum per byte column of its strip plus the halo in LDS (adding the entering and
 * subtracting the leaving source row per output row) and takes every pixel's horizontal window sum from a prefix scan of them: the work
 * per pixel does not depend on e.  An item of row r writes a pixel only if no later valid row of the image holds it (a short list of the
 * later rectangles that meet the item's tile, built per item in LDS; no atomics, no races: every destination byte has one writer per launch).
 *   images_host / images_dev, src, src_bytes, dets, num, rows_per_image: as for danhip_face_chips_u8.
 *   dst_items_host / dst_items_dev: one danhip_resize_item per image for the destination: src_offset is the byte offset from `dst` (any
 *     alignment), H, W, pitch; H and W equal the source's.  The other fields are not read.
 *   count_out int32 [1]: the number of valid rectangles.  workspace: danhip_redact_workspace bytes (the table).
 * DANHIP_EINVAL with a message and no launch: mode or shape out of range, strength_pm outside 1 .. 1000, margin_pm outside 0 .. 4000, a NaN
 * threshold, a NULL pointer, negative counts or n_images * rows_per_image > 2^24, an image whose size is not positive, whose pitch is below
 * 3 * W or whose bytes leave its buffer, a destination whose size differs from its source or that overlaps a source image or another
 * destination, a workspace below the query.  n_images == 0: success, nothing is done.  rows_per_image == 0: the images are copied,
 * *count_out = 0 (dets and num may be NULL).
 * The index arithmetic of the walk (csrc/redact_walk.h: plain functions the kernels call) is exported for the host, no GPU call is made:
 *   danhip_redact_extent -> e of clipped sides; danhip_redact_item_count -> items of a rectangle (blur / fill: tiles, row-major; mosaic: cells,
 *   row-major), band / strip are the tile's sides (the kernels pass DANHIP_REDACT_BAND / _STRIP);
 *   danhip_redact_tile: item -> out[8] = (tx1, ty1, tx2, ty2 of the tile, inclusive; sx1, sy1, sx2, sy2 = the source columns and rows a blur
 *   item of extent e reads: the tile grown by e, intersected with the image);
 *   danhip_redact_window: pixel -> out[5] = (lo_x, lo_y, hi_x, hi_y, A) of the blur window; danhip_redact_cell: cell -> out[5] = (cx1, cy1,
 *   cx2, cy2, A); danhip_redact_in_shape -> 1 / 0.  Each answers DANHIP_EINVAL (or -1 for the int64 count) for arguments outside the rule.
 * ------------------------------------------------------------------------------------------------ */
#define DANHIP_REDACT_LAUNCHES 3
#define DANHIP_REDACT_MAX_EXTENT 255
#define DANHIP_REDACT_BAND 64
#define DANHIP_REDACT_STRIP 256
#define DANHIP_REDACT_BLUR 0
#define DANHIP_REDACT_MOSAIC 1
#define DANHIP_REDACT_FILL 2
#define DANHIP_REDACT_RECT 0
#define DANHIP_REDACT_ELLIPSE 1
int danhip_redact_workspace(int32_t n_images, int32_t rows_per_image, size_t* bytes);
int danhip_redact_u8(const danhip_resize_item* images_host, const danhip_resize_item* images_dev, int32_t n_images, const uint8_t* src,
                     int64_t src_bytes, const float* dets, const int32_t* num, int32_t rows_per_image, int32_t mode, int32_t shape,
                     int32_t strength_pm, int32_t margin_pm, float score_threshold, const uint8_t fill_rgb[3],
                     const danhip_resize_item* dst_items_host, const danhip_resize_item* dst_items_dev, uint8_t* dst, int64_t dst_bytes,
                     int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream);
int danhip_redact_extent(int32_t wc, int32_t hc, int32_t strength_pm);
int64_t danhip_redact_item_count(int32_t mode, const int32_t rect[4], int32_t e, int32_t band, int32_t strip);
int danhip_redact_tile(int32_t H, int32_t W, const int32_t rect[4], int32_t e, int32_t band, int32_t strip, int64_t item, int32_t out[8]);
int danhip_redact_window(int32_t H, int32_t W, int32_t e, int32_t px, int32_t py, int32_t out[5]);
int danhip_redact_cell(const int32_t rect[4], int32_t c, int64_t cell, int32_t out[5]);
int danhip_redact_in_shape(int32_t shape, const int32_t rect[4], int32_t px, int32_t py);

#ifdef __cplusplus
}
#endif
#endif /* DANHIP_H_ */
