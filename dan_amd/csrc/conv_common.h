// Shared between the convolution kernels: their argument block, the epilogue helpers and the kernel selection (ConvInstance below).
#pragma once
#include "lds_dma.h"

struct ConvArgs {
  const bf16_t* x;
  const bf16_t* w;
  const float* bias;
  const bf16_t* mask;
  const unsigned char* mask_bits;   // data gradient: the ReLU mask as one bit per element, [M][Co/8] bytes (danhip_relu_bits), instead of `mask`
  const bf16_t* resid;
  void* y;
  unsigned char* bits_out;        // forward conv_relu on the 128-wide halo tiles: also writes the ReLU bit mask of y ([M][Co/8] bytes) ...
  unsigned char* pool_bits_out;   // ... and of the fused pooled output
  bf16_t* pool_y;   // optional: 2x2/stride-2 SAME max-pool of y (ReLU outputs), written by the kernels that can fuse it
  unsigned char* pool_arg_out;    // optional, with pool_y: 2-bit arg-max codes of the pooled map ([pooled pixel][Co/4] bytes, channel c in bits
                                  // 2(c%4).. of byte c/4; code = 2*dh + dw of the FIRST maximum in row-major window order) for danhip_maxpool2x2_bwd_arg
  int N, H, W, C;
  int Ho, Wo, Co;
  int kh, kw, stride, pad_t, pad_l;
  int M, Kpad, ktiles, taps, cpt;
  FastDiv div_wo, div_howo, div_c, div_kw;
  int relu, out_f32, accumulate;
  int dshift;    // log2(dstride)
  float* splitk_ws;      // split-K (conv_igemm.hip, maps too small to fill the chip): fp32 partial outputs [splits][M][Co]; null = no split
  int splits, kt_per_split;
  int dstride;   // >1: strided data gradient — a source tap exists only where (h,w) are multiples of dstride (power of two)
  // Channel-slice views (round 4: the DAN context block writes its branches straight into the concat buffer and reads branch inputs
  // out of a wider tensor): pixel pitches in ELEMENTS of x, y and of the mask tensor of a data gradient (a slice [.., c0:c0+C] of an NHWC
  // tensor of width ld is its base pointer + c0 and pitch ld).  fwd_args / bwd_args set them to the dense values C / Co / Co;
  // conv_pointwise.hip, conv_igemm.hip (+ split-K finish) and conv_halo_c64.hip honour other values - strided() keeps the call off the rest.
  int ldx, ldy, ldm;
  int relu_co;   // forward: ReLU applies to output channels < relu_co only (fused 1x1 block whose last columns stay linear); default Co
  bool strided() const { return ldx != C || ldy != Co || (mask && ldm != Co) || (relu && relu_co < Co); }
  // (appended last: the layout of everything above is what the tuned kernels were built against)
  const bf16_t* x2;   // conv_pointwise.hip, forward 1x1: second source of the K axis (channels ksplit*64 .. C-1 of the virtual input [x | x2], same
  int ksplit;         // pixel pitch ldx as x); null = one source.  Only danhip_conv2d_fwd_concat2 sets them.
  // Split-operand evaluation (csrc/split_infer.hip; fp16 build, forward, Co % 8 == 0): y is the 3-limb-layout map [M][3 Co] of the NEXT
  // convolution — hi = half(v) at column co, lo = half(v - hi) at Co + co, hi again at 2 Co + co — written from the fp32 epilogue value.
  // Honoured by conv_halo.hip's general epilogue and by the flat-M kernel / split-K finish (conv_store4); every other kernel declines.
  int split_out;
  // conv_halo_c64.hip, data gradient of the SECOND layer (conv1_2) with the FIRST layer's weight gradient folded in (round 6): dx of this
  // call is conv1_1's dY; conv1_1 has no data gradient of its own, so dx's only reader would be conv_wgrad_c8.hip.  With fuse_dw set the
  // kernel keeps each dx tile in LDS, multiplies it with the tile's patch of the 8-channel image x8 (transposing reads, M = 12 tap slots x 4
  // channels, N = 64) into per-wave accumulators and never stores dx (y == NULL allowed): dw8 [3,3,cin_real,64] / db8 [64] fp32, atomically added.
  const bf16_t* fuse_x8;
  float* fuse_dw;
  float* fuse_db;
  int fuse_cin_real;
  // Split-operand evaluation (danhip_conv2d_fwd_split; 0 everywhere else): the forward epilogue computes v = fma(acc, 2^acc_exp, bias) - the
  // power of two undoes the exponents of the weights, of the input limbs and of the output map exactly, and costs nothing where a bias is
  // added anyway.  A limb-layout output raises *range_flag (if set) for a value the hi limb cannot hold (|v| >= 65520).
  int acc_exp;
  int* range_flag;
};

// 2^acc_exp (acc_exp in [-126, 127]) from the kernel argument with scalar integer operations
__device__ __forceinline__ float dh_acc_scale(const ConvArgs& a) { return __builtin_bit_cast(float, (a.acc_exp + 127) << 23); }

// *flag = 1 when one of the N values is outside half's finite range (|v| >= 65520 rounds hi to inf and lo to -inf: the next convolution would
// sum inf - inf = NaN, which a ReLU turns into 0); split_infer.hip, checked on the host by ops.split_range_check.  The maximum ignores a NaN:
// one can only come from an inf limb, which its writer flagged.
template <int N>
__device__ __forceinline__ void dh_range_check(const float* v, int* flag) {
  float m = fabsf(v[0]);
#pragma unroll
  for (int r = 1; r < N; ++r) m = fmaxf(m, fabsf(v[r]));
  if (!(m < 65520.f) && flag) *flag = 1;
}

// hi / lo limbs of 4 fp32 values as two packed pairs each (the build's 16-bit type: IEEE half where split_out is allowed)
__device__ __forceinline__ void dh_split4(const float v[4], uint2& hi, uint2& lo) {
  hi.x = pack2bf(v[0], v[1]);
  hi.y = pack2bf(v[2], v[3]);
  float h[4];
  unpack2bf(hi.x, h[0], h[1]);
  unpack2bf(hi.y, h[2], h[3]);
  lo.x = pack2bf(v[0] - h[0], v[1] - h[1]);
  lo.y = pack2bf(v[2] - h[2], v[3] - h[3]);
}

// the device flag the split-operand limb writers raise (split_infer.hip, danhip_split_set_range_flag; null = none)
int* danhip_split_range_flag();

// packed max of two pairs of NON-NEGATIVE 16-bit floats (ReLU outputs): they order like signed 16-bit integers, and a
// stray -0.0 (0x8000) is the smallest value.  One v_pk_max_i16.
typedef __attribute__((ext_vector_type(2))) short s16x2;
__device__ __forceinline__ unsigned pkmax_relu(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b)));
}

// ---- epilogue arithmetic shared by the tile kernels (measured with tools/halo2_trace.hip: the epilogues, not the waits around them, were
// the longest stretch without MFMAs).
// ReLU in ONE instruction (fmaxf compiles to a canonicalising v_max_f32 plus the max); max(NaN, 0) = 0 like fmaxf.
__device__ __forceinline__ float dh_relu(float v) {
  float r;
  asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(v));
  return r;
}
// Two packed 16-bit ReLU OUTPUTS (>= +0 and never NaN after dh_relu) -> 1 per half that is > 0: min(x, 1) as unsigned 16-bit integers
// (clang lowers the generic vector min to compares and selects, hence the asm).
typedef __attribute__((ext_vector_type(2))) unsigned short dh_u16x2;
typedef __attribute__((ext_vector_type(2))) unsigned dh_u32x2;
__device__ __forceinline__ dh_u16x2 dh_pos2(unsigned packed) {
  unsigned r;
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(packed), "s"(0x00010001u));
  return __builtin_bit_cast(dh_u16x2, r);
}
// bits | (value r of the 8 packed ReLU outputs > 0) << (SHIFT + r): one v_pk_min_u16 + one v_dot2_u32_u16 per register (danhip_relu_bits
// layout: bit r of the byte = channel 8 k + r)
template <int SHIFT>
__device__ __forceinline__ unsigned dh_pos_bits8_acc(const dh_u32x4& t, unsigned bits) {
  static_assert(SHIFT == 0 || SHIFT == 8, "16-bit weights");
#pragma unroll
  for (int e = 0; e < 4; ++e)
    bits = __builtin_amdgcn_udot2(dh_pos2(t[e]), dh_u16x2{(unsigned short)(1u << (SHIFT + 2 * e)), (unsigned short)(2u << (SHIFT + 2 * e))}, bits, false);
  return bits;
}
// ---- 2-bit arg-max codes of a 2x2 max-pool window, from the packed ReLU outputs the pooling epilogues hold (round 4: the pool's backward
// then scatters through the codes instead of re-reading the full-resolution activation).  a / b / c = top-left / top-right / bottom-left
// values of two channels per 32-bit word, m = the window maximum (pkmax_relu); all non-negative 16-bit floats, so they order as unsigned
// integers and m - x is 0 exactly where x is a maximum (packed ops: no borrow between the halves).  TF's MaxPoolGrad takes the FIRST maximum
// in row-major order (the rule of maxpool_bwd_kernel): code = 0 if a == m, else 1 if b == m, else 2 if c == m, else 3 = ne_a (1 + ne_b (1 + ne_c)).
__device__ __forceinline__ unsigned dh_pk_ne(unsigned m, unsigned x) {      // per half: 0 where x == m, 1 elsewhere
  unsigned d, r;
  asm("v_pk_sub_u16 %0, %1, %2" : "=v"(d) : "v"(m), "v"(x));
  asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(d), "s"(0x00010001u));
  return r;
}
__device__ __forceinline__ unsigned dh_argmax2x2_pk(unsigned a, unsigned b, unsigned c, unsigned m) {   // -> per half a code 0..3
  const unsigned na = dh_pk_ne(m, a), nb = dh_pk_ne(m, b), nc = dh_pk_ne(m, c);
  unsigned t, r;
  asm("v_pk_mad_u16 %0, %1, %2, %1" : "=v"(t) : "v"(nb), "v"(nc));         // nb * nc + nb
  asm("v_pk_mad_u16 %0, %1, %2, %1" : "=v"(r) : "v"(na), "v"(t));          // na * t + na
  return r;
}
// the eight codes of a lane's eight consecutive channels (four words of two) as 16 bits: channel j in bits 2j, 2j+1
__device__ __forceinline__ unsigned dh_argmax2x2_codes16(const dh_u32x4& a, const dh_u32x4& b, const dh_u32x4& c, const dh_u32x4& m) {
  unsigned out = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned w = dh_argmax2x2_pk(a[e], b[e], c[e], m[e]);
    out |= ((w | (w >> 14)) & 0xFu) << (4 * e);
  }
  return out;
}

// x | x(lane ^ 16) | x(lane ^ 32) | x(lane ^ 48) with the gfx950 row swaps (VALU) instead of two ds_bpermute round trips:
//   v_permlane16_swap(x, x) -> {rows [0,0,2,2], rows [1,1,3,3]};  v_permlane32_swap(y, y) -> {lower half twice, upper half twice}
__device__ __forceinline__ unsigned dh_or_rows(unsigned x) {
  const dh_u32x2 a = __builtin_amdgcn_permlane16_swap(x, x, false, false);
  const unsigned y = a[0] | a[1];
  const dh_u32x2 b = __builtin_amdgcn_permlane32_swap(y, y, false, false);
  return b[0] | b[1];
}
// value of lane ^ 1 (DPP quad_perm [1,0,3,2])
__device__ __forceinline__ unsigned dh_lane_xor1(unsigned v) { return (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true); }

// ---- kernel selection.  Every convolution call picks ONE kernel instance, and everything that has to know which - the launch, the
// kernel-label functions (danhip_conv_kernel_label / danhip_conv_wgrad_kernel_label: ops._prof_end and bench.py file measured time under
// these names) and the capability queries ops.py asks before each layer - reads the same selection:
//   * each family file exports one select(args) that returns its instance for these arguments or "not mine" (launch == nullptr); forward
//     or data gradient is decided there, by the family's own rule, from the arguments;
//   * select_conv (conv_igemm.hip) / select_wgrad (conv_wgrad.hip) hold the order of precedence between the families;
//   * dh_run_instance is the one place that calls an instance's launch function (and remembers its label for
//     danhip_conv_last_launch_label).
// A label is the exact demangled kernel name the profiler reports, written once, next to the template instance it names.
struct ConvInstance {
  const char* label = nullptr;
  int (*launch)(const ConvArgs&, hipStream_t) = nullptr;      // DANHIP_OK or a negative status
  // what THIS call gets from the instance (the queries of danhip.h build representative arguments and read these):
  bool fuses_pool = false;      // writes a.pool_y (2x2 max-pool of y) in its epilogue ...
  bool skips_y = false;         // ... and then takes y == NULL (only the pooled map is stored)
  bool emits_bits = false;      // forward: writes a.bits_out (and a.pool_bits_out beside a fused pool)
  bool takes_bits = false;      // data gradient: reads the ReLU mask as a.mask_bits
  bool folds_first = false;     // data gradient of conv1_2: folds conv1_1's weight gradient in (a.fuse_*), dx is never stored
  explicit operator bool() const { return launch != nullptr; }
};
ConvInstance conv_c8_select(const ConvArgs& a);          // conv_c8.hip: 8 (= 3 padded) -> 64 channel first layer, store-bound
ConvInstance conv_c64_select(const ConvArgs& a);         // conv_halo_c64.hip: 3x3, 64 -> 64 channels, register-resident weights (views too)
ConvInstance conv_halo_select(const ConvArgs& a);        // conv_halo.hip: halo-reuse 3x3 / stride 1 on large dense maps
ConvInstance conv_pointwise_select(const ConvArgs& a);   // conv_pointwise.hip: streaming GEMM, 1x1 (and tap forms) with 64-multiple channels

// A weight-gradient call (x / dy with pixel pitches ldx / ldy; ws: optional slab scratch) and its instance: conv_wgrad_rows.hip (3x3 'same',
// row-streaming), conv_wgrad_pw.hip (1x1, 256 x 256 gradient tile), conv_wgrad_c8.hip (first layer), else the generic tiles of conv_wgrad.hip.
struct WgradCall {
  const danhip_conv_desc* d;
  const bf16_t* x;
  const bf16_t* dy;
  float* dw;
  float* db;
  int cin_real, ldx, ldy;
  void* ws;
  size_t ws_bytes;
};
struct WgradInstance {
  const char* label = nullptr;
  int (*launch)(const WgradCall&, hipStream_t) = nullptr;
  explicit operator bool() const { return launch != nullptr; }
};
WgradInstance wgrad_rows_select(const WgradCall& c);
WgradInstance wgrad_pw_select(const WgradCall& c);
WgradInstance wgrad_c8_select(const WgradCall& c);
size_t wgrad_rows_workspace_bytes(const danhip_conv_desc* d);      // slab scratch the family's launch would use; 0 = none / not its shape
size_t wgrad_pw_workspace_bytes(const danhip_conv_desc* d);

size_t wgrad_c8_workspace_bytes(const WgradCall& c);                // deterministic mode only (0 otherwise / not its shape)
// The ordered cross-workgroup sum of deterministic mode (ordered_reduce.hip; the order: danhip.h): out[c] (+)= sum_p part[p * pitch + c].
int dh_ordered_reduce(const float* part, long pitch, int P, long C, float* out, int accumulate, hipStream_t s);

// label of the instance most recently launched on this thread (danhip_conv_last_launch_label); "" before the first launch
inline const char*& dh_last_launch_label() {
  static thread_local const char* label = "";
  return label;
}
// Launches the selected instance: its status, or 1 when the selection was "not mine".
template <class Instance, class Args>
int dh_run_instance(const Instance& inst, const Args& a, hipStream_t s) {
  if (!inst) return 1;
  dh_last_launch_label() = inst.label;
  return inst.launch(a, s);
}

// Epilogue for one lane's 4 consecutive output channels [co, co+4) of output pixel m (shared by both kernels).
__device__ __forceinline__ void conv_store4(const ConvArgs& a, float v[4], size_t m, int co) {
  if (co >= a.Co) return;
  const size_t o = m * (size_t)(a.split_out ? 3 * a.ldy : a.ldy) + co;      // output (pitched view: ldy elements per pixel; limb layout: three of them)
  const size_t om = m * (size_t)a.ldm + co;         // mask tensor of a data gradient
  const size_t orr = m * (size_t)a.Co + co;         // residual: always dense
  const bool full = (co + 4 <= a.Co) && ((a.Co & 3) == 0);
  if (a.bias) {
    const float sc = dh_acc_scale(a);
#pragma unroll
    for (int r = 0; r < 4; ++r) if (co + r < a.Co) v[r] = fmaf(v[r], sc, a.bias[co + r]);
  } else if (a.acc_exp) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] *= dh_acc_scale(a);
  }
  if (a.relu && co < a.relu_co) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
  }
  if (a.out_f32) {
    float* y = reinterpret_cast<float*>(a.y) + o;
    if (full) {
      float4 t = make_float4(v[0], v[1], v[2], v[3]);
      if (a.accumulate) { float4 u = *reinterpret_cast<float4*>(y); t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w; }
      *reinterpret_cast<float4*>(y) = t;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) if (co + r < a.Co) y[r] = a.accumulate ? y[r] + v[r] : v[r];
    }
  } else {
    bf16_t* y = reinterpret_cast<bf16_t*>(a.y) + o;
    if (a.split_out) {                                  // (forward only, Co % 8 == 0: always a full quad)
      dh_range_check<4>(v, a.range_flag);
      uint2 hi, lo;
      dh_split4(v, hi, lo);
      *reinterpret_cast<uint2*>(y) = hi;
      *reinterpret_cast<uint2*>(y + a.Co) = lo;
      *reinterpret_cast<uint2*>(y + 2 * a.Co) = hi;
      return;
    }
    if (full) {
      if (a.mask) {
        const uint2 mk = *reinterpret_cast<const uint2*>(a.mask + om);
        const bf16_t* mp = reinterpret_cast<const bf16_t*>(&mk);
#pragma unroll
        for (int r = 0; r < 4; ++r) if (!(bf2f(mp[r]) > 0.f)) v[r] = 0.f;
      }
      if (a.resid) {
        const uint2 rs = *reinterpret_cast<const uint2*>(a.resid + orr);
        const bf16_t* rp = reinterpret_cast<const bf16_t*>(&rs);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bf2f(rp[r]);
      }
      if (a.accumulate) {
        const uint2 old = *reinterpret_cast<const uint2*>(y);
        const bf16_t* op = reinterpret_cast<const bf16_t*>(&old);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += bf2f(op[r]);
      }
      uint2 t;
      t.x = pack2bf(v[0], v[1]);
      t.y = pack2bf(v[2], v[3]);
      *reinterpret_cast<uint2*>(y) = t;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (co + r < a.Co) {
          float t = v[r];
          if (a.mask && !(bf2f(a.mask[om + r]) > 0.f)) t = 0.f;
          if (a.resid) t += bf2f(a.resid[orr + r]);
          if (a.accumulate) t += bf2f(y[r]);
          y[r] = f2bf(t);
        }
      }
    }
  }
}
