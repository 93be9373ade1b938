// The one cross-workgroup sum of the deterministic mode (option "deterministic"): out[c] (+)= sum over p of part[p][c], fp32, in an order
// that is a function of P alone - never of the grid, of the CU count or of which workgroup finished first.  Every kernel that ends in
// float atomics by default stores its per-workgroup partial sums as rows of a caller-provided slab instead and hands the slab to this
// kernel (conv_wgrad.hip, conv_wgrad_c8.hip, the bias-gradient rows of conv_wgrad_rows.hip / conv_wgrad_pw.hip, elementwise.hip, loss.hip).
//
// THE ORDER (danhip.h, DESIGN.md "Deterministic mode"):
//   P <= DANHIP_ORDERED_REDUCE_SEQ_MAX:  S = (((part[0][c] + part[1][c]) + part[2][c]) + ...) + part[P-1][c]
//   P >  DANHIP_ORDERED_REDUCE_SEQ_MAX:  G = ceil(P / 4); S_k = the same sequential sum over rows [k G, min(P, (k+1) G)) for k = 0..3 (every group
//                                    holds at least one row: 3 G < P for P > 64); S = ((S_0 + S_1) + S_2) + S_3
//   out[c] = S, or out[c] = out[c] + S when accumulating: one add onto the old value.
// The four-group form keeps four independent add chains (and four 16-byte loads) in flight per lane where one chain of P dependent adds
// would be latency-bound (the first layer's gradient: P = CU count rows).
//
// A lane owns 4 consecutive columns and reads them as one 16-byte load per row: the kernel moves P x C x 4 bytes once and is HBM / L2 bound.
// No atomics, no LDS.  Rows whose pitch or column count is no multiple of 4 (or whose pointers are not 16-byte aligned) take the same
// arithmetic with 4-byte loads (a lane owns one column).
#include "common.h"

namespace {

template <typename V>
__device__ __forceinline__ V ordered_sum(const V* __restrict__ col, long pitch_v, int P) {
  if (P <= DANHIP_ORDERED_REDUCE_SEQ_MAX) {
    V s = __builtin_nontemporal_load(col);
    int p = 1;
    for (; p + 4 <= P; p += 4) {                         // four loads in flight, added in row order
      const V a = __builtin_nontemporal_load(col + (long)p * pitch_v), b = __builtin_nontemporal_load(col + (long)(p + 1) * pitch_v);
      const V c = __builtin_nontemporal_load(col + (long)(p + 2) * pitch_v), d = __builtin_nontemporal_load(col + (long)(p + 3) * pitch_v);
      s = s + a; s = s + b; s = s + c; s = s + d;
    }
    for (; p < P; ++p) s = s + __builtin_nontemporal_load(col + (long)p * pitch_v);
    return s;
  }
  const int G = (P + 3) >> 2;
  const int last = P - 3 * G;                            // rows of group 3 (1 .. G)
  const V* c0 = col;
  const V* c1 = col + (long)G * pitch_v;
  const V* c2 = col + (long)(2 * G) * pitch_v;
  const V* c3 = col + (long)(3 * G) * pitch_v;
  V s0 = __builtin_nontemporal_load(c0), s1 = __builtin_nontemporal_load(c1), s2 = __builtin_nontemporal_load(c2), s3 = __builtin_nontemporal_load(c3);
  int i = 1;
  for (; i + 1 < last; i += 2) {                         // eight loads in flight; each chain still adds its rows in ascending order
    const long o = (long)i * pitch_v, o1 = o + pitch_v;
    const V a = __builtin_nontemporal_load(c0 + o), b = __builtin_nontemporal_load(c1 + o), c = __builtin_nontemporal_load(c2 + o),
            d = __builtin_nontemporal_load(c3 + o);
    const V a1 = __builtin_nontemporal_load(c0 + o1), b1 = __builtin_nontemporal_load(c1 + o1), c1v = __builtin_nontemporal_load(c2 + o1),
            d1 = __builtin_nontemporal_load(c3 + o1);
    s0 = s0 + a; s1 = s1 + b; s2 = s2 + c; s3 = s3 + d;
    s0 = s0 + a1; s1 = s1 + b1; s2 = s2 + c1v; s3 = s3 + d1;
  }
  for (; i < last; ++i) {
    const long o = (long)i * pitch_v;
    const V a = __builtin_nontemporal_load(c0 + o), b = __builtin_nontemporal_load(c1 + o), c = __builtin_nontemporal_load(c2 + o),
            d = __builtin_nontemporal_load(c3 + o);
    s0 = s0 + a; s1 = s1 + b; s2 = s2 + c; s3 = s3 + d;
  }
  for (; i < G; ++i) {
    const long o = (long)i * pitch_v;
    const V a = __builtin_nontemporal_load(c0 + o), b = __builtin_nontemporal_load(c1 + o), c = __builtin_nontemporal_load(c2 + o);
    s0 = s0 + a; s1 = s1 + b; s2 = s2 + c;
  }
  return ((s0 + s1) + s2) + s3;
}

// V = f32x4 (pitch and C counted in float4s) or float
template <typename V>
__global__ __launch_bounds__(256) void ordered_reduce_kernel(const V* __restrict__ part, long pitch_v, int P, long Cv, V* __restrict__ out, int accumulate) {
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < Cv; c += (long)gridDim.x * blockDim.x) {
    const V s = ordered_sum<V>(part + c, pitch_v, P);
    out[c] = accumulate ? out[c] + s : s;
  }
}

}  // namespace

// part: P rows of C columns, `pitch` floats apart.  Asynchronous on `s`, allocates nothing.
int dh_ordered_reduce(const float* part, long pitch, int P, long C, float* out, int accumulate, hipStream_t s) {
  DH_REQUIRE(part && out && P >= 1 && C >= 1 && pitch >= C, DANHIP_EINVAL, "ordered_reduce: bad arguments (P=%d, C=%ld, pitch=%ld)", P, C, pitch);
  const bool vec = ((pitch | C) & 3) == 0 && ((((uintptr_t)part) | ((uintptr_t)out)) & 15) == 0;
  const long cols = vec ? C / 4 : C;
  long blocks = (cols + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (vec)
    hipLaunchKernelGGL(ordered_reduce_kernel<f32x4>, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const f32x4*>(part), pitch / 4, P, cols,
                       reinterpret_cast<f32x4*>(out), accumulate);
  else
    hipLaunchKernelGGL(ordered_reduce_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, part, pitch, P, cols, out, accumulate);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_ordered_reduce_f32(const float* part, int32_t P, int64_t C, float* out, int accumulate, void* stream) {
  return dh_ordered_reduce(part, (long)C, P, (long)C, out, accumulate, (hipStream_t)stream);
}

extern "C" size_t danhip_loss_workspace_bytes(void) { return DANHIP_LOSS_WS_BYTES; }
extern "C" size_t danhip_sgd_workspace_bytes(void) { return DANHIP_SGD_WS_BYTES; }

// Scratch of the _ws forms of the memory-bound kernels (elementwise.hip, loss.hip): one row of C partial sums per workgroup, for the
// largest grid any of them launches (2048 workgroups for danhip_relu_bwd_bias_grad_ws, 512 for the L2-norm pair; a function of M and C alone).
extern "C" size_t danhip_reduce_workspace_bytes(int64_t M, int32_t C) {
  if (M <= 0 || C <= 0) return 0;
  const int64_t rows = M < 2048 ? M : 2048;
  return (size_t)rows * (size_t)((C + 3) / 4 * 4) * sizeof(float);
}
