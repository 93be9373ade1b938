// Fused batch-norm tails of the ResNet backbone (gfx950): batch norm (+ residual add) (+ ReLU) in ONE apply pass, and a backward that
// applies the ReLU mask on the fly in both of its passes.  net/resnet_danet.py:157-218 (conv_bn / conv_bn_relu / bottleneck_block).
//   forward   y = act((x - mean) rstd gamma + beta + shortcut)        fp32 sum, one rounding to 16 bits at the store
//   backward  g = dy [y > 0];  dbeta = sum g, dgamma = sum g xhat;  dx (training or frozen form) and dshortcut = g in one pass
// Streaming kernels in the style of layers2.hip: 8 channels per lane, 16-byte loads and stores, whole-line stores, fp32 arithmetic.
// The batch statistics are those of danhip_batchnorm_fwd_train: the same two kernels (bn_stats.h), launched the same way.
#include "common.h"
#include "bn_stats.h"

namespace {

// eight consecutive fp32 per-channel parameters (c0 a multiple of 8: 32-byte aligned) as two 16-byte loads
__device__ __forceinline__ void bn_load8(const float* __restrict__ p, int c0, float* f) {
  const float4 a = *reinterpret_cast<const float4*>(p + c0), b = *reinterpret_cast<const float4*>(p + c0 + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// y = act((x - mean) * rstd * gamma + beta + shortcut): 2 reads (1 without a shortcut) and 1 write of the map
__global__ void bn_act_apply_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ sc, const float* __restrict__ mean,
                                    const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                    bf16_t* __restrict__ y, long M, int C, int relu) {
  const int cg = C / 8;
  const long total = M * cg;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % cg) * 8;
    float f[8], s[8], mu[8], rs[8], ga[8], be[8];
    dh_unpack8(*reinterpret_cast<const uint4*>(x + idx * 8), f);
    if (sc) dh_unpack8(*reinterpret_cast<const uint4*>(sc + idx * 8), s);
    bn_load8(mean, c0, mu); bn_load8(rstd, c0, rs); bn_load8(gamma, c0, ga); bn_load8(beta, c0, be);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float v = (f[i] - mu[i]) * rs[i] * ga[i] + be[i];
      if (sc) v += s[i];
      f[i] = relu ? fmaxf(v, 0.f) : v;
    }
    *reinterpret_cast<uint4*>(y + idx * 8) = dh_pack8(f);
  }
}

// s1[c] += sum g, s2[c] += sum g * xhat with g = dy * [y > 0] (y == nullptr: g = dy).  Thread owns 8 channels and strides rows;
// block-level reduction through LDS; one fp32 atomic per channel per block (the shape of layers2.hip's bn_reduce_kernel).
__global__ void bn_act_reduce_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const bf16_t* __restrict__ y,
                                     const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ s1,
                                     float* __restrict__ s2, long M, int C) {
  const int cg = C / 8;
  const int g = threadIdx.x % cg, rsub = threadIdx.x / cg, tpr = blockDim.x / cg;
  float t1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float mu[8], rs[8];
  bn_load8(mean, g * 8, mu); bn_load8(rstd, g * 8, rs);
  if (rsub < tpr) {
    for (long r = (long)blockIdx.x * tpr + rsub; r < M; r += (long)gridDim.x * tpr) {
      float fd[8], fx[8], fy[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(dy + r * C + g * 8), fd);
      dh_unpack8(*reinterpret_cast<const uint4*>(x + r * C + g * 8), fx);
      if (y) dh_unpack8(*reinterpret_cast<const uint4*>(y + r * C + g * 8), fy);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float gi = (!y || fy[i] > 0.f) ? fd[i] : 0.f;
        t1[i] += gi;
        t2[i] += gi * ((fx[i] - mu[i]) * rs[i]);
      }
    }
  }
  extern __shared__ float red[];
  float* r1 = red;
  float* r2 = red + blockDim.x * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) { r1[threadIdx.x * 8 + i] = t1[i]; r2[threadIdx.x * 8 + i] = t2[i]; }
  __syncthreads();
  if (threadIdx.x < cg) {
    for (int k = 1; k < tpr; ++k)
#pragma unroll
      for (int i = 0; i < 8; ++i) { t1[i] += r1[(k * cg + threadIdx.x) * 8 + i]; t2[i] += r2[(k * cg + threadIdx.x) * 8 + i]; }
#pragma unroll
    for (int i = 0; i < 8; ++i) { atomicAdd(s1 + threadIdx.x * 8 + i, t1[i]); atomicAdd(s2 + threadIdx.x * 8 + i, t2[i]); }
  }
}

// g = dy * [y > 0];  training form: dx = gamma rstd (g - mean(g) - xhat mean(g xhat)) with sg = sum g, sgx = sum g xhat of the reduce
// pass;  frozen form (statistics are constants): dx = g gamma rstd, x is not read.  dsc = g (a 16-bit value or 0: exact) when asked for.
__global__ void bn_act_bwd_apply_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, const bf16_t* __restrict__ y,
                                        const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma,
                                        const float* __restrict__ sg, const float* __restrict__ sgx, bf16_t* __restrict__ dx,
                                        bf16_t* __restrict__ dsc, long M, int C, float inv_m, int frozen) {
  const int cg = C / 8;
  const long total = M * cg;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(idx % cg) * 8;
    float fd[8], fy[8], ga[8], rs[8], r[8];
    dh_unpack8(*reinterpret_cast<const uint4*>(dy + idx * 8), fd);
    if (y) {
      dh_unpack8(*reinterpret_cast<const uint4*>(y + idx * 8), fy);
#pragma unroll
      for (int i = 0; i < 8; ++i) fd[i] = fy[i] > 0.f ? fd[i] : 0.f;
    }
    bn_load8(gamma, c0, ga); bn_load8(rstd, c0, rs);
    if (frozen) {
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = fd[i] * ga[i] * rs[i];
    } else {
      float fx[8], mu[8], a[8], b[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(x + idx * 8), fx);
      bn_load8(mean, c0, mu); bn_load8(sg, c0, a); bn_load8(sgx, c0, b);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xh = (fx[i] - mu[i]) * rs[i];
        r[i] = ga[i] * rs[i] * (fd[i] - a[i] * inv_m - xh * b[i] * inv_m);
      }
    }
    *reinterpret_cast<uint4*>(dx + idx * 8) = dh_pack8(r);
    if (dsc) *reinterpret_cast<uint4*>(dsc + idx * 8) = dh_pack8(fd);
  }
}

int bn_act_check(const void* x, int64_t M, int32_t C, const char* what) {
  DH_REQUIRE(x != nullptr, DANHIP_EINVAL, "%s: null pointer", what);
  DH_REQUIRE(M > 0 && C > 0 && C % 8 == 0 && C <= 2048, DANHIP_EINVAL, "%s: bad dims (C %% 8 == 0, C <= 2048)", what);
  DH_REQUIRE(((uintptr_t)x & 15) == 0, DANHIP_EINVAL, "%s: the activations must be 16-byte aligned", what);
  return DANHIP_OK;
}
// per-channel fp32 arrays are read 16 bytes at a time
bool bn_act_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

}  // namespace

/* workspace: 2*C doubles, 8-byte aligned (sum x, sum x^2), zeroed inside - that of danhip_batchnorm_fwd_train */
extern "C" int danhip_bn_act_fwd_train(const uint16_t* x, const uint16_t* shortcut, const float* gamma, const float* beta, uint16_t* y,
                                       float* save_mean, float* save_rstd, float* moving_mean, float* moving_var, int64_t M, int32_t C,
                                       float eps, float momentum, int relu, float* workspace, void* stream) {
  int rc = bn_act_check(x, M, C, "bn_act_fwd_train");
  if (rc) return rc;
  DH_REQUIRE(danhip_option("deterministic") == 0, DANHIP_EINVAL, "bn_act_fwd_train: no deterministic form (option \"deterministic\" is set; its float atomics are out of that mode's scope)");
  DH_REQUIRE(gamma && beta && y && save_mean && save_rstd && workspace, DANHIP_EINVAL, "bn_act_fwd_train: null pointer");
  DH_REQUIRE(((uintptr_t)workspace & 7) == 0, DANHIP_EINVAL, "bn_act_fwd_train: the workspace (2*C doubles) must be 8-byte aligned");
  DH_REQUIRE(bn_act_aligned16(y, shortcut) && bn_act_aligned16(gamma, beta, save_mean, save_rstd), DANHIP_EINVAL,
             "bn_act_fwd_train: every array must be 16-byte aligned");
  double* sums = reinterpret_cast<double*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(sums, 0, sizeof(double) * 2 * C, s) != hipSuccess) { danhip_set_error("bn_act_fwd_train: memset failed"); return DANHIP_ELAUNCH; }
  const BnReduceGeom g = bn_reduce_geom(M, C);
  hipLaunchKernelGGL(bn_stats_kernel, dim3(g.grid), dim3(g.block), sizeof(double) * g.block * 16, s, x, sums, sums + C, (long)M, C);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, s, sums, sums + C, save_mean, save_rstd, (float*)nullptr,
                     moving_mean, moving_var, (double)M, eps, momentum, C);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_act_apply_kernel, dim3(dh_grid_for(M * (C / 8), 256, 8192)), dim3(256), 0, s, x, shortcut, save_mean, save_rstd, gamma,
                     beta, y, (long)M, C, relu);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

/* rstd = rsqrt(moving_var + eps) is supplied by the caller, as for danhip_batchnorm_fwd_infer */
extern "C" int danhip_bn_act_fwd_infer(const uint16_t* x, const uint16_t* shortcut, const float* gamma, const float* beta, const float* mean,
                                       const float* rstd, uint16_t* y, int64_t M, int32_t C, int relu, void* stream) {
  int rc = bn_act_check(x, M, C, "bn_act_fwd_infer");
  if (rc) return rc;
  DH_REQUIRE(danhip_option("deterministic") == 0, DANHIP_EINVAL, "bn_act_fwd_infer: no deterministic form (option \"deterministic\" is set; its float atomics are out of that mode's scope)");
  DH_REQUIRE(gamma && beta && mean && rstd && y, DANHIP_EINVAL, "bn_act_fwd_infer: null pointer");
  DH_REQUIRE(bn_act_aligned16(y, shortcut) && bn_act_aligned16(gamma, beta, mean, rstd), DANHIP_EINVAL,
             "bn_act_fwd_infer: every array must be 16-byte aligned");
  hipLaunchKernelGGL(bn_act_apply_kernel, dim3(dh_grid_for(M * (C / 8), 256, 8192)), dim3(256), 0, (hipStream_t)stream, x, shortcut, mean, rstd,
                     gamma, beta, y, (long)M, C, relu);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

/* dgamma[c] = sum g*xhat, dbeta[c] = sum g (both OVERWRITTEN; one memset when dbeta == dgamma + C), then dx / dshortcut: two launches */
extern "C" int danhip_bn_act_bwd(const uint16_t* x, const uint16_t* dy, const uint16_t* y, const float* gamma, const float* mean,
                                 const float* rstd, uint16_t* dx, uint16_t* dshortcut, float* dgamma, float* dbeta, int64_t M, int32_t C,
                                 int frozen, void* stream) {
  int rc = bn_act_check(x, M, C, "bn_act_bwd");
  if (rc) return rc;
  DH_REQUIRE(danhip_option("deterministic") == 0, DANHIP_EINVAL, "bn_act_bwd: no deterministic form (option \"deterministic\" is set; its float atomics are out of that mode's scope)");
  DH_REQUIRE(dy && gamma && mean && rstd && dx && dgamma && dbeta, DANHIP_EINVAL, "bn_act_bwd: null pointer");
  DH_REQUIRE(bn_act_aligned16(dy, y, dx, dshortcut) && bn_act_aligned16(gamma, mean, rstd) && bn_act_aligned16(dgamma, dbeta), DANHIP_EINVAL,
             "bn_act_bwd: every array must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const bool joined = dbeta == dgamma + C;
  if (hipMemsetAsync(dgamma, 0, sizeof(float) * C * (joined ? 2 : 1), s) != hipSuccess ||
      (!joined && hipMemsetAsync(dbeta, 0, sizeof(float) * C, s) != hipSuccess)) {
    danhip_set_error("bn_act_bwd: memset failed");
    return DANHIP_ELAUNCH;
  }
  const BnReduceGeom g = bn_reduce_geom(M, C);
  hipLaunchKernelGGL(bn_act_reduce_kernel, dim3(g.grid), dim3(g.block), sizeof(float) * g.block * 16, s, dy, x, y, mean, rstd, dbeta, dgamma,
                     (long)M, C);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_act_bwd_apply_kernel, dim3(dh_grid_for(M * (C / 8), 256, 8192)), dim3(256), 0, s, x, dy, y, mean, rstd, gamma, dbeta,
                     dgamma, dx, dshortcut, (long)M, C, 1.0f / (float)M, frozen);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}
