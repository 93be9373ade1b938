// Forward statistics of batch normalisation over (N,H,W) per channel, shared by the batch-norm entry points of layers2.hip and the
// fused batch-norm tails of bn_act.hip: both take their batch statistics from these two kernels, launched the same way.
#pragma once
#include "common.h"

namespace {

// Forward statistics: per-channel sum(x) and sum(x^2) in DOUBLE (per-thread accumulators, LDS reduction, one double atomic per channel per
// block).  The fp32 form lost the variance of a channel with |mean| >> std to the cancellation in E[x^2] - mean^2, and its 1024 serial
// fp32 atomics per channel alone cost up to 3e-6 of E[x^2] (tests/test_hbm_layers_gpu.py, bn-C64-shifted-loops / bn-C2048-random).  The
// square of a 16-bit value is exact in fp32, so every addend is exact and the sums carry 53 bits.
__global__ void bn_stats_kernel(const bf16_t* __restrict__ x, double* __restrict__ s1, double* __restrict__ s2, long M, int C) {
  const int cg = C / 8;
  const int g = threadIdx.x % cg, rsub = threadIdx.x / cg, tpr = blockDim.x / cg;
  double t1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (rsub < tpr) {
    for (long r = (long)blockIdx.x * tpr + rsub; r < M; r += (long)gridDim.x * tpr) {
      float f[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(x + r * C + g * 8), f);
#pragma unroll
      for (int i = 0; i < 8; ++i) { t1[i] += (double)f[i]; t2[i] += (double)(f[i] * f[i]); }
    }
  }
  extern __shared__ double redd[];
  double* r1 = redd;
  double* r2 = redd + blockDim.x * 8;
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

// mean/var from the (double) sums; optionally updates the moving averages: moving = moving*m + batch*(1-m).  tf.layers.batch_normalization
// on a 4-D input takes TF1's FUSED path, which normalises with the biased batch variance but feeds the moving average the Bessel-corrected
// one (var * M / (M - 1), nn_impl.fused_batch_norm's batch_var output)
__global__ void bn_finalize_kernel(const double* __restrict__ s1, const double* __restrict__ s2, float* __restrict__ mean, float* __restrict__ rstd,
                                   float* __restrict__ var_out, float* __restrict__ mov_mean, float* __restrict__ mov_var, double m, float eps,
                                   float momentum, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double mud = s1[c] / m;
  double vard = s2[c] / m - mud * mud;
  vard = vard > 0.0 ? vard : 0.0;
  const float mu = (float)mud, var = (float)vard;
  mean[c] = mu;
  rstd[c] = (float)(1.0 / sqrt(vard + (double)eps));
  if (var_out) var_out[c] = var;
  if (mov_mean) mov_mean[c] = mov_mean[c] * momentum + mu * (1.f - momentum);
  if (mov_var) {
    const float unbiased = m > 1.0 ? (float)(vard * (m / (m - 1.0))) : var;
    mov_var[c] = mov_var[c] * momentum + unbiased * (1.f - momentum);
  }
}

// launch shape of bn_stats_kernel / the backward's reduce kernels: a block is a whole number of rows of C/8 lanes
struct BnReduceGeom { int block, grid; };
static inline BnReduceGeom bn_reduce_geom(int64_t M, int32_t C) {
  const int cg = C / 8;
  BnReduceGeom g;
  g.block = cg <= 256 ? 256 / cg * cg : cg;        // multiple of cg (>= 1 row per block)
  const int tpr = g.block / cg;
  g.grid = (int)((M + tpr - 1) / tpr);
  if (g.grid > 1024) g.grid = 1024;
  return g;
}

}  // namespace
