// Far corners of the deformable backward in deterministic mode (include/danhip.h, "Deformable backward in deterministic mode").
// The default path adds every corner outside the gather window to the fp32 side buffer far_dx with a float atomic (doff_far_corners in
// deform_conv.hip): the sum's order is the order the memory system happens to serve.  Here every far corner becomes a RECORD, the records
// are grouped by destination, and one 8-lane group per destination forms its 64 sums in ascending key order and stores them plainly:
//
//   1 count   one lane per source (output pixel, group, tap): far corners -> integer atomicAdd on count[dest]
//   2 scan    exclusive prefix sum of count -> start[0 .. dests] (three launches: block sums, their scan, the write)
//   3 fill    the same walk; a record's key goes to recs[start[dest] + --count[dest]]: ANY order inside a segment
//   4 sum     per destination: repeatedly take the smallest key above the last one taken (the fill order is gone after this), recompute the
//             record's weight from the offsets with corner_set, F = fma(w, dS, F); store F - or zeros for a destination without records
//
// Six launches whatever the offsets are, no host synchronisation, integer atomics only.  The key search costs L / 8 loads per lane and term for a
// segment of L records (L^2 / 8 in all): right for any L, fast for the short segments training produces.  When the statistic says that no offset
// leaves the window at all, every kernel returns at once and far_dx is not written (the dX kernel does not read it then).
#include "common.h"
#include "deform_far.h"

namespace {

struct FarArgs {
  DhFarGeom g;
  const unsigned* stat;    // stat[0] / stat[1] = offset pairs outside [-2, 2) / [-1, 1) (deform_far_stat_kernel)
  unsigned thresh1;
  int window;              // 0: by the statistic, 1 / 2: fixed
};
__device__ __forceinline__ int far_R(const FarArgs& a) { return dh_far_window(a.window, a.stat[1], a.thresh1); }
__device__ __forceinline__ bool far_any(const FarArgs& a, int R) { return a.stat[R == 1 ? 1 : 0] != 0u; }

// Exclusive prefix sum of one value per thread over a 256-thread workgroup; total = the workgroup's sum.  sh: 4 words.
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* sh, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  unsigned base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { if (i < wave) base += sh[i]; tot += sh[i]; }
  __syncthreads();
  total = tot;
  return base + inc - v;
}

template <bool FILL>
__global__ __launch_bounds__(256) void far_records_kernel(const unsigned* __restrict__ offw, FarArgs a, unsigned* __restrict__ count,
                                                          const unsigned* __restrict__ start, unsigned* __restrict__ recs, unsigned nsrc) {
  const int R = far_R(a);
  if (!far_any(a, R)) return;
  const DhFarGeom g = a.g;
  for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < nsrc; s += gridDim.x * 256u) {     // (nsrc < 2^30: no wrap)
    const unsigned oraw = offw[s];
    const float oh = dh_far_act2f((uint16_t)(oraw & 0xffffu)), ow = dh_far_act2f((uint16_t)(oraw >> 16));
    if (!dh_far_offset_outside(oh, ow, R)) continue;
    const int t = (int)(s % 9u);
    const unsigned q = s / 9u;
    const int grp = (int)(q % (unsigned)g.dg);
    const unsigned m = q / (unsigned)g.dg;
    const int wo = (int)(m % (unsigned)g.W);
    const unsigned mr = m / (unsigned)g.W;
    const int ho = (int)(mr % (unsigned)g.H), n = (int)(mr / (unsigned)g.H);
    CornerSet cs;
    const unsigned mask = dh_far_mask(g, ho, wo, t, oh, ow, R, cs);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!((mask >> k) & 1u)) continue;
      const unsigned d = dh_far_dest(g, n, cs.rh[k], cs.rw[k], grp);       // (corner_set accepted the corner: inside the image)
      if (FILL) recs[start[d] + (atomicSub(count + d, 1u) - 1u)] = dh_far_key(m, t, k);
      else atomicAdd(count + d, 1u);
    }
  }
}

__global__ __launch_bounds__(256) void far_scan_sums_kernel(const unsigned* __restrict__ count, unsigned ndest, unsigned* __restrict__ bsum, FarArgs a) {
  if (!far_any(a, far_R(a))) return;
  __shared__ unsigned sh[4];
  const unsigned i0 = blockIdx.x * DH_FAR_SCAN_BLOCK + threadIdx.x * 8u;
  unsigned v = 0;
#pragma unroll
  for (unsigned e = 0; e < 8; ++e) if (i0 + e < ndest) v += count[i0 + e];
  unsigned total;
  block_excl_scan(v, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum[b] <- sum of the blocks before b; *total_out = all records
__global__ __launch_bounds__(256) void far_scan_top_kernel(unsigned* __restrict__ bsum, unsigned nblk, unsigned* __restrict__ total_out, FarArgs a) {
  if (!far_any(a, far_R(a))) return;
  __shared__ unsigned sh[4];
  unsigned carry = 0;
  for (unsigned b0 = 0; b0 < nblk; b0 += 256u) {                            // (uniform)
    const unsigned b = b0 + threadIdx.x;
    const unsigned v = b < nblk ? bsum[b] : 0u;
    unsigned total;
    const unsigned ex = block_excl_scan(v, sh, total);
    if (b < nblk) bsum[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) *total_out = carry;
}

__global__ __launch_bounds__(256) void far_scan_write_kernel(const unsigned* __restrict__ count, unsigned ndest, const unsigned* __restrict__ bsum,
                                                             unsigned* __restrict__ start, FarArgs a) {
  if (!far_any(a, far_R(a))) return;
  __shared__ unsigned sh[4];
  const unsigned i0 = blockIdx.x * DH_FAR_SCAN_BLOCK + threadIdx.x * 8u;
  unsigned c[8], v = 0;
#pragma unroll
  for (unsigned e = 0; e < 8; ++e) { c[e] = i0 + e < ndest ? count[i0 + e] : 0u; v += c[e]; }
  unsigned total;
  unsigned run = bsum[blockIdx.x] + block_excl_scan(v, sh, total);
#pragma unroll
  for (unsigned e = 0; e < 8; ++e) {
    if (i0 + e < ndest) start[i0 + e] = run;
    run += c[e];
  }
}

// DH_FAR_LANES = 8 lanes own a destination; lane l8 holds 8 of its 64 channels and searches the keys l8, l8 + 8, ... of the segment.
__global__ __launch_bounds__(256) void far_sum_kernel(const unsigned* __restrict__ offw, const bf16_t* __restrict__ dS, const unsigned* __restrict__ start,
                                                      const unsigned* __restrict__ recs, float* __restrict__ far_dx, FarArgs a, unsigned ndest, int always) {
  const int R = far_R(a);
  const bool any = far_any(a, R);
  if (!any && !always) return;
  const DhFarGeom g = a.g;
  const int lane = threadIdx.x & 63, l8 = lane & 7;
  for (unsigned base = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 8u; base < ndest; base += gridDim.x * 32u) {      // (uniform in a wave; ndest < 2^31)
    const unsigned d = base + (unsigned)(lane >> 3);
    const bool live = d < ndest;
    unsigned s0 = 0, L = 0;
    if (live && any) { s0 = start[d]; L = start[d + 1] - s0; }
    const int grp = (int)(d % (unsigned)g.dg);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    unsigned done = 0, last = 0;
    while (__any(done < L)) {
      // the smallest key above `last` (any key in the first round): keys are unique inside a segment and below 2^32 - 1
      unsigned best = 0xffffffffu;
      if (done < L)
        for (unsigned i = (unsigned)l8; i < L; i += DH_FAR_LANES) {
          const unsigned key = recs[s0 + i];
          if ((done == 0 || key > last) && key < best) best = key;
        }
#pragma unroll
      for (int o = 1; o < DH_FAR_LANES; o <<= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 64));
      if (done < L) {
        const unsigned row = best >> 2, m = row / 9u;
        const int k = (int)(best & 3u), t = (int)(row % 9u);
        const int wo = (int)(m % (unsigned)g.W), ho = (int)((m / (unsigned)g.W) % (unsigned)g.H);
        const unsigned oraw = offw[((size_t)m * g.dg + grp) * 9u + t];
        CornerSet cs;
        dh_far_mask(g, ho, wo, t, dh_far_act2f((uint16_t)(oraw & 0xffffu)), dh_far_act2f((uint16_t)(oraw >> 16)), R, cs);
        float wk = cs.wg[0];
        if (k == 1) wk = cs.wg[1]; else if (k == 2) wk = cs.wg[2]; else if (k == 3) wk = cs.wg[3];
        float f[8];
        dh_unpack8(*reinterpret_cast<const uint4*>(dS + (size_t)row * g.C + grp * 64 + l8 * 8), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = dh_far_term(acc[e], wk, f[e]);
        last = best;
        ++done;
      }
    }
    if (live) {
      float* o = far_dx + (size_t)(d / (unsigned)g.dg) * g.C + grp * 64 + l8 * 8;
      *reinterpret_cast<float4*>(o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<float4*>(o + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    }
  }
}

}  // namespace

// The shape class of the ordered form and its 32-bit guards.  NULL: fine; otherwise what is wrong.
const char* danhip_deform_far_shape_error(int N, int H, int W, int C, int dg) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || dg <= 0 || C != dg * 64) return "C / deformable_group must be 64";
  const DhFarGeom g{N, H, W, C, dg};
  if (dh_far_sources(g) >= (1ull << 30)) return "N * H * W * deformable_group * 9 must stay below 2^30 (32-bit record ids)";
  return nullptr;
}

size_t danhip_deform_far_region_bytes(int N, int H, int W, int C, int dg) {
  const DhFarGeom g{N, H, W, C, dg};
  return (size_t)dh_far_layout(g).words * sizeof(uint32_t);
}

// far_dx fp32 [N,H,W,C] <- the ordered sums of the far corners (plain stores; untouched when the statistic reports no far offset, unless
// `always`).  stat: the 64 statistic words, already counted on this stream; region: danhip_deform_far_region_bytes, its count words zeroed.
int danhip_launch_deform_far_ordered(const uint16_t* offsets, const uint16_t* dS, float* far_dx, const unsigned* stat, uint32_t* region, int N, int H,
                                     int W, int C, int dg, int window, int always, hipStream_t s) {
  const DhFarGeom g{N, H, W, C, dg};
  const DhFarLayout l = dh_far_layout(g);
  const unsigned nsrc = (unsigned)dh_far_sources(g), ndest = (unsigned)dh_far_dests(g), nblk = (unsigned)l.nblk;
  const FarArgs a{g, stat, dh_far_thresh1(dh_far_sources(g)), window};
  unsigned *count = region + l.count, *start = region + l.start, *bsum = region + l.bsum, *recs = region + l.recs;
  const unsigned* offw = reinterpret_cast<const unsigned*>(offsets);
  const dim3 gsrc(dh_grid_for(nsrc, 256, 8192));
  hipLaunchKernelGGL(far_records_kernel<false>, gsrc, dim3(256), 0, s, offw, a, count, start, recs, nsrc);
  hipLaunchKernelGGL(far_scan_sums_kernel, dim3(nblk), dim3(256), 0, s, count, ndest, bsum, a);
  hipLaunchKernelGGL(far_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, nblk, start + ndest, a);
  hipLaunchKernelGGL(far_scan_write_kernel, dim3(nblk), dim3(256), 0, s, count, ndest, bsum, start, a);
  hipLaunchKernelGGL(far_records_kernel<true>, gsrc, dim3(256), 0, s, offw, a, count, start, recs, nsrc);
  hipLaunchKernelGGL(far_sum_kernel, dim3(dh_grid_for((long)(ndest + 7u) / 8 * 8, 32, 16384)), dim3(256), 0, s, offw, reinterpret_cast<const bf16_t*>(dS),
                     start, recs, far_dx, a, ndest, always);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}
