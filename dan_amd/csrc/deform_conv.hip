// Deformable convolution sampling for gfx950 — the arithmetic of cpp/Deform/deform_conv.cu (deformable_im2col_bilinear
// :91-126, deformable_im2col_gpu_kernel :229-275, deformable_col2im_coord_gpu_kernel :335-389 + get_coordinate_weight
// :177-221, deformable_col2im_gpu_kernel :281-328 + get_gradient_weight :130-173) restated for NHWC bf16 tensors.
//
// DeformConvOp (cpp/Deform/deform_conv.cc:392-535) = per sample { deformable im2col ; GEMM with W[Cout, Cin*kh*kw] }.
// Here the im2col is the batched kernel below writing S[pixel][tap*C + c] (bf16, K-contiguous), and the GEMM is the MFMA
// convolution kernel run as a 1x1 convolution over S (forward, data gradient = dS, weight gradient) — see
// dan_amd/ops.py:deform_conv_op.  DeformConvBackpropOp (:635-771): dS = dY * W (1x1 data gradient), then
// deform_sample_bwd produces dOffset (gather over the group's channels) and dX (bilinear scatter, fp32 atomics as the
// reference does with CudaAtomicAdd :314-326).
//
// Offsets: NHWC [B,Ho,Wo, dg*2*kh*kw], channel (g*kh*kw + t)*2 + {0: dh, 1: dw}  (deform_conv.cu:251-259).
// The three sampling rules themselves live in deform_sample.h; the kernels here keep their addressing, load scheduling and reductions.
#include "deform_sample.h"

namespace {

struct DeformGeom {
  int N, H, W, C, Ho, Wo, kh, kw, stride, dil, dg, pad_t, pad_l;
};

// A 256-thread block owns SAMPLE_PXB consecutive output pixels of ONE output row: (image, row, first column) are block-uniform
// (scalar registers) and a thread's item q -> (pixel in the block, tap, 8-channel chunk) is 32-bit arithmetic — the earlier form (one
// flat 64-bit index per thread, five 64-bit divisions each) spent more instructions on its index than on the four 16-byte gathers.
// Items run chunk-fastest, then tap: a wave stores 1 KiB of S contiguously and its corner loads are whole 128-byte group rows.
constexpr int SAMPLE_PXB = 8;
__global__ __launch_bounds__(256) void deform_sample_fwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ offs, bf16_t* __restrict__ S,
                                                                DeformGeom g, int segs, int cch_shift) {
  const int taps = g.kh * g.kw, cch = g.C / 8, cpg8 = g.C / g.dg / 8;
  const int offc = g.dg * 2 * taps;
  const int seg = (int)(blockIdx.x % (unsigned)segs);
  const int rowid = (int)(blockIdx.x / (unsigned)segs);                 // n * Ho + ho
  const int ho = rowid % g.Ho, n = rowid / g.Ho;
  const int wo0 = seg * SAMPLE_PXB;
  const int npx = min(SAMPLE_PXB, g.Wo - wo0);
  const int items = npx * taps * cch;
  const int h_in = ho * g.stride - g.pad_t;
  const long m0 = (long)rowid * g.Wo + wo0;
  const bf16_t* xn = x + ((long)n * g.H * g.W) * g.C;
  // Three items per trip: the three offset words are fetched first, then all twelve corner rows are in flight together — a trip
  // costs two dependent memory latencies instead of six (the kernel is latency bound, not bandwidth bound: 16 bytes per lane and load).
  constexpr int U = 3;
  for (int q0 = threadIdx.x; q0 < items; q0 += 256 * U) {
    int chunk[U], t[U], pxl[U], grp[U];
    bool live[U];
    unsigned oraw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int q = q0 + u * 256;
      live[u] = q < items;
      if (!live[u]) q = items - 1;
      int r;
      if (cch_shift >= 0) { chunk[u] = q & (cch - 1); r = q >> cch_shift; } else { chunk[u] = q % cch; r = q / cch; }
      pxl[u] = r / taps; t[u] = r - pxl[u] * taps;
      grp[u] = chunk[u] / cpg8;
      oraw[u] = *reinterpret_cast<const unsigned*>(offs + (m0 + pxl[u]) * offc + (grp[u] * taps + t[u]) * 2);
    }
    uint4 c4[U][4];
    DeformFwdTap tap[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = t[u] / g.kw, j = t[u] - i * g.kw;
      const int w_in = (wo0 + pxl[u]) * g.stride - g.pad_l;
      const DeformOffset off = deform_offset_pair(oraw[u]);
      const DeformFwdTap s = deform_fwd_tap(h_in, w_in, i * g.dil, j * g.dil, off.h, off.w, g.H, g.W);
      tap[u] = s;
      const bf16_t* base = xn + chunk[u] * 8;
      const int rl = (h_in + s.h_low) * g.W + w_in, rh = (h_in + s.h_high) * g.W + w_in;  // pixel indices inside image n
      c4[u][0] = *reinterpret_cast<const uint4*>(base + (long)(rl + s.w_low) * g.C);
      c4[u][1] = *reinterpret_cast<const uint4*>(base + (long)(rl + s.w_high) * g.C);
      c4[u][2] = *reinterpret_cast<const uint4*>(base + (long)(rh + s.w_low) * g.C);
      c4[u][3] = *reinterpret_cast<const uint4*>(base + (long)(rh + s.w_high) * g.C);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float v1[8], v2[8], v3[8], v4[8], out[8];
      dh_unpack8(c4[u][0], v1); dh_unpack8(c4[u][1], v2); dh_unpack8(c4[u][2], v3); dh_unpack8(c4[u][3], v4);
#pragma unroll
      for (int e = 0; e < 8; ++e) out[e] = tap[u].in ? deform_blend(tap[u].wq, v1[e], v2[e], v3[e], v4[e]) : 0.f;
      if (live[u]) *reinterpret_cast<uint4*>(S + ((m0 + pxl[u]) * taps + t[u]) * g.C + chunk[u] * 8) = dh_pack8(out);
    }
  }
}

// backward: dS [M][taps*C] -> dOffset [M][dg*2*taps] (bf16, written), dX fp32 [N,H,W,C] (atomic +=, zero it first)
// thread = (m, t, 8-channel chunk); the chunks of one deformable group are consecutive lanes (cpg8 a power of two <= 32)
__global__ void deform_sample_bwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ offs, const bf16_t* __restrict__ dS,
                                         float* __restrict__ dx, bf16_t* __restrict__ doffs, DeformGeom g) {
  const int taps = g.kh * g.kw, cch = g.C / 8, cpg8 = g.C / g.dg / 8;
  const long total = (long)g.N * g.Ho * g.Wo * taps * cch;
  const int offc = g.dg * 2 * taps;
  const long total_pad = (total + blockDim.x - 1) / blockDim.x * blockDim.x;        // keep whole waves alive for the shuffles
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total_pad; idx += (long)gridDim.x * blockDim.x) {
    const bool live = idx < total;
    const long id = live ? idx : total - 1;
    const int chunk = (int)(id % cch);
    long r = id / cch;
    const int t = (int)(r % taps);
    const long m = r / taps;
    const int wo = (int)(m % g.Wo);
    const int ho = (int)((m / g.Wo) % g.Ho);
    const int n = (int)(m / ((long)g.Wo * g.Ho));
    const int grp = chunk / cpg8;
    const int i = t / g.kw, j = t % g.kw;
    const int h_in = ho * g.stride - g.pad_t, w_in = wo * g.stride - g.pad_l;
    const bf16_t* op = offs + m * offc + (grp * taps + t) * 2;
    const float inv_h = (float)(h_in + i * g.dil) + bf2f(op[0]);      // absolute sample coordinate (:365-366, :304-305)
    const float inv_w = (float)(w_in + j * g.dil) + bf2f(op[1]);
    float cg[8];
    dh_unpack8(*reinterpret_cast<const uint4*>(dS + (m * taps + t) * g.C + chunk * 8), cg);
    const bf16_t* base = x + ((long)n * g.H * g.W) * g.C + chunk * 8;
    // ---- dOffset: get_coordinate_weight; out-of-range samples give 0
    float s_h = 0.f, s_w = 0.f;
    const DeformCoordWeights cw = deform_coord_weights(inv_h, inv_w, g.H, g.W);
    if (cw.in) {
      float vll[8], vlh[8], vhl[8], vhh[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(base + ((long)cw.hl * g.W + cw.wl) * g.C), vll);
      dh_unpack8(*reinterpret_cast<const uint4*>(base + ((long)cw.hl * g.W + cw.wh) * g.C), vlh);
      dh_unpack8(*reinterpret_cast<const uint4*>(base + ((long)cw.hh * g.W + cw.wl) * g.C), vhl);
      dh_unpack8(*reinterpret_cast<const uint4*>(base + ((long)cw.hh * g.W + cw.wh) * g.C), vhh);
      deform_coord_sum8(cw, vll, vlh, vhl, vhh, cg, s_h, s_w);
    }
    if (!live) { s_h = 0.f; s_w = 0.f; }
    for (int o = 1; o < cpg8; o <<= 1) { s_h += __shfl_xor(s_h, o); s_w += __shfl_xor(s_w, o); }
    if (live && (chunk % cpg8) == 0) {
      bf16_t* dp = doffs + m * offc + (grp * taps + t) * 2;
      dp[0] = f2bf(s_h);
      dp[1] = f2bf(s_w);
    }
    // ---- dX: get_gradient_weight scattered to the <= 4 corners
    const CornerSet cs = corner_set(inv_h, inv_w, g.H, g.W);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (live && cs.ok[k]) {
        float* dst = dx + (((long)n * g.H + cs.rh[k]) * g.W + cs.rw[k]) * g.C + chunk * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) atomicAdd(dst + e, cs.wg[k] * cg[e]);
      }
    }
  }
}


// ---- which backward form runs is decided ON THE DEVICE (no host synchronisation, capturable): the gather form below enumerates source
// taps within +-DEFORM_R of an input pixel and hands every corner outside that window to fp32 atomics one by one ("far" corners) — 3.2 ms
// at 160 x 160 x 256 with offsets of N(0, 0.5 px), but 43 ms at N(0, 2 px), where 85 % of the taps have a far corner; the all-atomics
// scatter form costs 12 ms whatever the offsets are.  deform_far_stat_kernel counts the (dh, dw) pairs outside [-2, 2) and [-1, 1) into
// stat[0..1] (zeroed with the scatter buffer); every backward kernel reads them and returns at once when it belongs to another form.
struct BwdGate {
  const unsigned* stat;   // stat[0] / stat[1] = number of offset pairs with a component outside [-2, 2) / [-1, 1)
  unsigned thresh2;       // scatter form when stat[0] > thresh2
  unsigned thresh1;       // gather window +-1 (81 candidates instead of 225) when stat[1] <= thresh1
  int force;              // option "deform_bwd_form": 0 by the statistics, 1 gather +-2, 2 scatter, 3 gather +-1
};
// form: 0 = gather with a +-1 window, 1 = gather with a +-2 window, 2 = scatter
__device__ __forceinline__ int gate_form(const BwdGate& q) {
  if (q.force) return q.force == 3 ? 0 : q.force;
  if (q.stat[0] > q.thresh2) return 2;
  return q.stat[1] <= q.thresh1 ? 0 : 1;
}
__device__ __forceinline__ bool gate_runs(const BwdGate& q, int form) { return gate_form(q) == form; }

// Fast path for C / deformable_group == 64: one WAVE per (output pixel, tap, deformable group), lane = channel.  Every
// atomic wave-instruction then adds 64 consecutive floats (256 contiguous bytes — the full-rate shape of the memory-side
// float atomics), and the offset gradient is a plain 64-lane reduction.
__global__ void deform_sample_bwd_c64_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ offs, const bf16_t* __restrict__ dS,
                                             float* __restrict__ dx, bf16_t* __restrict__ doffs, DeformGeom g, BwdGate gate) {
  if (gate.stat && !gate_runs(gate, 2)) return;
  const int taps = g.kh * g.kw;
  const int offc = g.dg * 2 * taps;
  const int lane = threadIdx.x & 63;
  const long nwork = (long)g.N * g.Ho * g.Wo * taps * g.dg;              // (m, t, grp) triples, grp fastest
  const long wave0 = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
  for (long wk = wave0; wk < nwork; wk += nwaves) {
    const int grp = (int)(wk % g.dg);
    long r = wk / g.dg;
    const int t = (int)(r % taps);
    const long m = r / taps;
    const int wo = (int)(m % g.Wo);
    const int ho = (int)((m / g.Wo) % g.Ho);
    const int n = (int)(m / ((long)g.Wo * g.Ho));
    const int i = t / g.kw, j = t % g.kw;
    const int h_in = ho * g.stride - g.pad_t, w_in = wo * g.stride - g.pad_l;
    const bf16_t* op = offs + m * offc + (grp * taps + t) * 2;
    const float inv_h = (float)(h_in + i * g.dil) + bf2f(op[0]);
    const float inv_w = (float)(w_in + j * g.dil) + bf2f(op[1]);
    const int c = grp * 64 + lane;
    const float cg = bf2f(dS[(m * taps + t) * g.C + c]);
    const bf16_t* base = x + ((long)n * g.H * g.W) * g.C + c;
    // ---- dOffset (get_coordinate_weight)
    float s_h = 0.f, s_w = 0.f;
    const DeformCoordWeights cw = deform_coord_weights(inv_h, inv_w, g.H, g.W);
    if (cw.in) {
      const float vll = bf2f(base[((long)cw.hl * g.W + cw.wl) * g.C]), vlh = bf2f(base[((long)cw.hl * g.W + cw.wh) * g.C]);
      const float vhl = bf2f(base[((long)cw.hh * g.W + cw.wl) * g.C]), vhh = bf2f(base[((long)cw.hh * g.W + cw.wh) * g.C]);
      s_h = (-1.f * cw.a_w * vll + -1.f * cw.b_w * vlh + cw.a_w * vhl + cw.b_w * vhh) * cg;
      s_w = (-1.f * cw.a_h * vll + cw.a_h * vlh + -1.f * cw.b_h * vhl + cw.b_h * vhh) * cg;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s_h += __shfl_xor(s_h, o, 64); s_w += __shfl_xor(s_w, o, 64); }
    if (lane == 0) {
      bf16_t* dp = doffs + m * offc + (grp * taps + t) * 2;
      dp[0] = f2bf(s_h);
      dp[1] = f2bf(s_w);
    }
    // ---- dX (get_gradient_weight), wave-uniform corner geometry
    const CornerSet cs = corner_set(inv_h, inv_w, g.H, g.W);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (cs.ok[k]) atomicAdd(dx + (((long)n * g.H + cs.rh[k]) * g.W + cs.rw[k]) * g.C + c, cs.wg[k] * cg);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Atomic-free backward for the shape the context modules use (3x3 taps, stride 1, C / deformable_group == 64).
// L2 float atomics run at ~1.4 TB/s on this part and the scatter issues 36 of them (256 B each) per output pixel and group, so the
// col2im is turned around: a wave owns one INPUT pixel (x 64 channels), enumerates the (output pixel, tap) pairs whose nominal sampling
// position lies within +-R pixels, evaluates get_gradient_weight for each in one lane, and accumulates the matching dS rows — a
// deterministic gather.  Corners further than R from their nominal position (offsets beyond ~R-1 px) keep the memory atomic
// (`far` below); the two sets are complementary by construction.  dOffset needs no atomics at all: one wave per (output pixel, group)
// has all nine taps' loads in flight and reduces the 18 sums with a transposing butterfly (29 shuffles instead of 108).

__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// The 18 sums of an item, spread over its 8 lanes -> lane l8 holds the (dh, dw) pair of tap (4*b0 + 2*b1 + b2) and stores it as one 32-bit
// word: a transposing butterfly (14 + 6 shuffles).  `dp` = the item's 18 bf16 of dOffset (an even element index: 32-bit aligned pairs).
__device__ __forceinline__ void doff_reduce_store(const float (&sv)[18], bool live, bf16_t* __restrict__ dp, int lane) {
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
  // 16 of the 18 sums: after the step with partner distance d a lane keeps the half its bit selects
  float r8[8], r4[4], r2[2];
#pragma unroll
  for (int j = 0; j < 8; ++j) r8[j] = (b0 ? sv[j + 8] : sv[j]) + __shfl_xor(b0 ? sv[j] : sv[j + 8], 1, 64);
#pragma unroll
  for (int j = 0; j < 4; ++j) r4[j] = (b1 ? r8[j + 4] : r8[j]) + __shfl_xor(b1 ? r8[j] : r8[j + 4], 2, 64);
#pragma unroll
  for (int j = 0; j < 2; ++j) r2[j] = (b2 ? r4[j + 2] : r4[j]) + __shfl_xor(b2 ? r4[j] : r4[j + 2], 4, 64);
  float e0 = sv[16], e1 = sv[17];
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) { e0 += __shfl_xor(e0, o, 64); e1 += __shfl_xor(e1, o, 64); }
  if (live) {
    *reinterpret_cast<unsigned*>(dp + (b0 ? 8 : 0) + (b1 ? 4 : 0) + (b2 ? 2 : 0)) = pack2bf(r2[0], r2[1]);
    if ((lane & 7) == 0) *reinterpret_cast<unsigned*>(dp + 16) = pack2bf(e0, e1);
  }
}

// Far corners: not reachable by the gather kernels' +-R enumeration.  A corner that corner_set() accepts sits floor(o) or
// floor(o) + 1 from the nominal position (under the high-edge clamp the only candidate one further away, H - 1 for a position of
// exactly H, fails the |position - corner| < 1 guard), so offsets in [-R, R) cannot produce one: the whole search is skipped then.
// `farm` = the item's taps with an offset outside [-R, R); uo / ud = the item's offsets and (lane's piece of the) dS rows.
template <int R>
__device__ __forceinline__ void doff_far_corners(unsigned farm, bool live, const bf16_t* __restrict__ uo, const bf16_t* __restrict__ ud,
                                                 float* __restrict__ far_dx, const DeformGeom& g, int n, int h_in, int w_in, int grp, int l8) {
  if (!__any(live && farm != 0)) return;
  if (!live) farm = 0;
  while (farm) {                                                        // (uniform inside an 8-lane item; rare)
    const int t = __builtin_ctz(farm);
    farm &= farm - 1;
    const DeformOffset off = deform_offset_pair(*reinterpret_cast<const unsigned*>(uo + 2 * t));
    const int nh = h_in + (t / 3) * g.dil, nw = w_in + (t % 3) * g.dil;
    const CornerSet cs = corner_set((float)nh + off.h, (float)nw + off.w, g.H, g.W);
    bool any_far = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) any_far = any_far || (cs.ok[k] && (abs(cs.rh[k] - nh) > R || abs(cs.rw[k] - nw) > R));
    if (!any_far) continue;
    float cg[8];
    dh_unpack8(*reinterpret_cast<const uint4*>(ud + t * g.C), cg);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool far = abs(cs.rh[k] - nh) > R || abs(cs.rw[k] - nw) > R;
      if (cs.ok[k] && far) {
        float* dst = far_dx + (((long)n * g.H + cs.rh[k]) * g.W + cs.rw[k]) * g.C + grp * 64 + l8 * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) atomicAdd(dst + e, cs.wg[k] * cg[e]);
      }
    }
  }
}

// dOffset (+ the far corners' atomics into the fp32 side buffer): EIGHT LANES per (output pixel, group) — lane l8 owns 8 of the group's
// 64 channels, i.e. one 16-byte piece of every row it touches, so the 45 loads of an item are 16-byte lane accesses (the earlier
// wave-per-item form issued them as 2-byte ones: eight times the load instructions for the same bytes).  The sampling geometry is
// recomputed by each of the 8 lanes (cheaper than handing it around); the 18 sums are reduced over the 8 lanes with a transposing
// butterfly (14 + 6 shuffles) after which lane l8 holds the (dh, dw) pair of tap (4*b0 + 2*b1 + b2) and stores it as one 32-bit word.
template <int R>
__device__ __forceinline__ void deform_bwd_doff9_c64_body(const bf16_t* __restrict__ x, const bf16_t* __restrict__ offs,
                                                          const bf16_t* __restrict__ dS, float* __restrict__ far_dx,
                                                          bf16_t* __restrict__ doffs, const DeformGeom& g) {
  const int offc = g.dg * 18;
  const int lane = threadIdx.x & 63, l8 = lane & 7;
  const unsigned nwork = (unsigned)g.N * g.Ho * g.Wo * g.dg;            // (< 2^31: checked by the launcher)
  const float lim = (float)R;
  for (unsigned wbase = (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 8u; wbase < nwork; wbase += gridDim.x * (blockDim.x >> 6) * 8u) {
    const unsigned item = wbase + (lane >> 3);
    const bool live = item < nwork;
    const unsigned wk = live ? item : nwork - 1;
    const int grp = (int)(wk % (unsigned)g.dg);
    const unsigned m = wk / (unsigned)g.dg;
    const int wo = (int)(m % (unsigned)g.Wo);
    const unsigned mr = m / (unsigned)g.Wo;
    const int ho = (int)(mr % (unsigned)g.Ho), n = (int)(mr / (unsigned)g.Ho);
    const int h_in = ho - g.pad_t, w_in = wo - g.pad_l;
    const bf16_t* ub = x + ((long)n * g.H * g.W) * g.C + grp * 64 + l8 * 8;
    const bf16_t* ud = dS + (long)m * 9 * g.C + grp * 64 + l8 * 8;
    const bf16_t* uo = offs + (long)m * offc + grp * 18;
    float sv[18];
    unsigned farm = 0;                                                  // taps whose offset may reach a corner beyond +-R
#pragma unroll
    for (int tb = 0; tb < 3; ++tb) {
      uint4 v[3][4], cgr[3];
      DeformCoordWeights cw[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int t = tb * 3 + u;
        // (decoded in place: through deform_offset_pair hipcc turns the range test below into compares that cost the fp16 build 8 bytes of scratch)
        const unsigned oraw = *reinterpret_cast<const unsigned*>(uo + 2 * t);
        const float off_h = bf2f((bf16_t)(oraw & 0xffffu)), off_w = bf2f((bf16_t)(oraw >> 16));
        if (off_h < -lim || off_h >= lim || off_w < -lim || off_w >= lim) farm |= 1u << t;
        cw[u] = deform_coord_weights((float)(h_in + tb * g.dil) + off_h, (float)(w_in + u * g.dil) + off_w, g.H, g.W);
        const DeformCoordWeights& c = cw[u];
        v[u][0] = *reinterpret_cast<const uint4*>(ub + (long)(c.hl * g.W + c.wl) * g.C);
        v[u][1] = *reinterpret_cast<const uint4*>(ub + (long)(c.hl * g.W + c.wh) * g.C);
        v[u][2] = *reinterpret_cast<const uint4*>(ub + (long)(c.hh * g.W + c.wl) * g.C);
        v[u][3] = *reinterpret_cast<const uint4*>(ub + (long)(c.hh * g.W + c.wh) * g.C);
        cgr[u] = *reinterpret_cast<const uint4*>(ud + t * g.C);
      }
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        float vll[8], vlh[8], vhl[8], vhh[8], cg[8];
        dh_unpack8(v[u][0], vll); dh_unpack8(v[u][1], vlh); dh_unpack8(v[u][2], vhl); dh_unpack8(v[u][3], vhh); dh_unpack8(cgr[u], cg);
        float s_h = 0.f, s_w = 0.f;
        deform_coord_sum8(cw[u], vll, vlh, vhl, vhh, cg, s_h, s_w);
        sv[2 * (tb * 3 + u)] = s_h;
        sv[2 * (tb * 3 + u) + 1] = s_w;
      }
    }
    doff_reduce_store(sv, live, doffs + (long)m * offc + grp * 18, lane);
    doff_far_corners<R>(farm, live, uo, ud, far_dx, g, n, h_in, w_in, grp, l8);
  }
}

// dX: one wave per (input pixel, group), lane = candidate during the enumeration, lane = channel during the accumulation
// ONE launch for both gather windows (the window is picked from the statistics at run time): a form that does not run must not cost a
// launch of its own on a 65536-block grid (~150 us to retire empty; DAN-Deform has 12 of these calls per step).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void deform_bwd_doff9_c64_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ offs,
                                                                   const bf16_t* __restrict__ dS, float* __restrict__ far_dx,
                                                                   bf16_t* __restrict__ doffs, DeformGeom g, BwdGate gate) {
  const int form = gate_form(gate);
  if (form == 0) deform_bwd_doff9_c64_body<1>(x, offs, dS, far_dx, doffs, g);
  else if (form == 1) deform_bwd_doff9_c64_body<2>(x, offs, dS, far_dx, doffs, g);
}

template <int R>
__device__ __forceinline__ void deform_bwd_dx_gather9_c64_body(const bf16_t* __restrict__ offs, const bf16_t* __restrict__ dS,
                                                               const float* __restrict__ far_dx, bf16_t* __restrict__ dx, const DeformGeom& g,
                                                               int accumulate, const bf16_t* __restrict__ relu_x) {
  constexpr int D = 2 * R + 1, NC = D * D * 9, ROUNDS = (NC + 63) / 64;
  const int offc = g.dg * 18;
  const int lane = threadIdx.x & 63;
  const long nwork = (long)g.N * g.H * g.W * g.dg;
  const long wave0 = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
  for (long wk = wave0; wk < nwork; wk += nwaves) {
    const int grp = (int)(wk % g.dg);
    const long p = wk / g.dg;
    const int w = (int)(p % g.W);
    const int h = (int)((p / g.W) % g.H);
    const int n = (int)(p / ((long)g.W * g.H));
    const int c = grp * 64 + lane;
    unsigned oraw[ROUNDS];
    int row[ROUNDS], nhv[ROUNDS], nwv[ROUNDS];
    bool valid[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int cand = r * 64 + lane;
      const int t = cand % 9, pos = cand / 9;
      nhv[r] = h + pos / D - R;
      nwv[r] = w + pos % D - R;
      const int ho = nhv[r] + g.pad_t - (t / 3) * g.dil, wo = nwv[r] + g.pad_l - (t % 3) * g.dil;     // stride 1
      valid[r] = cand < NC && ho >= 0 && ho < g.Ho && wo >= 0 && wo < g.Wo;
      const long m = valid[r] ? ((long)n * g.Ho + ho) * g.Wo + wo : 0;
      row[r] = (int)(m * 9 + t);
      oraw[r] = *reinterpret_cast<const unsigned*>(offs + m * offc + (grp * 9 + t) * 2);
    }
    float wgt[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const DeformOffset off = deform_offset_pair(oraw[r]);
      const float wv = corner_weight_at((float)nhv[r] + off.h, (float)nwv[r] + off.w, h, w, g.H, g.W);
      wgt[r] = valid[r] ? wv : 0.f;
    }
    float acc = 0.f;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      unsigned long long mask = __ballot(wgt[r] != 0.f);
      while (mask) {                                                    // four dS rows in flight per trip
        float w4[4];
        int r4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (mask) {
            const int b = __builtin_ctzll(mask);
            mask &= mask - 1;
            w4[q] = lane_f(wgt[r], b);
            r4[q] = __builtin_amdgcn_readlane(row[r], b);
          } else { w4[q] = 0.f; r4[q] = 0; }
        }
        bf16_t d4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) d4[q] = (dS + (long)r4[q] * g.C + grp * 64)[lane];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc += w4[q] * bf2f(d4[q]);
      }
    }
    const long o = p * g.C + c;
    float out = acc + far_dx[o];
    if (relu_x && !(bf2f(relu_x[o]) > 0.f)) out = 0.f;              // x is a ReLU output: its producer's ReLU backward, folded in here
    if (accumulate) out += bf2f(dx[o]);
    dx[o] = f2bf(out);
  }
}

// (8 waves per SIMD: the gather is two dependent global-load phases per item - offsets, then the dS rows they select - so it lives on
// occupancy; capping it at 64 VGPRs (4 spilled in the +-2 px body) measured 2.02 -> 1.96 ms at zero offsets, 3.20 -> 3.02 at sigma = 0.3 px
// (160 x 160 x 256, batch 16).  The opposite trade - prefetching the next item's offsets, 90 VGPRs, 5 waves - was 7-13 % SLOWER.)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void deform_bwd_dx_gather9_c64_kernel(const bf16_t* __restrict__ offs, const bf16_t* __restrict__ dS,
                                                                        const float* __restrict__ far_dx, bf16_t* __restrict__ dx, DeformGeom g,
                                                                        int accumulate, BwdGate gate, const bf16_t* __restrict__ relu_x) {
  const int form = gate_form(gate);
  if (form == 0) deform_bwd_dx_gather9_c64_body<1>(offs, dS, far_dx, dx, g, accumulate, relu_x);
  else if (form == 1) deform_bwd_dx_gather9_c64_body<2>(offs, dS, far_dx, dx, g, accumulate, relu_x);
}

constexpr int DT_H = 8, DT_W = 16;

// dOffset in a +-R window (R = 1, 2), TILE form (round 5).  The item-per-8-lanes kernel above reads the four bilinear corners of all nine taps
// from L1 / L2: 36 sixteen-byte gathers of x per 9 of dS, and at 160 x 160 x 256 (batch 16) the cache pipes, not HBM, set its 0.77 ms.
// Here a 256-thread block owns an 8 x 16 tile of OUTPUT pixels of one group and stages the group's 64 channels of the x pixels any tap
// with an offset in [-R, R) can touch (tile +-(R + 1): 12 x 20 pixels, 30 KB for R = 1) in LDS once; the corner gathers become ds_read_b128.
// A tap whose corners leave the staged region (offset outside [-R, R): rare in the form the statistic picks) takes the global loads.  Arithmetic,
// reduction and the far corners' atomics are the item kernel's.  3 x 3, stride 1, dilation 1, C / deformable_group == 64.
template <int R>
__device__ __forceinline__ void deform_bwd_doff_tile_c64_body(const bf16_t* __restrict__ x, const bf16_t* __restrict__ offs,
                                                              const bf16_t* __restrict__ dS, float* __restrict__ far_dx,
                                                              bf16_t* __restrict__ doffs, const DeformGeom& g, int tiles_h, int tiles_w, uint4* sx) {
  constexpr int DT_RH = DT_H + 2 * (R + 1), DT_RW = DT_W + 2 * (R + 1);
  // XCD-aware order: workgroup i runs on XCD i % 8; each XCD walks a contiguous eighth of the (image, tile, group) items, so the four groups of
  // a tile (the same offset lines, neighbouring slices of the same x / dS rows) and the overlapping regions of neighbouring tiles meet in ONE L2
  const unsigned nitems = (unsigned)g.N * (unsigned)tiles_h * (unsigned)tiles_w * (unsigned)g.dg, per_xcd = (nitems + 7u) / 8u;
  unsigned b = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  if (b >= nitems) return;                                               // (uniform; the grid is 8 * per_xcd)
  const int grp = (int)(b % (unsigned)g.dg); b /= (unsigned)g.dg;
  const int tw0 = (int)(b % (unsigned)tiles_w) * DT_W; b /= (unsigned)tiles_w;
  const int th0 = (int)(b % (unsigned)tiles_h) * DT_H;
  const int n = (int)(b / (unsigned)tiles_h);
  const int offc = g.dg * 18;
  const bf16_t* xn = x + ((long)n * g.H * g.W) * g.C + grp * 64;
  for (int idx = threadIdx.x; idx < DT_RH * DT_RW * 8; idx += 256) {
    const int px = idx >> 3, pc = idx & 7;
    const int hh = th0 - (R + 1) + px / DT_RW, ww = tw0 - (R + 1) + px % DT_RW;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (hh >= 0 && hh < g.H && ww >= 0 && ww < g.W) v = *reinterpret_cast<const uint4*>(xn + (long)(hh * g.W + ww) * g.C + pc * 8);
    sx[idx] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, l8 = lane & 7;
  const int slot = threadIdx.x >> 3;
  const int pw = slot % DT_W, ph0 = slot / DT_W;
#pragma unroll 1
  for (int bt = 0; bt < 4; ++bt) {
    const int ho_raw = th0 + 2 * bt + ph0, wo_raw = tw0 + pw;
    const bool live = ho_raw < g.Ho && wo_raw < g.Wo;
    const int ho = live ? ho_raw : g.Ho - 1, wo = live ? wo_raw : g.Wo - 1;
    const long m = ((long)n * g.Ho + ho) * g.Wo + wo;
    const int h_in = ho - g.pad_t, w_in = wo - g.pad_l;
    const bf16_t* ub = xn + l8 * 8;
    const bf16_t* ud = dS + m * 9 * g.C + grp * 64 + l8 * 8;
    const bf16_t* uo = offs + m * offc + grp * 18;
    unsigned farm = 0;                                                  // taps whose offset may reach a corner beyond +-R
    bf16_t* dp = doffs + m * offc + grp * 18;
    // A tap ROW at a time, the loop kept rolled: unrolled over all nine taps hipcc computes every tap's geometry up front (290 VGPRs).
    // The row's six sums are reduced over the item's 8 lanes by a transposing butterfly (4 + 2 + 1 shuffles): lane l8 ends with sum
    // 4*b0 + 2*b1 + b2 (6 and 7 are padding) and stores it as one 16-bit value.
#pragma unroll 1
    for (int tb = 0; tb < 3; ++tb) {
      uint4 cgr[3];
      unsigned orw[3];
#pragma unroll
      for (int u = 0; u < 3; ++u) { cgr[u] = *reinterpret_cast<const uint4*>(ud + (tb * 3 + u) * g.C); orw[u] = *reinterpret_cast<const unsigned*>(uo + 2 * (tb * 3 + u)); }
      float sv[8];
      sv[6] = 0.f; sv[7] = 0.f;
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const DeformOffset off = deform_offset_pair(orw[u]);
        if (off.h < -(float)R || off.h >= (float)R || off.w < -(float)R || off.w >= (float)R) farm |= 1u << (tb * 3 + u);
        const DeformCoordWeights c = deform_coord_weights((float)(h_in + tb) + off.h, (float)(w_in + u) + off.w, g.H, g.W);
        const int rl = c.hl - (th0 - (R + 1)), rh = c.hh - (th0 - (R + 1)), cl = c.wl - (tw0 - (R + 1)), ch = c.wh - (tw0 - (R + 1));
        const bool staged = rl >= 0 && rh < DT_RH && cl >= 0 && ch < DT_RW;
        uint4 v0 = make_uint4(0, 0, 0, 0), v1 = v0, v2 = v0, v3 = v0;
        if (c.in && staged) {
          v0 = sx[(rl * DT_RW + cl) * 8 + l8]; v1 = sx[(rl * DT_RW + ch) * 8 + l8];
          v2 = sx[(rh * DT_RW + cl) * 8 + l8]; v3 = sx[(rh * DT_RW + ch) * 8 + l8];
        }
        if (__any(c.in && !staged)) {                                   // (an offset outside [-R, R): rare in this form)
          if (c.in && !staged) {
            v0 = *reinterpret_cast<const uint4*>(ub + (long)(c.hl * g.W + c.wl) * g.C); v1 = *reinterpret_cast<const uint4*>(ub + (long)(c.hl * g.W + c.wh) * g.C);
            v2 = *reinterpret_cast<const uint4*>(ub + (long)(c.hh * g.W + c.wl) * g.C); v3 = *reinterpret_cast<const uint4*>(ub + (long)(c.hh * g.W + c.wh) * g.C);
          }
        }
        // get_coordinate_weight's two sums, with the corner weights (the same for every channel) taken out of the channel sum: four dot
        // products of the packed dS piece with the packed corner pieces (v_dot2c: 16 instructions, nothing unpacked - the loop was
        // VALU-bound on 40 unpacks + 80 multiply-adds per tap), then s_h = a_w (D_hl - D_ll) + b_w (D_hh - D_lh), s_w likewise
        const unsigned cgw[4] = {cgr[u].x, cgr[u].y, cgr[u].z, cgr[u].w};
        const unsigned w0[4] = {v0.x, v0.y, v0.z, v0.w}, w1[4] = {v1.x, v1.y, v1.z, v1.w}, w2[4] = {v2.x, v2.y, v2.z, v2.w}, w3[4] = {v3.x, v3.y, v3.z, v3.w};
        float d_ll = 0.f, d_lh = 0.f, d_hl = 0.f, d_hh = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          d_ll = dh_dot2(cgw[e], w0[e], d_ll); d_lh = dh_dot2(cgw[e], w1[e], d_lh);
          d_hl = dh_dot2(cgw[e], w2[e], d_hl); d_hh = dh_dot2(cgw[e], w3[e], d_hh);
        }
        sv[2 * u] = c.a_w * (d_hl - d_ll) + c.b_w * (d_hh - d_lh);
        sv[2 * u + 1] = c.a_h * (d_lh - d_ll) + c.b_h * (d_hh - d_hl);
      }
      const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
      float r4[4], r2[2];
#pragma unroll
      for (int j = 0; j < 4; ++j) r4[j] = (b0 ? sv[j + 4] : sv[j]) + __shfl_xor(b0 ? sv[j] : sv[j + 4], 1, 64);
#pragma unroll
      for (int j = 0; j < 2; ++j) r2[j] = (b1 ? r4[j + 2] : r4[j]) + __shfl_xor(b1 ? r4[j] : r4[j + 2], 2, 64);
      const float r1 = (b2 ? r2[1] : r2[0]) + __shfl_xor(b2 ? r2[0] : r2[1], 4, 64);
      const int which = (b0 ? 4 : 0) + (b1 ? 2 : 0) + (b2 ? 1 : 0);
      if (live && which < 6) dp[tb * 6 + which] = f2bf(r1);
    }
    if (far_dx) doff_far_corners<R>(farm, live, uo, ud, far_dx, g, n, h_in, w_in, grp, l8);   // (NULL: deterministic mode, deform_far.hip has them)
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void deform_bwd_doff_tile_c64_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ offs,
                                                                       const bf16_t* __restrict__ dS, float* __restrict__ far_dx,
                                                                       bf16_t* __restrict__ doffs, DeformGeom g, BwdGate gate, int tiles_h, int tiles_w) {
  __shared__ uint4 sx[(DT_H + 6) * (DT_W + 6) * 8];                     // the +-2 window's region: 14 x 22 pixels x 128 B = 39 KB
  const int form = gate_form(gate);
  if (form == 0) deform_bwd_doff_tile_c64_body<1>(x, offs, dS, far_dx, doffs, g, tiles_h, tiles_w, sx);
  else if (form == 1) deform_bwd_doff_tile_c64_body<2>(x, offs, dS, far_dx, doffs, g, tiles_h, tiles_w, sx);
}

// dX in a +-R window (R = 1: 81 candidates per input pixel, R = 2: 225), TILE form (round 5).  The wave-per-pixel gather above spends its life on memory round trips: per input pixel and
// group it loads 81 candidates' offsets from 81 scattered 4-byte places, then the dS rows they select as 2-byte lane accesses (1.96 ms at
// 160 x 160 x 256, batch 16, zero offsets: 9 rows per pixel).  Here a 256-thread block owns an 8 x 16 tile of INPUT pixels of one group:
// the offsets of every (output pixel, tap) that can reach the tile (output pixels within +-(R + 1): 12 x 20 x 9 words for R = 1) are staged in LDS once,
// EIGHT lanes own a pixel (lane l8 = 8 of the group's 64 channels = one 16-byte piece of each dS row), the 81 candidates are weighed
// eight at a time (one per lane, offsets from LDS), and every non-zero one is handed to the pixel's eight lanes by two ds_bpermutes and
// accumulated from ONE 16-byte load per lane.  Same candidate set, same weights (corner_weight_at) and the same order (candidate
// index ascending) as the wave-per-pixel form: deterministic, no atomics; far corners as before (the fp32 side buffer, read only when
// the statistic says an offset left [-R, R) at all).  3 x 3, stride 1, dilation 1, C / deformable_group == 64.

template <int R>
__device__ __forceinline__ void deform_bwd_dx_tile_c64_body(const bf16_t* __restrict__ offs, const bf16_t* __restrict__ dS,
                                                            const float* __restrict__ far_dx, bf16_t* __restrict__ dx, const DeformGeom& g,
                                                            int accumulate, const BwdGate& gate, const bf16_t* __restrict__ relu_x, int tiles_h,
                                                            int tiles_w, unsigned* soff) {
  constexpr int DT_RH = DT_H + 2 * (R + 1), DT_RW = DT_W + 2 * (R + 1), D = 2 * R + 1, NC = D * D * 9, ROUNDS = (NC + 7) / 8;
  // XCD-aware order: workgroup i runs on XCD i % 8; each XCD walks a contiguous eighth of the (image, tile, group) items, so the four groups of
  // a tile (the same offset lines, neighbouring slices of the same x / dS rows) and the overlapping regions of neighbouring tiles meet in ONE L2
  const unsigned nitems = (unsigned)g.N * (unsigned)tiles_h * (unsigned)tiles_w * (unsigned)g.dg, per_xcd = (nitems + 7u) / 8u;
  unsigned b = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
  if (b >= nitems) return;                                               // (uniform; the grid is 8 * per_xcd)
  const int grp = (int)(b % (unsigned)g.dg); b /= (unsigned)g.dg;
  const int tw0 = (int)(b % (unsigned)tiles_w) * DT_W; b /= (unsigned)tiles_w;
  const int th0 = (int)(b % (unsigned)tiles_h) * DT_H;
  const int n = (int)(b / (unsigned)tiles_h);
  const int offc = g.dg * 18;
  const bool has_far = gate.stat[R == 1 ? 1 : 0] != 0u;                     // an offset outside [-R, R) exists at all
  {
    const unsigned far_away = (unsigned)f2bf(60000.f) * 0x10001u;            // a position no pixel is near: weight 0
    for (int idx = threadIdx.x; idx < DT_RH * DT_RW * 9; idx += 256) {
      const int t = idx % 9, r = idx / 9;
      const int ho = th0 - (R + 1) + r / DT_RW, wo = tw0 - (R + 1) + r % DT_RW;
      unsigned v = far_away;
      if (ho >= 0 && ho < g.Ho && wo >= 0 && wo < g.Wo)
        v = *reinterpret_cast<const unsigned*>(offs + (((long)n * g.Ho + ho) * g.Wo + wo) * offc + (grp * 9 + t) * 2);
      soff[idx] = v;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, l8 = lane & 7, gbase = lane & 56;
  const int slot = threadIdx.x >> 3;                                         // 0..31: pixel (2 * bt + slot / 16, slot % 16) of the tile in batch bt
  const int pw = slot % DT_W, ph0 = slot / DT_W;
  const int w = tw0 + pw;
  const bf16_t* dsg = dS + grp * 64 + l8 * 8;
  // (batch outermost, one pixel's eight sums live at a time: 8 waves per SIMD — the loop is two dependent round trips per candidate round)
#pragma unroll 1
  for (int bt = 0; bt < 4; ++bt) {
    const int ph = 2 * bt + ph0, h = th0 + ph;
    const bool pvalid = h < g.H && w < g.W;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll 1
    for (int r = 0; r < ROUNDS; ++r) {
      const int cand = r * 8 + l8;
      const bool live = cand < NC && pvalid;
      const int t = cand % 9, pos = cand < NC ? cand / 9 : (D * D) / 2;
      const int dh = pos / D - R, dw = pos % D - R;
      const int ti = t / 3, tj = t % 3;
      // output pixel of the candidate: (nominal position) + pad - tap, pad = 1: row h + dh + 1 - ti, staged at row index (that) - (th0 - R - 1)
      const int nh = h + dh, nw = w + dw;
      const unsigned oraw = soff[((ph + dh + R + 2 - ti) * DT_RW + (pw + dw + R + 2 - tj)) * 9 + t];
      const DeformOffset off = deform_offset_pair(oraw);
      float wv = corner_weight_at((float)nh + off.h, (float)nw + off.w, h, w, g.H, g.W);
      if (!live) wv = 0.f;
      const int row = (((n * g.Ho + (nh + 1 - ti)) * g.Wo) + (nw + 1 - tj)) * 9 + t;       // (used only where wv != 0: a valid output pixel)
      unsigned m8 = (unsigned)(__ballot(wv != 0.f) >> gbase) & 0xffu;
      while (__any(m8 != 0u)) {                                              // four dS rows in flight per trip and pixel
        float w4[4];
        int r4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool has = m8 != 0u;
          const int src = gbase + (has ? __builtin_ctz(m8) : 0);
          m8 &= m8 - 1u;
          const float wq = __shfl(wv, src, 64);
          const int rq = __shfl(row, src, 64);
          w4[q] = has ? wq : 0.f;
          r4[q] = has ? rq : 0;
        }
        uint4 d4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) d4[q] = *reinterpret_cast<const uint4*>(dsg + (long)r4[q] * g.C);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float f[8];
          dh_unpack8(d4[q], f);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += w4[q] * f[e];
        }
      }
    }
    if (!pvalid) continue;
    const long o = (((long)n * g.H + h) * g.W + w) * g.C + grp * 64 + l8 * 8;
    if (has_far) {
      const float4 fa = *reinterpret_cast<const float4*>(far_dx + o), fb = *reinterpret_cast<const float4*>(far_dx + o + 4);
      acc[0] += fa.x; acc[1] += fa.y; acc[2] += fa.z; acc[3] += fa.w; acc[4] += fb.x; acc[5] += fb.y; acc[6] += fb.z; acc[7] += fb.w;
    }
    if (relu_x) {                                                            // x is a ReLU output: its producer's ReLU backward, folded in here
      float m[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(relu_x + o), m);
#pragma unroll
      for (int e = 0; e < 8; ++e) if (!(m[e] > 0.f)) acc[e] = 0.f;
    }
    if (accumulate) {
      float old[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(dx + o), old);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += old[e];
    }
    *reinterpret_cast<uint4*>(dx + o) = dh_pack8(acc);
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void deform_bwd_dx_tile_c64_kernel(const bf16_t* __restrict__ offs, const bf16_t* __restrict__ dS,
                                                                     const float* __restrict__ far_dx, bf16_t* __restrict__ dx, DeformGeom g,
                                                                     int accumulate, BwdGate gate, const bf16_t* __restrict__ relu_x, int tiles_h,
                                                                     int tiles_w) {
  __shared__ unsigned soff[(DT_H + 6) * (DT_W + 6) * 9];                     // the +-2 window's region: 14 x 22 output pixels x 9 taps = 11 KB
  const int form = gate_form(gate);
  if (form == 0) deform_bwd_dx_tile_c64_body<1>(offs, dS, far_dx, dx, g, accumulate, gate, relu_x, tiles_h, tiles_w, soff);
  else if (form == 1) deform_bwd_dx_tile_c64_body<2>(offs, dS, far_dx, dx, g, accumulate, gate, relu_x, tiles_h, tiles_w, soff);
}

// The fp32 side buffer is needed only when a corner can fall outside the gather window or the scatter form runs: both imply an offset
// outside [-1, 1) (stat[1] != 0) unless a form is forced.  420 MB of zero stores per call at 160 x 160 x 256, batch 16, otherwise.
__global__ void zero_if_far_kernel(uint4* __restrict__ p16, long n16, const unsigned* __restrict__ stat, int force) {
  if (!(stat[1] != 0u || force == 1 || force == 2)) return;
  const uint4 z = make_uint4(0, 0, 0, 0);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) p16[i] = z;
}

__global__ void f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long n8, int accumulate, BwdGate gate,
                                   const bf16_t* __restrict__ relu_x) {
  if (gate.stat && !gate_runs(gate, 2)) return;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    const float4 a = *reinterpret_cast<const float4*>(src + i * 8), b = *reinterpret_cast<const float4*>(src + i * 8 + 4);
    float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    if (relu_x) {
      float m[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(relu_x + i * 8), m);
#pragma unroll
      for (int e = 0; e < 8; ++e) if (!(m[e] > 0.f)) f[e] = 0.f;
    }
    if (accumulate) {
      float o[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(dst + i * 8), o);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] += o[e];
    }
    *reinterpret_cast<uint4*>(dst + i * 8) = dh_pack8(f);
  }
}

// offsets bf16 [pairs][2] -> stat[0] / stat[1] += number of pairs with dh or dw outside [-2, 2) / [-1, 1)
__global__ __launch_bounds__(256) void deform_far_stat_kernel(const bf16_t* __restrict__ offs, long pairs, unsigned* __restrict__ stat) {
  unsigned c2 = 0, c1 = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (long)gridDim.x * blockDim.x) {
    const DeformOffset d = deform_offset_pair(reinterpret_cast<const unsigned*>(offs)[i]);
    c2 += (!(d.h >= -2.f && d.h < 2.f) || !(d.w >= -2.f && d.w < 2.f)) ? 1u : 0u;
    c1 += (!(d.h >= -1.f && d.h < 1.f) || !(d.w >= -1.f && d.w < 1.f)) ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { c2 += __shfl_xor(c2, o, 64); c1 += __shfl_xor(c1, o, 64); }
  __shared__ unsigned part[2][4];                                        // one atomic per block and word (8192 waves queued on one address: 100 us)
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = c2; part[1][threadIdx.x >> 6] = c1; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned v = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
    if (v) atomicAdd(stat + threadIdx.x, v);
  }
}

int make_geom(DeformGeom* g, int N, int H, int W, int C, int kh, int kw, int stride, int dil, int dg, const char* what) {
  DH_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && kh > 0 && kw > 0 && stride > 0 && dil > 0 && dg > 0, DANHIP_EINVAL, "%s: non-positive dims", what);
  DH_REQUIRE(C % dg == 0 && (C / dg) % 8 == 0, DANHIP_EINVAL, "%s: C/deformable_group must be a multiple of 8", what);
  const int cpg8 = C / dg / 8;
  DH_REQUIRE((cpg8 & (cpg8 - 1)) == 0 && cpg8 <= 32, DANHIP_EINVAL, "%s: C/deformable_group/8 must be a power of two <= 32", what);
  g->N = N; g->H = H; g->W = W; g->C = C; g->kh = kh; g->kw = kw; g->stride = stride; g->dil = dil; g->dg = dg;
  g->Ho = (H + stride - 1) / stride;
  g->Wo = (W + stride - 1) / stride;
  // SAME pad_before from the UNDILATED kernel (deform_conv.cc:473-479)
  g->pad_t = dh_same_pad_before(H, g->Ho, kh, stride);
  g->pad_l = dh_same_pad_before(W, g->Wo, kw, stride);
  DH_REQUIRE((int64_t)N * g->Ho * g->Wo * kh * kw * C < (1ll << 40), DANHIP_EINVAL, "%s: tensor too large", what);
  return DANHIP_OK;
}

}  // namespace

/* S [N*Ho*Wo, kh*kw*C] bf16 = deformable im2col of x [N,H,W,C] under offsets [N,Ho,Wo,dg*2*kh*kw] (both bf16). */
extern "C" int danhip_deform_sample_fwd(const uint16_t* x, const uint16_t* offsets, uint16_t* S, int32_t N, int32_t H, int32_t W, int32_t C,
                                        int32_t kh, int32_t kw, int32_t stride, int32_t dilation, int32_t deformable_group, void* stream) {
  DH_REQUIRE(x && offsets && S, DANHIP_EINVAL, "deform_sample_fwd: null pointer");
  DeformGeom g;
  int rc = make_geom(&g, N, H, W, C, kh, kw, stride, dilation, deformable_group, "deform_sample_fwd");
  if (rc) return rc;
  const int segs = (g.Wo + SAMPLE_PXB - 1) / SAMPLE_PXB, cch = C / 8;
  const long blocks = (long)N * g.Ho * segs;
  DH_REQUIRE(blocks < (1l << 31), DANHIP_EINVAL, "deform_sample_fwd: %ld output row segments", blocks);
  int shift = -1;
  if ((cch & (cch - 1)) == 0) { shift = 0; while ((1 << shift) < cch) ++shift; }
  hipLaunchKernelGGL(deform_sample_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, offsets, S, g, segs, shift);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" size_t danhip_deform_sample_bwd_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
  return ((size_t)N * H * W * C + 64) * sizeof(float);
}

// deform_far.hip: the ordered far-corner path of deterministic mode
const char* danhip_deform_far_shape_error(int N, int H, int W, int C, int dg);
size_t danhip_deform_far_region_bytes(int N, int H, int W, int C, int dg);
int danhip_launch_deform_far_ordered(const uint16_t* offsets, const uint16_t* dS, float* far_dx, const unsigned* stat, uint32_t* region, int N, int H,
                                     int W, int C, int dg, int window, int always, hipStream_t s);

extern "C" size_t danhip_deform_sample_bwd_ordered_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t deformable_group) {
  if (danhip_deform_far_shape_error(N, H, W, C, deformable_group)) return 0;
  return danhip_deform_sample_bwd_workspace_bytes(N, H, W, C) + danhip_deform_far_region_bytes(N, H, W, C, deformable_group);
}

// zero the statistic and the count words behind it, count the statistic, run the far path: far_dx = workspace[0 .. N*H*W*C)
static int deform_far_ordered_run(const uint16_t* offsets, const uint16_t* dS, int N, int H, int W, int C, int dg, int window, int always, float* workspace,
                                  hipStream_t s) {
  const long nx = (long)N * H * W * C, pairs = (long)N * H * W * dg * 9;
  unsigned* stat = reinterpret_cast<unsigned*>(workspace + nx);
  const int zrc = danhip_zero_async(stat, sizeof(unsigned) * (64 + (size_t)N * H * W * dg), s);
  if (zrc) return zrc;
  hipLaunchKernelGGL(deform_far_stat_kernel, dim3(dh_grid_for(pairs, 256, 1024)), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(offsets), pairs, stat);
  return danhip_launch_deform_far_ordered(offsets, dS, workspace, stat, stat + 64, N, H, W, C, dg, window, always, s);
}

/* Deterministic mode: 3 x 3, stride 1, dilation 1 (SAME padding of 1), C / deformable_group == 64 alone.  The tile kernels as in default mode,
 * never the scatter form; the far corners through deform_far.hip instead of float atomics. */
static int deform_sample_bwd_ordered(const uint16_t* x, const uint16_t* offsets, const uint16_t* dS, uint16_t* dx, uint16_t* d_offsets, int32_t N,
                                     int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride, int32_t dilation, int32_t dg,
                                     int accumulate, int relu_x, float* workspace, size_t workspace_bytes, void* stream) {
  DH_REQUIRE(x && offsets && dS && dx && d_offsets && workspace, DANHIP_EINVAL, "deform_sample_bwd: null pointer");
  DeformGeom g;
  int rc = make_geom(&g, N, H, W, C, kh, kw, stride, dilation, dg, "deform_sample_bwd");
  if (rc) return rc;
  const char* why = danhip_deform_far_shape_error(N, H, W, C, dg);
  const int tiles_h = (H + DT_H - 1) / DT_H, tiles_w = (W + DT_W - 1) / DT_W;
  const long tile_blocks = (long)N * tiles_h * tiles_w * dg;
  if (!why && !(kh == 3 && kw == 3 && stride == 1 && dilation == 1 && g.pad_t == 1 && g.pad_l == 1)) why = "3 x 3 taps, stride 1, dilation 1 only";
  if (!why && !(dg <= 9 && tile_blocks < (1l << 31) - 8)) why = "deformable_group <= 9 and fewer than 2^31 tiles";
  DH_REQUIRE(!why, DANHIP_EINVAL, "deform_sample_bwd: this shape class has no ordered form (option \"deterministic\" is set): %s", why);
  const int force = danhip_option("deform_bwd_form");
  DH_REQUIRE(force != 2, DANHIP_EINVAL, "deform_sample_bwd: the scatter form (option \"deform_bwd_form\" = 2) has no ordered form (option \"deterministic\" is set)");
  DH_REQUIRE(!danhip_option("deform_dx_untiled"), DANHIP_EINVAL, "deform_sample_bwd: option \"deform_dx_untiled\" has no ordered form (option \"deterministic\" is set)");
  const size_t need = danhip_deform_sample_bwd_ordered_workspace_bytes(N, H, W, C, dg);
  DH_REQUIRE(workspace_bytes >= need, DANHIP_EWORKSPACE, "deform_sample_bwd: workspace of %zu bytes, deterministic mode needs %zu (danhip_deform_sample_bwd_ordered_workspace_bytes)",
             workspace_bytes, need);
  hipStream_t s = (hipStream_t)stream;
  const long nx = (long)N * H * W * C, pairs = (long)N * H * W * dg * 9;
  const unsigned* stat = reinterpret_cast<const unsigned*>(workspace + nx);
  rc = deform_far_ordered_run(offsets, dS, N, H, W, C, dg, force == 3 ? 1 : (force == 1 ? 2 : 0), 0, workspace, s);
  if (rc) return rc;
  const BwdGate gate{stat, 0xffffffffu, (unsigned)(pairs / 128), force};         // (never the scatter form; the window as in default mode)
  const unsigned tgrid = (unsigned)((tile_blocks + 7) / 8 * 8);
  hipLaunchKernelGGL(deform_bwd_doff_tile_c64_kernel, dim3(tgrid), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(x), reinterpret_cast<const bf16_t*>(offsets),
                     reinterpret_cast<const bf16_t*>(dS), (float*)nullptr, reinterpret_cast<bf16_t*>(d_offsets), g, gate, tiles_h, tiles_w);
  hipLaunchKernelGGL(deform_bwd_dx_tile_c64_kernel, dim3(tgrid), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(offsets), reinterpret_cast<const bf16_t*>(dS),
                     workspace, reinterpret_cast<bf16_t*>(dx), g, accumulate, gate, relu_x ? reinterpret_cast<const bf16_t*>(x) : nullptr, tiles_h, tiles_w);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

/* Test and measurement hook: the ordered far path alone.  workspace as danhip_deform_sample_bwd takes it in deterministic mode; on return (stream
 * order) its first N*H*W*C floats are far_dx - zeros where no far corner lands, also when the statistic reports none at all.  window: 0 by the
 * statistic, 1 / 2 fixed. */
extern "C" int danhip_deform_far_ordered(const uint16_t* offsets, const uint16_t* dS, int32_t N, int32_t H, int32_t W, int32_t C, int32_t deformable_group,
                                         int32_t window, float* workspace, size_t workspace_bytes, void* stream) {
  DH_REQUIRE(offsets && dS && workspace, DANHIP_EINVAL, "deform_far_ordered: null pointer");
  const char* why = danhip_deform_far_shape_error(N, H, W, C, deformable_group);
  DH_REQUIRE(!why, DANHIP_EINVAL, "deform_far_ordered: this shape class has no ordered form: %s", why);
  DH_REQUIRE(window >= 0 && window <= 2, DANHIP_EINVAL, "deform_far_ordered: window %d (0 by the statistic, 1, 2)", window);
  const size_t need = danhip_deform_sample_bwd_ordered_workspace_bytes(N, H, W, C, deformable_group);
  DH_REQUIRE(workspace_bytes >= need, DANHIP_EWORKSPACE, "deform_far_ordered: workspace of %zu bytes, needs %zu", workspace_bytes, need);
  return deform_far_ordered_run(offsets, dS, N, H, W, C, deformable_group, window, 1, workspace, (hipStream_t)stream);
}

/* dS [N*Ho*Wo, kh*kw*C] -> d_offsets bf16 [N,Ho,Wo,dg*2*kh*kw] (overwritten) and dx bf16 [N,H,W,C] (=|+= if accumulate).
 * workspace: N*H*W*C + 64 floats (fp32 scatter target + the far-corner statistic), zeroed inside. */
static int deform_sample_bwd_impl(const uint16_t* x, const uint16_t* offsets, const uint16_t* dS, uint16_t* dx, uint16_t* d_offsets,
                                  int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride, int32_t dilation,
                                  int32_t deformable_group, int accumulate, int relu_x, float* workspace, size_t workspace_bytes, void* stream) {
  if (danhip_option("deterministic") != 0)
    return deform_sample_bwd_ordered(x, offsets, dS, dx, d_offsets, N, H, W, C, kh, kw, stride, dilation, deformable_group, accumulate, relu_x, workspace,
                                     workspace_bytes, stream);
  const bf16_t* rx = relu_x ? x : nullptr;              // dx *= (x > 0): x is a ReLU output whose producer takes dx as delivered
  DH_REQUIRE(x && offsets && dS && dx && d_offsets && workspace, DANHIP_EINVAL, "deform_sample_bwd: null pointer");
  DH_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && workspace_bytes >= danhip_deform_sample_bwd_workspace_bytes(N, H, W, C), DANHIP_EWORKSPACE,
             "deform_sample_bwd: workspace of %zu bytes, needs %zu (N*H*W*C + 64 floats)", workspace_bytes,
             danhip_deform_sample_bwd_workspace_bytes(N, H, W, C));
  DeformGeom g;
  int rc = make_geom(&g, N, H, W, C, kh, kw, stride, dilation, deformable_group, "deform_sample_bwd");
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const long nx = (long)N * H * W * C;
  unsigned* stat = reinterpret_cast<unsigned*>(workspace + nx);
  const bool gathered = C / deformable_group == 64 && stride == 1 && kh == 3 && kw == 3 && (long)N * g.Ho * g.Wo * 9 < (1l << 31) && deformable_group <= 9;
  // fp32 scatter target + 64 words of statistics behind it: zeroed together — or, for the gather forms, the statistics now and the
  // target by zero_if_far_kernel once they say it will be used at all
  const int tiles_h = (H + DT_H - 1) / DT_H, tiles_w = (W + DT_W - 1) / DT_W;
  const long tile_blocks = (long)N * tiles_h * tiles_w * deformable_group;
  // both gather windows as the tile kernels (dilation 1); other dilations keep the item / wave-per-pixel kernels (which read the side buffer always)
  const bool tiled = gathered && dilation == 1 && g.pad_t == 1 && g.pad_l == 1 && tile_blocks < (1l << 31) - 8 && !danhip_option("deform_dx_untiled");
  const bool lazy_zero = tiled && (nx * 4) % 16 == 0;
  { const int zrc = lazy_zero ? danhip_zero_async(stat, sizeof(unsigned) * 64, s) : danhip_zero_async(workspace, sizeof(float) * (nx + 64), s); if (zrc) return zrc; }
  if (gathered) {
    const long nd = (long)N * g.Ho * g.Wo * deformable_group, ng = (long)N * H * W * deformable_group;
    const long pairs = (long)N * g.Ho * g.Wo * deformable_group * 9;
    // A corner lies floor(o) or floor(o) + 1 from the tap's nominal position, so it is outside the +-R window iff o is outside [-R, R).
    // Scatter form beyond 15 % of the taps outside [-2, 2) (160 x 160 x 256, batch 16, offsets N(0, s): s = 0.5 / 1.0 px -> 0 % / 9 % ->
    // 3.4 / 7.7 ms in the +-2 gather form; s = 2.0 -> 53 % -> 43 ms; the scatter form: 12.0 ms whatever the offsets); the +-1 window
    // (81 candidates per input pixel and group instead of 225) while fewer than 1 / 128 of the taps lie outside [-1, 1).
    BwdGate gate{stat, (unsigned)(pairs / 20 * 3), (unsigned)(pairs / 128), danhip_option("deform_bwd_form")};
    hipLaunchKernelGGL(deform_far_stat_kernel, dim3(dh_grid_for(pairs, 256, 1024)), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(offsets), pairs, stat);
    if (lazy_zero)
      hipLaunchKernelGGL(zero_if_far_kernel, dim3(dh_grid_for(nx / 4, 256, 2048)), dim3(256), 0, s, reinterpret_cast<uint4*>(workspace), nx / 4, stat, gate.force);
    if (tiled) {
      const unsigned tgrid = (unsigned)((tile_blocks + 7) / 8 * 8);       // 8 XCDs x their share of the items (the kernels map blockIdx -> item)
      hipLaunchKernelGGL(deform_bwd_doff_tile_c64_kernel, dim3(tgrid), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(x),
                         reinterpret_cast<const bf16_t*>(offsets), reinterpret_cast<const bf16_t*>(dS), workspace, reinterpret_cast<bf16_t*>(d_offsets), g, gate,
                         tiles_h, tiles_w);
      hipLaunchKernelGGL(deform_bwd_dx_tile_c64_kernel, dim3(tgrid), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(offsets),
                         reinterpret_cast<const bf16_t*>(dS), workspace, reinterpret_cast<bf16_t*>(dx), g, accumulate, gate, rx, tiles_h, tiles_w);
    } else {
      const dim3 gd(dh_grid_for((nd + 31) / 32 * 256, 256, 65536)), gg(dh_grid_for((ng + 3) / 4 * 256, 256, 65536));
      hipLaunchKernelGGL(deform_bwd_doff9_c64_kernel, gd, dim3(256), 0, s, x, offsets, dS, workspace, d_offsets, g, gate);
      hipLaunchKernelGGL(deform_bwd_dx_gather9_c64_kernel, gg, dim3(256), 0, s, offsets, dS, workspace, dx, g, accumulate, gate, rx);
    }
    // the scatter form's two kernels on small grids (grid-stride loops): empty ~10 us each when a gather form runs
    const long nwork = (long)N * g.Ho * g.Wo * kh * kw * deformable_group;
    hipLaunchKernelGGL(deform_sample_bwd_c64_kernel, dim3(dh_grid_for((nwork + 3) / 4 * 256, 256, 2048)), dim3(256), 0, s, x, offsets, dS, workspace, d_offsets, g,
                       gate);
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(dh_grid_for(nx / 8, 256, 2048)), dim3(256), 0, s, workspace, dx, nx / 8, accumulate, gate, rx);
    DH_LAUNCH_CHECK();
    return DANHIP_OK;
  }
  const BwdGate none{nullptr, 0u, 0u, 0};
  if (C / deformable_group == 64) {
    const long nwork = (long)N * g.Ho * g.Wo * kh * kw * deformable_group;
    hipLaunchKernelGGL(deform_sample_bwd_c64_kernel, dim3(dh_grid_for((nwork + 3) / 4 * 256, 256, 65536)), dim3(256), 0, s, x, offsets, dS, workspace, d_offsets, g,
                       none);
  } else {
    const long total = (long)N * g.Ho * g.Wo * kh * kw * (C / 8);
    hipLaunchKernelGGL(deform_sample_bwd_kernel, dim3(dh_grid_for(total, 256, 16384)), dim3(256), 0, s, x, offsets, dS, workspace, d_offsets, g);
  }
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(f32_to_bf16_kernel, dim3(dh_grid_for(nx / 8, 256, 16384)), dim3(256), 0, s, workspace, dx, nx / 8, accumulate, none, rx);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_deform_sample_bwd(const uint16_t* x, const uint16_t* offsets, const uint16_t* dS, uint16_t* dx, uint16_t* d_offsets,
                                        int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride, int32_t dilation,
                                        int32_t deformable_group, int accumulate, float* workspace, size_t workspace_bytes, void* stream) {
  return deform_sample_bwd_impl(x, offsets, dS, dx, d_offsets, N, H, W, C, kh, kw, stride, dilation, deformable_group, accumulate, 0, workspace,
                                workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------------------------
// DeformConvOp / DeformConvBackpropOp as single entry points (cpp/Deform/deform_conv.cc:392-535, :635-771): the same
// orchestration as the reference's Compute() — im2col, GEMM; and for the backward GEMM^T, col2im_coord, col2im,
// re-im2col, filter GEMM — with the im2col buffer living in the caller's workspace only for the duration of the call
// (the reference allocates it with allocate_temp per call, :497-503) and all samples processed in one batch.
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

extern "C" size_t danhip_deform_conv_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t kh, int32_t kw, int32_t stride,
                                                     int backward) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || kh <= 0 || kw <= 0 || stride <= 0) return 0;
  const size_t Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
  const size_t col = align256((size_t)N * Ho * Wo * kh * kw * C * sizeof(uint16_t));
  return backward ? 2 * col + align256(((size_t)N * H * W * C + 64) * sizeof(float)) : col;
}

static int deform_gemm_desc(danhip_conv_desc* d, int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride) {
  d->N = N; d->Ho = (H + stride - 1) / stride; d->Wo = (W + stride - 1) / stride;
  d->H = d->Ho; d->W = d->Wo; d->Cin = kh * kw * C; d->Cout = Cout; d->kh = 1; d->kw = 1; d->stride = 1;
  return 0;
}

/* Deterministic mode's workspace of danhip_deform_conv_bwd*: answered with the option SET (the weight-gradient part is the active mode's).
 * 0: the shape class has no ordered form. */
extern "C" size_t danhip_deform_conv_bwd_ordered_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw,
                                                                 int32_t stride, int32_t deformable_group) {
  if (Cout <= 0 || kh != 3 || kw != 3 || stride != 1) return 0;
  const size_t sample = danhip_deform_sample_bwd_ordered_workspace_bytes(N, H, W, C, deformable_group);
  if (!sample) return 0;
  danhip_conv_desc d;
  deform_gemm_desc(&d, N, H, W, C, Cout, kh, kw, stride);
  return 2 * danhip_deform_conv_workspace_bytes(N, H, W, C, kh, kw, stride, 0) + align256(sample) + align256(danhip_conv2d_bwd_weight_workspace_bytes(&d));
}

bool danhip_deform_fused_eligible(int N, int H, int W, int C, int Cout, int kh, int kw, int stride, int dg);
int danhip_launch_deform_fused_fwd(const uint16_t* x, const uint16_t* wf_packed, int kpad, const float* bias, const uint16_t* offsets, uint16_t* y,
                                   uint16_t* col, int N, int H, int W, int C, int Cout, int stride, int dil, int dg, int relu, hipStream_t s);

extern "C" int danhip_deform_conv_fused(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                                        int32_t deformable_group) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || Cout <= 0 || stride <= 0 || deformable_group <= 0) return 0;
  return danhip_deform_fused_eligible(N, H, W, C, Cout, kh, kw, stride, deformable_group) ? 1 : 0;
}

extern "C" int danhip_deform_conv_fwd(const uint16_t* x, const uint16_t* wf_packed, const float* bias, const uint16_t* offsets, uint16_t* y,
                                      int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                                      int32_t dilation, int32_t deformable_group, int relu, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  DH_REQUIRE(x && wf_packed && offsets && y, DANHIP_EINVAL, "deform_conv_fwd: null pointer");
  if (danhip_deform_conv_fused(N, H, W, C, Cout, kh, kw, stride, deformable_group)) {
    // one kernel: sampling feeds the GEMM through LDS; the column buffer is written only if the caller hands a workspace for it
    DeformGeom g;
    int rc = make_geom(&g, N, H, W, C, kh, kw, stride, dilation, deformable_group, "deform_conv_fwd");
    if (rc) return rc;
    DH_REQUIRE(!workspace || workspace_bytes >= danhip_deform_conv_workspace_bytes(N, H, W, C, kh, kw, stride, 0), DANHIP_EWORKSPACE,
               "deform_conv_fwd: workspace too small for the column buffer");
    const int kpad = (kh * kw * C + 63) / 64 * 64;
    return danhip_launch_deform_fused_fwd(x, wf_packed, kpad, bias, offsets, y, (uint16_t*)workspace, N, H, W, C, Cout, stride, dilation,
                                          deformable_group, relu, (hipStream_t)stream);
  }
  DH_REQUIRE(workspace, DANHIP_EINVAL, "deform_conv_fwd: this shape needs the column-buffer workspace");
  DH_REQUIRE(workspace_bytes >= danhip_deform_conv_workspace_bytes(N, H, W, C, kh, kw, stride, 0) && workspace_bytes > 0, DANHIP_EWORKSPACE,
             "deform_conv_fwd: workspace too small");
  uint16_t* col = (uint16_t*)workspace;
  int rc = danhip_deform_sample_fwd(x, offsets, col, N, H, W, C, kh, kw, stride, dilation, deformable_group, stream);
  if (rc) return rc;
  danhip_conv_desc d;
  deform_gemm_desc(&d, N, H, W, C, Cout, kh, kw, stride);
  return danhip_conv2d_fwd(&d, col, wf_packed, bias, y, DANHIP_BF16, relu, nullptr, stream);
}

// `col_saved`: the im2col buffer danhip_deform_conv_fwd left in ITS workspace (same x / offsets), kept alive by the caller — the backward
// then skips the reference's re-im2col (:744-748; 1.9 GB rewritten per call at 160x160x256, batch 16).  NULL: re-sample as the reference.
static int deform_conv_bwd_impl(const uint16_t* x, const uint16_t* wb_packed, const uint16_t* offsets, const uint16_t* dy,
                                const uint16_t* col_saved, uint16_t* dx, uint16_t* d_offsets, float* dw, float* db, int32_t N,
                                int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                                int32_t dilation, int32_t deformable_group, int accumulate_dx, int relu_x, void* workspace,
                                size_t workspace_bytes, void* stream) {
  DH_REQUIRE(x && wb_packed && offsets && dy && dx && d_offsets && dw && workspace, DANHIP_EINVAL, "deform_conv_bwd: null pointer");
  const bool det = danhip_option("deterministic") != 0;
  danhip_conv_desc d;
  deform_gemm_desc(&d, N, H, W, C, Cout, kh, kw, stride);
  const size_t colb = danhip_deform_conv_workspace_bytes(N, H, W, C, kh, kw, stride, 0);
  size_t need = danhip_deform_conv_workspace_bytes(N, H, W, C, kh, kw, stride, 1), sample_ws = 0, wgrad_ws = 0;
  if (det) {        // [col | dcol | side buffer + statistic + ordered region | weight-gradient partial rows]
    need = danhip_deform_conv_bwd_ordered_workspace_bytes(N, H, W, C, Cout, kh, kw, stride, deformable_group);
    DH_REQUIRE(need > 0, DANHIP_EINVAL, "deform_conv_bwd: this shape class has no ordered form (option \"deterministic\" is set): 3 x 3 taps, stride 1, dilation 1, C / deformable_group == 64 only");
    sample_ws = align256(danhip_deform_sample_bwd_ordered_workspace_bytes(N, H, W, C, deformable_group));
    wgrad_ws = danhip_conv2d_bwd_weight_workspace_bytes(&d);
  }
  DH_REQUIRE(workspace_bytes >= need && need > 0, DANHIP_EWORKSPACE, "deform_conv_bwd: workspace of %zu bytes, needs %zu%s", workspace_bytes, need,
             det ? " (deterministic mode: danhip_deform_conv_bwd_ordered_workspace_bytes)" : "");
  uint16_t* col = (uint16_t*)workspace;
  uint16_t* dcol = (uint16_t*)((char*)workspace + colb);
  float* scatter = (float*)((char*)workspace + 2 * colb);
  int rc = danhip_conv2d_bwd_data(&d, dy, wb_packed, nullptr, dcol, 0, stream);                       // col gradient = W^T dOut (:700-712)
  if (rc) return rc;
  rc = deform_sample_bwd_impl(x, offsets, dcol, dx, d_offsets, N, H, W, C, kh, kw, stride, dilation, deformable_group, accumulate_dx, relu_x, scatter,
                              det ? sample_ws : workspace_bytes - 2 * colb, stream);                                              // col2im_coord + col2im (:716-741)
  if (rc) return rc;
  if (!col_saved) {
    rc = danhip_deform_sample_fwd(x, offsets, col, N, H, W, C, kh, kw, stride, dilation, deformable_group, stream);   // re-im2col (:744-748)
    if (rc) return rc;
  }
  if (det) return danhip_conv2d_bwd_weight_ws(&d, col_saved ? col_saved : col, dy, dw, db, kh * kw * C, (char*)workspace + 2 * colb + sample_ws, wgrad_ws, stream);
  return danhip_conv2d_bwd_weight(&d, col_saved ? col_saved : col, dy, dw, db, kh * kw * C, stream);  // dW += dOut col^T (:750-768)
}

extern "C" int danhip_deform_conv_bwd_with_col(const uint16_t* x, const uint16_t* wb_packed, const uint16_t* offsets, const uint16_t* dy,
                                               const uint16_t* col_saved, uint16_t* dx, uint16_t* d_offsets, float* dw, float* db, int32_t N,
                                               int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                                               int32_t dilation, int32_t deformable_group, int accumulate_dx, void* workspace,
                                               size_t workspace_bytes, void* stream) {
  return deform_conv_bwd_impl(x, wb_packed, offsets, dy, col_saved, dx, d_offsets, dw, db, N, H, W, C, Cout, kh, kw, stride, dilation, deformable_group,
                              accumulate_dx, 0, workspace, workspace_bytes, stream);
}

// The same with the input gradient DELIVERED the way the convolutions hand theirs over (dan_amd.ops.GradSlot): relu_x != 0 multiplies it by
// (x > 0) - x is then a ReLU output and its producer takes the gradient as final - before accumulate_dx adds what dx already holds.
extern "C" int danhip_deform_conv_bwd_deliver(const uint16_t* x, const uint16_t* wb_packed, const uint16_t* offsets, const uint16_t* dy,
                                              const uint16_t* col_saved, uint16_t* dx, uint16_t* d_offsets, float* dw, float* db, int32_t N,
                                              int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t kh, int32_t kw, int32_t stride,
                                              int32_t dilation, int32_t deformable_group, int accumulate_dx, int relu_x, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  return deform_conv_bwd_impl(x, wb_packed, offsets, dy, col_saved, dx, d_offsets, dw, db, N, H, W, C, Cout, kh, kw, stride, dilation, deformable_group,
                              accumulate_dx, relu_x, workspace, workspace_bytes, stream);
}

extern "C" int danhip_deform_conv_bwd(const uint16_t* x, const uint16_t* wb_packed, const uint16_t* offsets, const uint16_t* dy, uint16_t* dx,
                                      uint16_t* d_offsets, float* dw, float* db, int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cout,
                                      int32_t kh, int32_t kw, int32_t stride, int32_t dilation, int32_t deformable_group, int accumulate_dx,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return danhip_deform_conv_bwd_with_col(x, wb_packed, offsets, dy, nullptr, dx, d_offsets, dw, db, N, H, W, C, Cout, kh, kw, stride, dilation,
                                         deformable_group, accumulate_dx, workspace, workspace_bytes, stream);
}
