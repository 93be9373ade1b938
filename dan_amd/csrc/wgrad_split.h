// How the streaming weight-gradient kernels (conv_wgrad_rows.hip: 3x3, conv_wgrad_pw.hip: 1x1) split their reduction over the chip.
// The reduction (rows of a strip / 32-pixel K-steps: "units") is cut into `splits` equal shares; a workgroup owns one share of one
// (ci tile, co tile) pair.  Its partial tile is added into dW with fp32 atomics, or - the slab form - stored as it lies in the registers
// into a scratch slab that a second kernel sums in a fixed order.  Deterministic mode always takes the slab and also writes the bias
// gradient as rows [splits][db_pitch] behind the tiles, summed by dh_ordered_reduce.  Both kernels' argument blocks carry the fields
// ci_tiles, co_tiles, xcd_grouped, div_pairs, splits, slab, db_slab and db_pitch, which this header fills and reads.
#pragma once
#include "conv_common.h"

struct WgSplitPlan {
  int pairs, splits, per_split;      // (ci, co) tile pairs; shares of the reduction; units per share
  bool slab;              // the slab form (partial tiles as plain stores + a combine pass) is worth taking ...
  size_t slab_bytes;      // ... and needs this much scratch (one register tile per workgroup, at most one workgroup per CU)
  bool det;               // deterministic mode: always the slab form (any number of splits), the bias-gradient rows behind the tiles
  size_t db_off;          // byte offset of the [splits][db_pitch] bias-gradient rows in the scratch
  int db_pitch;
};
// units: length of the reduction; tile_slots: float4 slots of one workgroup's register tile
static inline WgSplitPlan wg_split_plan(int units, int ci_tiles, int co_tiles, int tile_slots, int Cout) {
  WgSplitPlan p{};
  p.pairs = ci_tiles * co_tiles;
  int splits = dh_cu_count() / p.pairs;
  if (splits < 1) splits = 1;
  if (splits > units) splits = units;
  p.per_split = (units + splits - 1) / splits;
  p.splits = (units + p.per_split - 1) / p.per_split;
  // The slab form pays when the launch is short (every block reaches its epilogue together and nothing hides the tail: 2-4 images per
  // GPU, the 40x40 / 20x20 levels); on long launches the blocks drift apart, the atomic tail hides under other blocks' MFMAs and the
  // extra pass costs more than it saves (batch 16: conv3_2 0.426 against 0.428 ms, conv2_2 0.479 against 0.455; profiles/r3).
  p.slab = p.splits >= 2 && (danhip_option("wgrad_slab") == 2 || p.per_split <= 192);
  p.slab_bytes = (size_t)dh_cu_count() * tile_slots * 16;
  p.det = danhip_option("deterministic") != 0;
  if (p.det) {            // every launch through the slab (the combine pass's order is fixed by `splits`), db as rows for the ordered reduction
    p.slab = true;
    p.db_pitch = (Cout + 3) / 4 * 4;
    p.db_off = (size_t)p.pairs * p.splits * tile_slots * 16;
    p.slab_bytes = p.db_off + (size_t)p.splits * p.db_pitch * sizeof(float);
  }
  return p;
}

// ---- workgroup <-> (split, pair).  Plain: block = split * pairs + pair.  XCD-grouped (splits % 8 == 0, more than one pair): blocks are
// dealt round-robin to the 8 XCDs, so block = ((split / 8) * pairs + pair) * 8 + split % 8 puts the pairs of one split - they read the
// same rows - behind one L2.  The kernels use the first function, the combine passes its inverse.
static inline int wg_xcd_grouped(const WgSplitPlan& p) { return (p.splits % 8 == 0 && p.pairs > 1) ? 1 : 0; }
template <class Args>
__device__ __forceinline__ void wg_block_to_split_pair(const Args& a, int pairs, int& split, int& pair) {
  if (a.xcd_grouped) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int sq = (int)fdiv((unsigned)slot, a.div_pairs);
    pair = slot - sq * pairs;
    split = sq * 8 + xcd;
  } else {
    split = (int)fdiv(blockIdx.x, a.div_pairs);
    pair = (int)blockIdx.x - split * pairs;
  }
}
template <class Args>
__device__ __forceinline__ size_t wg_split_pair_to_block(const Args& a, int pairs, int split, int pair) {
  return a.xcd_grouped ? (size_t)(((split >> 3) * pairs + pair) * 8 + (split & 7)) : (size_t)(split * pairs + pair);
}

// ---- the combine pass's summation, for a 256-thread workgroup that owns 64 consecutive float4 slots of pair `pair`
// (q: this lane's slot in the tile; pairs, lane = threadIdx.x & 63 and w = threadIdx.x >> 6 from the caller): wave w sums the splits
// w, w + 4, ... (eight independent 16-byte loads in flight per lane), the four partial sums meet in LDS.  True in wave 0, which holds the
// total in `sum`; the other waves are done.  The order of the additions is part of the contract (deterministic mode, bit-identity tests):
// do not regroup them.  (The caller-computed arguments and `sp` declared before the accumulators also keep both combine kernels' code
// objects byte-identical to the form that had this loop written out in each kernel.)
template <int TILE, class Args>
__device__ __forceinline__ bool wg_sum_splits(const Args& a, int pairs, int pair, int q, int lane, int w, f32x4 (&part)[4][64], f32x4& sum) {
  const f32x4* src = reinterpret_cast<const f32x4*>(a.slab) + q;
  int sp = w;
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s0 = s1;
  for (; sp + 28 < a.splits; sp += 32) {              // eight splits of this wave per round
    f32x4 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = __builtin_nontemporal_load(src + wg_split_pair_to_block(a, pairs, sp + 4 * e, pair) * TILE);
    s0 += (v[0] + v[1]) + (v[2] + v[3]);
    s1 += (v[4] + v[5]) + (v[6] + v[7]);
  }
  for (; sp < a.splits; sp += 4) s0 += __builtin_nontemporal_load(src + wg_split_pair_to_block(a, pairs, sp, pair) * TILE);
  part[w][lane] = s0 + s1;
  __syncthreads();
  if (w != 0) return false;
  sum = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
  return true;
}

// ---- host: the plan into the argument block, the kernel, the combine pass, the ordered bias-gradient sum.  The slab is taken when the
// plan wants it, the caller's workspace holds it, and deterministic mode or option "wgrad_slab" allows it (0: always fp32 atomics).
template <class Args>
int wg_split_launch(Args& a, const WgSplitPlan& p, const WgradCall& c, void (*kernel)(Args), int lds, void (*reduce)(Args), int tile_slots,
                    hipStream_t s) {
  a.div_pairs = make_fastdiv(p.pairs);
  a.xcd_grouped = wg_xcd_grouped(p);
  a.splits = p.splits;
  a.b2 = danhip_option("wgrad_b2");
  a.slab = ((p.det || danhip_option("wgrad_slab")) && c.ws && p.slab && c.ws_bytes >= p.slab_bytes) ? reinterpret_cast<float*>(c.ws) : nullptr;
  DH_REQUIRE(!p.det || a.slab, DANHIP_EINVAL, "conv2d_bwd_weight: deterministic mode needs a workspace of danhip_conv2d_bwd_weight_workspace_bytes(d) bytes (call danhip_conv2d_bwd_weight_ws)");
  if (p.det && c.db) { a.db_slab = reinterpret_cast<float*>(reinterpret_cast<char*>(c.ws) + p.db_off); a.db_pitch = p.db_pitch; }
  hipLaunchKernelGGL(kernel, dim3(p.pairs * p.splits), dim3(512), lds, s, a);
  DH_LAUNCH_CHECK();
  if (a.slab) {
    hipLaunchKernelGGL(reduce, dim3(p.pairs * (tile_slots / 64)), dim3(256), 0, s, a);
    DH_LAUNCH_CHECK();
  }
  if (a.db_slab) return dh_ordered_reduce(a.db_slab, a.db_pitch, p.splits, c.d->Cout, c.db, 1, s);
  return DANHIP_OK;
}
