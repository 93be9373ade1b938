// Far corners of the deformable backward, ordered form (include/danhip.h, "Deformable backward in deterministic mode"): get_gradient_weight
// with the col2im guards (corner_set, the rule every dX form shares) and the per-record routines - far test, destination, key, weight, term -
// as host + device functions.  The kernels of deform_far.hip run them over device memory, danhip_deform_far_ordered_emulate
// (deform_far_emulate.cpp) over checked host arrays: one body of code decides on both sides what a far record is and what it adds.
// Nothing here needs the HIP headers: a host compiler takes this file as it is.
//
// Shape class: 3 x 3 taps, stride 1, dilation 1, SAME padding of 1, C / deformable_group == 64 (Ho = H, Wo = W).
//   source   s = (m * dg + grp) * 9 + t       m = (n * H + ho) * W + wo; word s of the offsets tensor holds the tap's (dh, dw) pair
//   record   one corner k (0..3) of a source that corner_set accepts and that lies more than R pixels from the tap's nominal position
//   key      (m * 9 + t) * 4 + k              the row of dS the record reads, and the corner: unique inside a destination
//   dest     ((n * H + h) * W + w) * dg + grp the 64 fp32 sums of far_dx the record adds to
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DH_FAR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DH_FAR_HD inline
#endif
#if defined(__clang__)
#define DH_FAR_UNROLL _Pragma("unroll")
#else
#define DH_FAR_UNROLL
#endif

// ---- dX: get_gradient_weight (:130-173) + the guards of deformable_col2im_gpu_kernel (:311-326) for one sampling position
struct CornerSet {
  int rh[4], rw[4];
  float wg[4];
  bool ok[4];
};
DH_FAR_HD CornerSet corner_set(float inv_h, float inv_w, int H, int W) {
  CornerSet cs;
  const bool in = !(inv_h < 0 || inv_h > (float)H || inv_w < 0 || inv_w > (float)W);
  float ah = fmaxf(inv_h, 0.f), aw = fmaxf(inv_w, 0.f);
  if (!in) { ah = 0.f; aw = 0.f; }
  int hl = (int)ah, wl = (int)aw, hh, wh;
  const bool ch = hl >= H - 1, cw = wl >= W - 1;
  if (ch) { hh = hl = H - 1; ah = (float)hl; } else hh = hl + 1;
  if (cw) { wh = wl = W - 1; aw = (float)wl; } else wh = wl + 1;
  cs.rh[0] = hl; cs.rh[1] = hl; cs.rh[2] = hh; cs.rh[3] = hh;
  cs.rw[0] = wl; cs.rw[1] = wh; cs.rw[2] = wl; cs.rw[3] = wh;
  cs.wg[0] = ((float)(hl + 1) - ah) * ((float)(wl + 1) - aw);
  cs.wg[1] = ((float)(hl + 1) - ah) * (aw + 1.f - (float)wh);
  cs.wg[2] = (ah + 1.f - (float)hh) * ((float)(wl + 1) - aw);
  cs.wg[3] = (ah + 1.f - (float)hh) * (aw + 1.f - (float)wh);
  const bool dup[4] = {false, cw, ch, ch || cw};
  DH_FAR_UNROLL
  for (int k = 0; k < 4; ++k)
    cs.ok[k] = in && !dup[k] && fabsf(inv_h - (float)cs.rh[k]) < 1.f && fabsf(inv_w - (float)cs.rw[k]) < 1.f && cs.rh[k] >= 0 && cs.rh[k] < H &&
               cs.rw[k] >= 0 && cs.rw[k] < W;
  return cs;
}

struct DhFarGeom {
  int32_t N, H, W, C, dg;
};

// One 16-bit value of the build's activation type (bf16, or IEEE fp16 with -DDANHIP_FP16) as fp32
DH_FAR_HD float dh_far_act2f(uint16_t v) {
#ifdef DANHIP_FP16
  _Float16 h;
  __builtin_memcpy(&h, &v, 2);
  return (float)h;
#else
  const uint32_t u = (uint32_t)v << 16;
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
#endif
}

// The statistic the window follows: an offset pair with a component outside [-r, r) (a NaN counts as outside, as in deform_far_stat_kernel)
DH_FAR_HD bool dh_far_stat_outside(float oh, float ow, float r) { return !(oh >= -r && oh < r) || !(ow >= -r && ow < r); }
// Gather window R of the mode: +-1 while at most thresh1 = pairs / 128 offset pairs leave [-1, 1), else +-2.  Never the scatter form.
DH_FAR_HD uint32_t dh_far_thresh1(uint64_t pairs) { return (uint32_t)(pairs / 128); }
DH_FAR_HD int dh_far_window(int forced, uint32_t stat1, uint32_t thresh1) { return forced ? forced : (stat1 <= thresh1 ? 1 : 2); }
// The gather kernels' own test for "this tap may have a far corner": a corner lies floor(o) or floor(o) + 1 from the nominal position
DH_FAR_HD bool dh_far_offset_outside(float oh, float ow, int R) {
  const float lim = (float)R;
  return oh < -lim || oh >= lim || ow < -lim || ow >= lim;
}

DH_FAR_HD int dh_far_iabs(int v) { return v < 0 ? -v : v; }

// Far corners of tap t of output pixel (ho, wo) under the offset pair (oh, ow): bit k of the result = corner k is a record.  cs = the corners.
DH_FAR_HD unsigned dh_far_mask(const DhFarGeom& g, int ho, int wo, int t, float oh, float ow, int R, CornerSet& cs) {
  const int nh = ho - 1 + t / 3, nw = wo - 1 + t % 3;
  cs = corner_set((float)nh + oh, (float)nw + ow, g.H, g.W);
  unsigned mask = 0;
  DH_FAR_UNROLL
  for (int k = 0; k < 4; ++k)
    if (cs.ok[k] && (dh_far_iabs(cs.rh[k] - nh) > R || dh_far_iabs(cs.rw[k] - nw) > R)) mask |= 1u << k;
  return mask;
}
DH_FAR_HD uint32_t dh_far_key(uint32_t m, int t, int k) { return (m * 9u + (uint32_t)t) * 4u + (uint32_t)k; }
DH_FAR_HD uint32_t dh_far_dest(const DhFarGeom& g, int n, int h, int w, int grp) {
  return (((uint32_t)n * (uint32_t)g.H + (uint32_t)h) * (uint32_t)g.W + (uint32_t)w) * (uint32_t)g.dg + (uint32_t)grp;
}
// One term of the order contract: F <- F + w * dS as ONE fused multiply-add, on both sides
DH_FAR_HD float dh_far_term(float acc, float w, float ds) { return fmaf(w, ds, acc); }

// Sizes, from the shape alone.  sources < 2^30 keeps every key, record position and the record total below 2^32.
DH_FAR_HD uint64_t dh_far_sources(const DhFarGeom& g) { return (uint64_t)g.N * (uint64_t)g.H * (uint64_t)g.W * (uint64_t)g.dg * 9u; }
DH_FAR_HD uint64_t dh_far_dests(const DhFarGeom& g) { return (uint64_t)g.N * (uint64_t)g.H * (uint64_t)g.W * (uint64_t)g.dg; }
#define DH_FAR_SCAN_BLOCK 2048u   /* destinations per workgroup of the prefix sum */
#define DH_FAR_LANES 8            /* lanes that own a destination in the sum kernel = the stride of its key search */
// The ordered region behind the fp32 side buffer and its 64 statistic words, in 32-bit words:
//   count [dests] | start [dests + 1] | block sums [ceil(dests / DH_FAR_SCAN_BLOCK)] | (pad to 4 words) | records [4 * sources]
struct DhFarLayout {
  uint64_t count, start, bsum, recs, words, nblk;
};
DH_FAR_HD DhFarLayout dh_far_layout(const DhFarGeom& g) {
  DhFarLayout l;
  const uint64_t nd = dh_far_dests(g);
  l.nblk = (nd + DH_FAR_SCAN_BLOCK - 1) / DH_FAR_SCAN_BLOCK;
  l.count = 0;
  l.start = nd;
  l.bsum = l.start + nd + 1;
  l.recs = (l.bsum + l.nblk + 3) & ~(uint64_t)3;
  l.words = l.recs + 4 * dh_far_sources(g);
  return l;
}
