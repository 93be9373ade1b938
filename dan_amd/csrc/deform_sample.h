// The three sampling rules of cpp/Deform/deform_conv.cu that every deformable kernel (deform_conv.hip, deform_fused.hip, f32_infer.hip)
// restates: deformable_im2col_bilinear (:91-126), get_coordinate_weight (:177-221) and get_gradient_weight (:130-173) with the col2im
// guards (:311-326).  One definition each: the fused forward equals the stand-alone one, the tile kernels equal the per-item ones and all
// backward forms give the same dOffset because they call the same function, and a change to a seam rule is made in one place.
#pragma once
#include "common.h"
#include "deform_far.h"

// The (dh, dw) pair of one tap, stored as one 32-bit word of the offsets tensor
struct DeformOffset {
  float h, w;
};
__device__ __forceinline__ DeformOffset deform_offset_pair(unsigned oraw) {
  DeformOffset o;
  o.h = bf2f((bf16_t)(oraw & 0xffffu)); o.w = bf2f((bf16_t)(oraw >> 16));
  return o;
}

// ---- forward: deformable_im2col_gpu_kernel :261-268 + deformable_im2col_bilinear :94-125
struct DeformFwdTap {
  bool in;                                // the sample lies inside the image (:263); otherwise the value is 0 and the corners are pixel (0, 0)
  int h_low, h_high, w_low, w_high;       // corner rows / columns relative to (h_in, w_in)
  float wq[4];                            // weights of (low, low), (low, high), (high, low), (high, high)
};
// (h_in, w_in): the window's first input pixel; (di, dj) = (i, j) * dilation; (off_h, off_w): the tap's offset pair
__device__ __forceinline__ DeformFwdTap deform_fwd_tap(int h_in, int w_in, int di, int dj, float off_h, float off_w, int H, int W) {
  DeformFwdTap s;
  const float h_im = (float)(h_in + di) + off_h;                        // :261-262
  const float w_im = (float)(w_in + dj) + off_w;
  s.in = h_im >= 0 && w_im >= 0 && h_im < H && w_im < W;
  float mh = (float)di + off_h, mw = (float)dj + off_w;                 // :264-265 (relative to (h_in, w_in))
  if (!s.in) { mh = (float)(-h_in); mw = (float)(-w_in); }              // (any valid address: the result is discarded)
  const int cur_h = H - h_in, cur_w = W - w_in;                         // :266-268
  s.h_low = (int)floorf(mh); s.w_low = (int)floorf(mw);
  if (s.h_low >= cur_h - 1) { s.h_high = s.h_low = cur_h - 1; mh = (float)s.h_low; } else s.h_high = s.h_low + 1;
  if (s.w_low >= cur_w - 1) { s.w_high = s.w_low = cur_w - 1; mw = (float)s.w_low; } else s.w_high = s.w_low + 1;
  const float lh = mh - s.h_low, lw = mw - s.w_low, hh = 1 - lh, hw = 1 - lw;
  s.wq[0] = hh * hw; s.wq[1] = hh * lw; s.wq[2] = lh * hw; s.wq[3] = lh * lw;       // :118-125
  return s;
}
// One channel of the four corners blended in fp32.  The explicit fma chain is what "the column buffer" means: the stand-alone and the
// fused forward round the same way because both call this.  (Per channel, the callers unpack: as an eight-channel function the
// stand-alone kernel's `in ? blend : 0` moved behind all eight chains and hipcc then kept 4 instead of 12 corner loads in flight.)
__device__ __forceinline__ float deform_blend(const float (&wq)[4], float v1, float v2, float v3, float v4) {
  return fmaf(wq[3], v4, fmaf(wq[2], v3, fmaf(wq[1], v2, wq[0] * v1)));
}

// ---- dOffset: get_coordinate_weight (:177-221) for the absolute sampling position (inv_h, inv_w)
struct DeformCoordWeights {
  bool in;                                // out-of-range samples give 0 (:371-373): the weights are 0 and the corners sit at pixel 0
  int hl, hh, wl, wh;                     // absolute corner rows / columns
  float a_w, b_w, a_h, b_h;
};
__device__ __forceinline__ DeformCoordWeights deform_coord_weights(float inv_h, float inv_w, int H, int W) {
  DeformCoordWeights c;
  c.in = !(inv_h < 0 || inv_w < 0 || inv_h >= (float)H || inv_w >= (float)W);
  float ih = c.in ? inv_h : 0.f, iw = c.in ? inv_w : 0.f;
  c.hl = (int)ih; c.wl = (int)iw;                                       // (int) truncation as in the reference
  if (c.hl >= H - 1) { c.hh = c.hl = H - 1; ih = (float)c.hl; } else c.hh = c.hl + 1;
  if (c.wl >= W - 1) { c.wh = c.wl = W - 1; iw = (float)c.wl; } else c.wh = c.wl + 1;
  c.a_w = c.in ? (float)(c.wl + 1) - iw : 0.f; c.b_w = c.in ? iw - (float)c.wl : 0.f;
  c.a_h = c.in ? (float)(c.hl + 1) - ih : 0.f; c.b_h = c.in ? ih - (float)c.hl : 0.f;
  return c;
}
// s_h / s_w += the two coordinate-weight sums over eight channels of the corner values (low-low, low-high, high-low, high-high) times dS
__device__ __forceinline__ void deform_coord_sum8(const DeformCoordWeights& c, const float* vll, const float* vlh, const float* vhl,
                                                  const float* vhh, const float* cg, float& s_h, float& s_w) {
  const float a_w = c.a_w, b_w = c.b_w, a_h = c.a_h, b_h = c.b_h;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s_h += (-1.f * a_w * vll[e] + -1.f * b_w * vlh[e] + a_w * vhl[e] + b_w * vhh[e]) * cg[e];
    s_w += (-1.f * a_h * vll[e] + a_h * vlh[e] + -1.f * b_h * vhl[e] + b_h * vhh[e]) * cg[e];
  }
}

// ---- dX: get_gradient_weight (:130-173) + the guards of deformable_col2im_gpu_kernel (:311-326): CornerSet / corner_set live in deform_far.h,
// which the host emulation of the ordered far-corner path compiles too

// The weight corner_set() gives the corner that IS pixel (h, w), or 0: wg[k] and ok[k] factor into a row part and a column part
// (dup[1] = cw, dup[2] = ch, dup[3] = ch || cw), so the gather evaluates the two 1-D factors directly.
__device__ __forceinline__ float axis_factor(float inv, int target, int L) {
  float a = fmaxf(inv, 0.f);
  int lo = (int)a, hi;
  const bool clamp = lo >= L - 1;
  if (clamp) { hi = lo = L - 1; a = (float)lo; } else hi = lo + 1;
  const bool near = fabsf(inv - (float)target) < 1.f;
  float f = 0.f;
  if (target == lo) f = (float)(lo + 1) - a;                 // corners 0/1 (rows) or 0/2 (columns)
  else if (target == hi && !clamp) f = a + 1.f - (float)hi;  // the high corner, unless it duplicates the low one
  return near ? f : 0.f;
}
__device__ __forceinline__ float corner_weight_at(float inv_h, float inv_w, int h, int w, int H, int W) {
  if (inv_h < 0 || inv_h > (float)H || inv_w < 0 || inv_w > (float)W) return 0.f;
  return axis_factor(inv_h, h, H) * axis_factor(inv_w, w, W);
}
