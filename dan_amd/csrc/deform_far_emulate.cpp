// Host emulation of the ordered far-corner path (deform_far.hip) with checked indexing: the per-record routines are those of deform_far.h,
// which the kernels call too, and the sums are formed in the order of the contract (include/danhip.h) - ascending (m, t, k) per destination,
// one fused multiply-add per record.  Host only; needs no HIP header, so a host compiler with a sanitizer takes it as it is
// (tools/deform_far_emulate_asan.cpp).
#include <stdint.h>

#include "../../include/danhip.h"
#include "deform_far.h"

void danhip_set_error(const char* fmt, ...);

namespace {

struct Checked {
  const uint16_t* offsets; int64_t n_offsets;
  const uint16_t* dS; int64_t n_dS;
  float* far_dx; int64_t n_far;
  int64_t errors = 0;
  uint16_t off(int64_t i) { if (i < 0 || i >= n_offsets) { ++errors; return 0; } return offsets[i]; }
  uint16_t ds(int64_t i) { if (i < 0 || i >= n_dS) { ++errors; return 0; } return dS[i]; }
  float* out(int64_t i) { if (i < 0 || i >= n_far) { ++errors; return nullptr; } return far_dx + i; }
};

}  // namespace

extern "C" int danhip_deform_far_ordered_emulate(const uint16_t* offsets, const uint16_t* dS, float* far_dx, int64_t far_dx_elems, int32_t N, int32_t H,
                                                 int32_t W, int32_t C, int32_t deformable_group, int32_t window, int64_t* records_out,
                                                 int64_t* range_errors) {
  if (records_out) *records_out = 0;
  if (range_errors) *range_errors = 0;
  if (!offsets || !dS || !far_dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || deformable_group <= 0 || C != deformable_group * 64) {
    danhip_set_error("deform_far_ordered_emulate: bad arguments (no NULL buffer, C / deformable_group == 64)");
    return DANHIP_EINVAL;
  }
  const DhFarGeom g{N, H, W, C, deformable_group};
  if (dh_far_sources(g) >= (1ull << 30) || window < 0 || window > 2 || far_dx_elems != (int64_t)N * H * W * C) {
    danhip_set_error("deform_far_ordered_emulate: sources %llu (< 2^30), window %d (0, 1, 2), far_dx_elems %lld (N*H*W*C)", (unsigned long long)dh_far_sources(g),
                     (int)window, (long long)far_dx_elems);
    return DANHIP_EINVAL;
  }
  const int dg = deformable_group;
  const int64_t M = (int64_t)N * H * W;
  Checked c{offsets, M * dg * 18, dS, M * 9 * C, far_dx, far_dx_elems};
  // the statistic (deform_far_stat_kernel) and the window it picks
  uint32_t stat1 = 0;
  for (int64_t s = 0; s < M * dg * 9; ++s)
    if (dh_far_stat_outside(dh_far_act2f(c.off(2 * s)), dh_far_act2f(c.off(2 * s + 1)), 1.f)) ++stat1;
  const int R = dh_far_window(window, stat1, dh_far_thresh1(dh_far_sources(g)));
  for (int64_t i = 0; i < far_dx_elems; ++i) far_dx[i] = 0.f;
  // Sources in ascending (m, t), corners in ascending k, every group: a destination meets its records in ascending key, so the running
  // sum in far_dx IS the contract's F = ((0 + c_1) + c_2) + ...
  int64_t records = 0;
  for (int64_t m = 0; m < M; ++m) {
    const int wo = (int)(m % W), ho = (int)((m / W) % H), n = (int)(m / ((int64_t)W * H));
    for (int t = 0; t < 9; ++t)
      for (int grp = 0; grp < dg; ++grp) {
        const int64_t s = (m * dg + grp) * 9 + t;
        const float oh = dh_far_act2f(c.off(2 * s)), ow = dh_far_act2f(c.off(2 * s + 1));
        if (!dh_far_offset_outside(oh, ow, R)) continue;
        CornerSet cs;
        const unsigned mask = dh_far_mask(g, ho, wo, t, oh, ow, R, cs);
        for (int k = 0; k < 4; ++k) {
          if (!((mask >> k) & 1u)) continue;
          ++records;
          const uint32_t d = dh_far_dest(g, n, cs.rh[k], cs.rw[k], grp);
          const int64_t row = (int64_t)(dh_far_key((uint32_t)m, t, k) >> 2);
          for (int ch = 0; ch < 64; ++ch) {
            float* o = c.out((int64_t)(d / (uint32_t)dg) * C + grp * 64 + ch);
            if (o) *o = dh_far_term(*o, cs.wg[k], dh_far_act2f(c.ds(row * C + grp * 64 + ch)));
          }
        }
      }
  }
  if (records_out) *records_out = records;
  if (range_errors) *range_errors = c.errors;
  if (c.errors) {
    danhip_set_error("deform_far_ordered_emulate: %lld indices out of range", (long long)c.errors);
    return DANHIP_EINVAL;
  }
  return DANHIP_OK;
}
