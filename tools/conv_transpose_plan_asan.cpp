// Stand-alone check of the transposed convolution's host planning (dan_amd/csrc/conv_transpose_plan.h): shape validation, the weight
// gradient's slab split and its workspace layout, over a sweep of shapes.  CPU only:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan \
//         tools/conv_transpose_plan_asan.cpp -o /tmp/ct_plan && /tmp/ct_plan
// For every supported shape it lays the workspace out in a heap buffer of exactly the planned size and touches the first and last byte
// of every slab and every bias-gradient row (an off-by-one in the plan is a heap overflow the sanitizer reports), and checks that the
// slabs' K steps and the bias rows' pixels cover their ranges exactly once with no empty share.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../dan_amd/csrc/conv_transpose_plan.h"

static int fail(const char* what, long a, long b, long c) {
  printf("FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
  return 1;
}

static int check_shape(int64_t N, int64_t Hi, int64_t Wi, int crop_h, int crop_w, int64_t Ci, int64_t Co) {
  const int64_t Ho = 2 * Hi - crop_h, Wo = 2 * Wi - crop_w;
  if (ct_shape_error(N, Hi, Wi, Ho, Wo, Ci, Co)) return fail("a supported shape is refused", (long)Hi, (long)Wi, (long)Ci);
  const CtWgradPlan p = ct_wgrad_plan(N, Hi, Wi, Ho, Wo, Ci, Co);
  if (p.slabs < 1 || p.slabs > CT_WG_MAX_SLABS || p.steps_per_slab < 1) return fail("slab count", p.slabs, p.steps_per_slab, p.steps);
  if ((int64_t)(p.slabs - 1) * p.steps_per_slab >= p.steps) return fail("an empty slab", p.slabs, p.steps_per_slab, p.steps);
  if ((int64_t)p.slabs * p.steps_per_slab < p.steps) return fail("steps not covered", p.slabs, p.steps_per_slab, p.steps);
  if ((int64_t)p.steps * CT_BK < p.pixels || (int64_t)(p.steps - 1) * CT_BK >= p.pixels) return fail("step count", p.steps, (long)p.pixels, 0);
  if (p.slabs > 1 && p.steps_per_slab < CT_WG_MIN_STEPS) return fail("a slab below the minimum", p.slabs, p.steps_per_slab, p.steps);
  const int64_t Mo = N * Ho * Wo;
  if (p.db_rows < 1 || p.db_rows > CT_DB_MAX_ROWS) return fail("bias rows", p.db_rows, (long)p.db_pixels, (long)Mo);
  if ((int64_t)(p.db_rows - 1) * p.db_pixels >= Mo || (int64_t)p.db_rows * p.db_pixels < Mo) return fail("bias rows do not cover the pixels once", p.db_rows, (long)p.db_pixels, (long)Mo);
  if (p.db_off % 16 != 0) return fail("bias rows not 16-byte aligned", (long)p.db_off, 0, 0);
  if (p.bytes > ((size_t)1 << 24)) return 0;                      // (larger plans are checked by the arithmetic above, not allocated here)
  unsigned char* ws = (unsigned char*)malloc(p.bytes);
  if (!ws) return fail("malloc", (long)p.bytes, 0, 0);
  for (int s = 0; s < p.slabs; ++s) {
    unsigned char* slab = ws + (size_t)s * (size_t)p.dw_elems * sizeof(float);
    slab[0] = 1;
    slab[(size_t)p.dw_elems * sizeof(float) - 1] = 1;
  }
  for (int r = 0; r < p.db_rows; ++r) {
    unsigned char* row = ws + p.db_off + (size_t)r * (size_t)Co * sizeof(float);
    row[0] = 1;
    row[(size_t)Co * sizeof(float) - 1] = 1;
  }
  if (ws + p.db_off + (size_t)p.db_rows * (size_t)Co * sizeof(float) != ws + p.bytes) { free(ws); return fail("size", (long)p.bytes, 0, 0); }
  free(ws);
  return 0;
}

int main() {
  long shapes = 0;
  const int64_t sizes[] = {1, 2, 3, 5, 7, 8, 9, 16, 17, 20, 40, 63, 64, 65, 80};
  const int64_t chans[] = {64, 128, 192, 256, 512, 1024};
  const int64_t batches[] = {1, 2, 3, 16};
  for (int64_t N : batches)
    for (int64_t Hi : sizes)
      for (int64_t Wi : sizes)
        for (int64_t Ci : chans)
          for (int64_t Co : chans)
            for (int crop = 0; crop < 4; ++crop) {
              if (check_shape(N, Hi, Wi, crop >> 1, crop & 1, Ci, Co)) return 1;
              ++shapes;
            }
  // what must be refused
  struct { int64_t v[7]; } bad[] = {{{1, 3, 5, 6, 10, 72, 64}}, {{1, 3, 5, 6, 10, 64, 72}}, {{1, 3, 5, 7, 10, 64, 64}}, {{1, 3, 5, 6, 8, 64, 64}},
                                    {{0, 3, 5, 6, 10, 64, 64}}, {{1, 3, 5, 6, 10, 0, 64}}, {{1, 3, 5, 6, 10, 64, 1088}}, {{1, 0, 5, 0, 10, 64, 64}},
                                    {{1, 3, 5, 4, 10, 64, 64}}, {{1 << 20, 64, 64, 128, 128, 64, 64}}, {{-1, 3, 5, 6, 10, 64, 64}}};
  for (const auto& b : bad)
    if (!ct_shape_error(b.v[0], b.v[1], b.v[2], b.v[3], b.v[4], b.v[5], b.v[6])) return fail("an unsupported shape is accepted", (long)b.v[0], (long)b.v[5], (long)b.v[6]);
  // the LFPN's three levels at 640 x 640, batch 16: the plan stays inside its limits
  if (check_shape(16, 20, 20, 0, 0, 512, 512) || check_shape(16, 40, 40, 0, 0, 512, 512) || check_shape(16, 80, 80, 0, 0, 256, 256)) return 1;
#if defined(__SANITIZE_ADDRESS__)
  printf("sanitizers: address\n");
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
  printf("sanitizers: address\n");
#endif
#endif
  printf("ok: %ld shapes\n", shapes);
  return 0;
}
