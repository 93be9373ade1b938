// Stand-alone host program for the ordered far-corner routines of the deformable backward (csrc/deform_far.h, csrc/deform_far_emulate.cpp) under
// AddressSanitizer: it links the host source alone, has its own main, and runs on a CPU - nothing here touches a GPU or a Python process.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/deform_far_emulate_asan.cpp dan_amd/csrc/deform_far_emulate.cpp -o deform_far_emulate_asan
//   ./deform_far_emulate_asan
//
// Maps of several sizes (a tile, one past a tile, a single row, a single pixel) and 1, 2 and 4 deformable groups get bf16 offsets of three
// kinds - quarter steps up to +-8 px, integers that throw many taps onto one pixel, and positions on and beyond the image's edges - with
// exactly-sized heap buffers, so that a byte out of range is a report.  Every run is checked against a second, independent summation (records
// listed first, then summed per destination in key order); the program fails (exit 1) on a difference, a refused index or a bad status.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../dan_amd/csrc/deform_far.h"
#include "../include/danhip.h"

void danhip_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static uint16_t to_bf16(float f) {                  // the values used here are exact in bf16: truncation is the conversion
  uint32_t u;
  memcpy(&u, &f, 4);
  return (uint16_t)(u >> 16);
}

struct Rec { uint32_t dest, key; float w; };

static int run(int N, int H, int W, int dg, int kind, int window) {
  const int C = dg * 64;
  const DhFarGeom g{N, H, W, C, dg};
  const int64_t M = (int64_t)N * H * W;
  std::vector<uint16_t> off((size_t)(M * dg * 18)), dS((size_t)(M * 9 * C));
  for (int64_t s = 0; s < M * dg * 9; ++s) {
    const int64_t m = s / (9 * dg);
    const int t = (int)(s % 9), ho = (int)((m / W) % H), wo = (int)(m % W);
    float oh, ow;
    if (kind == 0) { oh = (float)((int)(rnd() % 65) - 32) / 4.f; ow = (float)((int)(rnd() % 65) - 32) / 4.f; }
    else if (kind == 1) { oh = (float)(H / 2 - (ho - 1 + t / 3)); ow = (float)(W / 2 - (wo - 1 + t % 3)); if (rnd() % 3 == 0) { oh = 0.f; ow = 0.25f; } }
    else {
      const float eh[6] = {-0.25f, 0.f, (float)H - 1.f, (float)H - 0.25f, (float)H, (float)H + 0.25f};
      const float ew[6] = {-0.25f, 0.f, (float)W - 1.f, (float)W - 0.25f, (float)W, (float)W + 0.25f};
      oh = eh[rnd() % 6] - (float)(ho - 1 + t / 3); ow = ew[rnd() % 6] - (float)(wo - 1 + t % 3);
    }
    off[(size_t)(2 * s)] = to_bf16(oh);
    off[(size_t)(2 * s + 1)] = to_bf16(ow);
  }
  for (size_t i = 0; i < dS.size(); ++i) dS[i] = to_bf16((float)((int)(rnd() % 255) - 127) * ldexpf(1.f, (int)(rnd() % 17) - 8));
  std::vector<float> far_dx((size_t)(M * C), -1.f);
  int64_t records = -1, errors = -1;
  if (danhip_deform_far_ordered_emulate(off.data(), dS.data(), far_dx.data(), (int64_t)far_dx.size(), N, H, W, C, dg, window, &records, &errors) != 0 ||
      errors != 0) {
    fprintf(stderr, "emulation failed: N %d H %d W %d dg %d kind %d window %d\n", N, H, W, dg, kind, window);
    return 1;
  }
  // the same through a record list: window from the statistic, records per destination sorted by key, sequential fma
  uint32_t stat1 = 0;
  for (int64_t s = 0; s < M * dg * 9; ++s)
    if (dh_far_stat_outside(dh_far_act2f(off[(size_t)(2 * s)]), dh_far_act2f(off[(size_t)(2 * s + 1)]), 1.f)) ++stat1;
  const int R = dh_far_window(window, stat1, dh_far_thresh1(dh_far_sources(g)));
  std::vector<Rec> recs;
  for (int64_t s = M * dg * 9 - 1; s >= 0; --s) {                      // (descending on purpose: the sort below restores the order)
    const int64_t q = s / 9, m = q / dg;
    const int t = (int)(s % 9), grp = (int)(q % dg), wo = (int)(m % W), ho = (int)((m / W) % H), n = (int)(m / ((int64_t)W * H));
    const float oh = dh_far_act2f(off[(size_t)(2 * s)]), ow = dh_far_act2f(off[(size_t)(2 * s + 1)]);
    if (!dh_far_offset_outside(oh, ow, R)) continue;
    CornerSet cs;
    const unsigned mask = dh_far_mask(g, ho, wo, t, oh, ow, R, cs);
    for (int k = 3; k >= 0; --k)
      if ((mask >> k) & 1u) recs.push_back(Rec{dh_far_dest(g, n, cs.rh[k], cs.rw[k], grp), dh_far_key((uint32_t)m, t, k), cs.wg[k]});
  }
  if ((int64_t)recs.size() != records) { fprintf(stderr, "record count %zu against %lld\n", recs.size(), (long long)records); return 1; }
  std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.dest != b.dest ? a.dest < b.dest : a.key < b.key; });
  std::vector<float> want((size_t)(M * C), 0.f);
  for (const Rec& r : recs) {
    const int grp = (int)(r.dest % (uint32_t)dg);
    const size_t base = (size_t)(r.dest / (uint32_t)dg) * C + (size_t)grp * 64, row = (size_t)(r.key >> 2) * C + (size_t)grp * 64;
    for (int ch = 0; ch < 64; ++ch) want.at(base + ch) = dh_far_term(want.at(base + ch), r.w, dh_far_act2f(dS.at(row + ch)));
  }
  if (memcmp(want.data(), far_dx.data(), want.size() * sizeof(float)) != 0) {
    fprintf(stderr, "far_dx differs: N %d H %d W %d dg %d kind %d window %d\n", N, H, W, dg, kind, window);
    return 1;
  }
  printf("N %d  %3d x %3d  dg %d  kind %d  window %d (R = %d): %lld records\n", N, H, W, dg, kind, window, R, (long long)records);
  return 0;
}

int main() {
  const int shapes[][3] = {{2, 8, 16}, {2, 9, 17}, {1, 1, 23}, {1, 1, 1}, {1, 17, 33}};
  int bad = 0;
  for (const auto& s : shapes)
    for (int dg : {1, 2, 4})
      for (int kind = 0; kind < 3; ++kind)
        for (int window = 0; window < 3; ++window) bad += run(s[0], s[1], s[2], dg, kind, window);
  if (bad) { fprintf(stderr, "%d runs failed\n", bad); return 1; }
  printf("all runs agree\n");
  return 0;
}
