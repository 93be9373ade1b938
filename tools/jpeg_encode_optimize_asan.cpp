// Stand-alone host program for the JPEG encoder's optimize=True (csrc/jpeg_encode.h dh_jenc_optimal_table, csrc/jpeg_encode.cpp
// danhip_jpeg_optimal_table_host / danhip_jpeg_encode_entropy_batch_ex) under AddressSanitizer and UBSan: it links the host source alone,
// has its own main, and runs on a CPU - nothing here touches a GPU or a Python process.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_encode_optimize_asan.cpp dan_amd/csrc/jpeg_encode.cpp -lpthread -o jpeg_encode_optimize_asan
//   ./jpeg_encode_optimize_asan
//
// No input: the count sets (one symbol, none, all equal, 40 Fibonacci numbers - the cut to 16 bits -, sums at the edge of int32) and the
// images (grey, ramp and noise at 1x1, 8x8, 16x16, 17x23, 64x48 and 200x136) are made here.  Every table goes into exactly-sized heap arrays,
// every batch of files into an exactly-sized heap buffer, for both chroma modes, qualities 1, 75 and 100, one and three threads.  The
// program fails (exit 1) when a table is no prefix code for its symbols, when an optimised file is not framed by SOI / EOI or is longer
// than the standard-table file, or when a coefficient without a baseline code is not refused.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../include/danhip.h"

void danhip_set_error(const char* fmt, ...) { (void)fmt; }

static int check_table(const std::vector<int32_t>& counts, bool expect_ok, const char* name) {
  std::unique_ptr<int32_t[]> c(new int32_t[257]);
  std::unique_ptr<uint8_t[]> bits(new uint8_t[17]), vals(new uint8_t[256]);
  for (int i = 0; i < 257; ++i) c[i] = i < (int)counts.size() ? counts[(size_t)i] : 0;
  const int rc = danhip_jpeg_optimal_table_host(c.get(), bits.get(), vals.get());
  if ((rc == 0) != expect_ok) { printf("%s: rc %d\n", name, rc); return 1; }
  if (rc != 0) return 0;
  int used = 0, listed = 0;
  double kraft = 0;
  for (int i = 0; i < 256; ++i) used += c[i] > 0;
  for (int l = 1; l <= 16; ++l) { listed += bits[l]; kraft += bits[l] / (double)(1 << l); }
  bool seen[256] = {false};
  for (int k = 0; k < listed; ++k) {
    if (c[vals[k]] <= 0 || seen[vals[k]]) { printf("%s: symbol %d listed without a count or twice\n", name, vals[k]); return 1; }
    seen[vals[k]] = true;
  }
  if (listed != used || bits[0] != 0 || kraft >= 1.0) { printf("%s: %d codes for %d symbols, Kraft sum %f\n", name, listed, used, kraft); return 1; }
  return 0;
}

struct Image {
  int32_t h, w;
  std::vector<uint8_t> rgb;
};

static Image make(int h, int w, int kind, uint32_t seed) {
  Image im;
  im.h = h; im.w = w;
  im.rgb.resize((size_t)h * w * 3);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x)
      for (int c = 0; c < 3; ++c) {
        seed = seed * 1664525u + 1013904223u;
        const int v = kind == 0 ? 128 : kind == 1 ? (x * 255 / (w > 1 ? w - 1 : 1) + c * y) & 255 : (int)(seed >> 24);
        im.rgb[((size_t)y * w + x) * 3 + c] = (uint8_t)v;
      }
  return im;
}

static int run(const std::vector<Image>& images, int32_t mode, int32_t quality, int32_t threads) {
  const int32_t B = (int32_t)images.size();
  std::vector<int32_t> widths, heights;
  std::vector<const void*> srcs;
  for (const Image& im : images) {
    widths.push_back(im.w);
    heights.push_back(im.h);
    srcs.push_back(im.rgb.data());
  }
  std::vector<danhip_jpeg_enc_desc> descs((size_t)B);
  int64_t totals[3];
  if (danhip_jpeg_encode_prepare(widths.data(), heights.data(), srcs.data(), B, mode, quality, descs.data(), totals) != 0) return 1;
  std::vector<int16_t> coef((size_t)totals[0]);
  if (danhip_jpeg_encode_pixels_host(descs.data(), B, coef.data(), totals[0]) != 0) return 1;
  std::vector<uint8_t> files((size_t)totals[2], (uint8_t)0xc3), plain((size_t)totals[2], (uint8_t)0xc3);
  std::vector<int64_t> sizes((size_t)B), psizes((size_t)B);
  if (danhip_jpeg_encode_entropy_batch_ex(coef.data(), totals[0], descs.data(), B, threads, DANHIP_JPEG_ENC_OPTIMIZE, files.data(), totals[2],
                                          sizes.data()) != 0)
    return 1;
  if (danhip_jpeg_encode_entropy_batch_ex(coef.data(), totals[0], descs.data(), B, threads, 0, plain.data(), totals[2], psizes.data()) != 0) return 1;
  int bad = 0;
  for (int32_t i = 0; i < B; ++i) {
    const uint8_t* f = files.data() + descs[(size_t)i].file_offset;
    const int64_t n = sizes[(size_t)i];
    if (n < 4 || n > psizes[(size_t)i] || f[0] != 0xff || f[1] != 0xd8 || f[n - 2] != 0xff || f[n - 1] != 0xd9) {
      printf("mode %d quality %d image %d (%d x %d): %lld bytes, standard tables %lld\n", mode, quality, i, images[(size_t)i].w, images[(size_t)i].h,
             (long long)n, (long long)psizes[(size_t)i]);
      bad = 1;
    }
  }
  coef[coef.size() - 64 + 5] = 32767;                      // the last block of the last image: no baseline code
  if (danhip_jpeg_encode_entropy_batch_ex(coef.data(), totals[0], descs.data(), B, threads, DANHIP_JPEG_ENC_OPTIMIZE, files.data(), totals[2],
                                          sizes.data()) == 0) {
    printf("mode %d quality %d: a value without a baseline code was taken\n", mode, quality);
    bad = 1;
  }
  return bad;
}

int main() {
  int bad = 0, runs = 0;
  std::vector<int32_t> one(256, 0), none(256, 0), equal(256, 9), fib(256, 0), edge(256, 0), over(256, 0);
  one[5] = 1000;
  int32_t a = 1, b = 1;
  for (int k = 0; k < 40; ++k) { fib[(size_t)(3 * k + 1)] = a; const int32_t n = a + b; a = b; b = n; }
  edge[0] = 0x7ffffffe;
  over[0] = over[1] = 0x40000000;
  bad |= check_table(one, true, "one symbol");
  bad |= check_table(none, true, "no symbol");
  bad |= check_table(equal, true, "all equal");
  bad |= check_table(fib, true, "fibonacci");
  bad |= check_table(edge, true, "sum 2^31 - 2");
  bad |= check_table(over, false, "sum 2^31");
  runs += 6;
  std::vector<Image> images;
  const int sizes[6][2] = {{1, 1}, {8, 8}, {16, 16}, {23, 17}, {48, 64}, {136, 200}};
  for (int k = 0; k < 6; ++k)
    for (int kind = 0; kind < 3; ++kind) images.push_back(make(sizes[k][0], sizes[k][1], kind, 77u + (uint32_t)k));
  const int32_t modes[2] = {DANHIP_JPEG_420, DANHIP_JPEG_444}, qualities[3] = {1, 75, 100};
  for (int32_t mode : modes)
    for (int32_t q : qualities) {
      bad |= run(images, mode, q, 3);
      for (const Image& im : images) bad |= run({im}, mode, q, 1);
      runs += 1 + (int)images.size();
    }
  printf("%d runs: %s\n", runs, bad ? "FAILED" : "ok");
  return bad;
}
