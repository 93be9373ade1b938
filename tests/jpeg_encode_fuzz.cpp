// Stand-alone driver of the host JPEG encoder (dan_amd/csrc/jpeg_encode.cpp, which makes no HIP call) for a sanitizer build:
//     g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan \
//         tests/jpeg_encode_fuzz.cpp dan_amd/csrc/jpeg_encode.cpp dan_amd/csrc/jpeg_entropy.cpp
// argv[1]: the number of rounds.  A round draws three images - seeded sizes 1 .. 70 per side with the odd ones favoured, noise, flat or a
// gradient - a mode and a quality, and runs: the whole encoder per image into a heap buffer of exactly the size the library's bound names;
// the decoder's entropy stage on each file (it must accept it and give the size back); prepare + host pixel stage + threaded entropy
// stage for the three together, every buffer allocated at exactly the size prepare names, so that a write outside is a heap overflow the
// sanitizer reports.  Passes (exit 0) when the two routes give the same files, the decoded coefficients equal the pixel stage's, and
// the sanitizer stays silent.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/danhip.h"

#if defined(__SANITIZE_ADDRESS__)
#define FUZZ_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define FUZZ_ASAN 1
#endif
#endif
#ifndef FUZZ_ASAN
#define FUZZ_ASAN 0
#endif

static char last_error[512];
void danhip_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(last_error, sizeof(last_error), fmt, ap);
  va_end(ap);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                                             // xorshift64*: the same images on every run
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int fail(const char* what, int round) {
  fprintf(stderr, "round %d: %s (%s)\n", round, what, last_error);
  return 1;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 20;
  long files = 0, bytes = 0;
  for (int round = 0; round < rounds; ++round) {
    const int B = 3;
    const int32_t mode = (rnd() & 1) ? DANHIP_JPEG_420 : DANHIP_JPEG_444;
    const int32_t quality = 1 + (int32_t)(rnd() % 100);
    int32_t widths[B], heights[B];
    std::vector<uint8_t> rgb[B];
    const void* srcs[B];
    for (int i = 0; i < B; ++i) {
      widths[i] = 1 + (int32_t)(rnd() % 70); heights[i] = 1 + (int32_t)(rnd() % 70);
      if (rnd() & 1) widths[i] |= 1;
      if (rnd() & 1) heights[i] |= 1;
      rgb[i].resize((size_t)widths[i] * heights[i] * 3);            // exactly the image: a read past it is reported
      const uint32_t kind = rnd() % 3;
      for (size_t k = 0; k < rgb[i].size(); ++k)
        rgb[i][k] = kind == 0 ? (uint8_t)rnd() : (kind == 1 ? (uint8_t)(255 * (round & 1)) : (uint8_t)(k * 255 / rgb[i].size()));
      srcs[i] = rgb[i].data();
    }
    // route 1: the whole encoder, image by image
    std::vector<uint8_t> single[B];
    for (int i = 0; i < B; ++i) {
      const int64_t cap = danhip_jpeg_encode_file_bound(widths[i], heights[i], mode);
      if (cap <= 0) return fail("no bound", round);
      std::vector<uint8_t> out((size_t)cap);
      int64_t n = 0;
      if (danhip_jpeg_encode_host(rgb[i].data(), widths[i], heights[i], mode, quality, out.data(), cap, &n) != DANHIP_OK) return fail("encode_host", round);
      if (n < 4 || n > cap || out[0] != 0xff || out[1] != 0xd8 || out[n - 2] != 0xff || out[n - 1] != 0xd9) return fail("no SOI / EOI", round);
      single[i].assign(out.begin(), out.begin() + n);
      std::vector<uint8_t> small((size_t)(n - 1));                   // one byte short: refused, nothing written past it
      int64_t m = 0;
      if (danhip_jpeg_encode_host(rgb[i].data(), widths[i], heights[i], mode, quality, small.data(), n - 1, &m) != DANHIP_EWORKSPACE || m != n)
        return fail("a short buffer was not refused", round);
      files += 1; bytes += n;
    }
    // route 2: prepare, the host pixel stage, the threaded entropy stage
    std::vector<danhip_jpeg_enc_desc> descs(B);
    int64_t totals[3];
    if (danhip_jpeg_encode_prepare(widths, heights, srcs, B, mode, quality, descs.data(), totals) != DANHIP_OK) return fail("prepare", round);
    std::vector<int16_t> coef((size_t)totals[0]);
    if (danhip_jpeg_encode_pixels_host(descs.data(), B, coef.data(), totals[0]) != DANHIP_OK) return fail("pixels_host", round);
    std::vector<uint8_t> out((size_t)totals[2]);
    int64_t sizes[B];
    if (danhip_jpeg_encode_entropy_batch(coef.data(), totals[0], descs.data(), B, 1 + (int32_t)(rnd() % 4), out.data(), totals[2], sizes) != DANHIP_OK)
      return fail("entropy_batch", round);
    for (int i = 0; i < B; ++i)
      if (sizes[i] != (int64_t)single[i].size() || memcmp(out.data() + descs[i].file_offset, single[i].data(), single[i].size()) != 0)
        return fail("the two routes give different files", round);
    // the decoder's entropy stage reads the files back into the same coefficients
    const uint8_t* datas[B];
    int64_t lens[B];
    for (int i = 0; i < B; ++i) { datas[i] = single[i].data(); lens[i] = (int64_t)single[i].size(); }
    std::vector<int16_t> back((size_t)totals[0]);
    std::vector<danhip_jpeg_desc> ddescs(B);
    int32_t status[B];
    if (danhip_jpeg_entropy_decode_batch(datas, lens, B, 2, back.data(), totals[0], ddescs.data(), status) != DANHIP_OK) return fail("decode_batch", round);
    for (int i = 0; i < B; ++i)
      if (status[i] != 0 || ddescs[i].width != widths[i] || ddescs[i].height != heights[i] || ddescs[i].mode != mode ||
          ddescs[i].coef_offset != descs[i].coef_offset)
        return fail("the decoder refuses the file or reads another geometry", round);
    if (memcmp(back.data(), coef.data(), coef.size() * sizeof(int16_t)) != 0) return fail("decoded coefficients differ from the pixel stage's", round);
  }
  printf("jpeg_encode_fuzz: %d rounds, %ld files, %ld bytes; sanitizers: %s\n", rounds, files, bytes, FUZZ_ASAN ? "address,undefined" : "none");
  return 0;
}
