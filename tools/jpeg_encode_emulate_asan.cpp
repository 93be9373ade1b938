// Stand-alone host program for the encoder's device Huffman stage routines (csrc/jpeg_encode_huffman.h) under AddressSanitizer: it links
// the host source alone, has its own main, and runs on a CPU - nothing here touches a GPU or a Python process.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_encode_emulate_asan.cpp dan_amd/csrc/jpeg_encode.cpp -lpthread -o jpeg_encode_emulate_asan
//   ./jpeg_encode_emulate_asan image.rgb [image.rgb ...]
//
// An input file is two little-endian int32 (height, width) followed by height * width * 3 bytes of RGB (tests/golden/jpeg_encode_golden.npz
// holds such images; a few lines of numpy write them out).  For both chroma modes and qualities 10, 75 and 100 every image is run alone and
// all together in one batch: host pixel stage, the staging buffer, the emulation of the device stage and the host Huffman stage, with
// exactly-sized heap buffers so that a byte out of range is a report.  The program fails (exit 1) when a file of the emulation differs
// from the host stage's, when a status is not 0, or when a checked accessor refused an index.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/danhip.h"

void danhip_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}

struct Image {
  int32_t h, w;
  std::vector<uint8_t> rgb;
};

static int run(const std::vector<const Image*>& images, int32_t mode, int32_t quality) {
  const int32_t B = (int32_t)images.size();
  std::vector<int32_t> widths, heights;
  std::vector<const void*> srcs;
  for (const Image* im : images) {
    widths.push_back(im->w);
    heights.push_back(im->h);
    srcs.push_back(im->rgb.data());
  }
  std::vector<danhip_jpeg_enc_desc> descs((size_t)B);
  int64_t totals[3];
  if (danhip_jpeg_encode_prepare(widths.data(), heights.data(), srcs.data(), B, mode, quality, descs.data(), totals) != 0) return 1;
  std::vector<int16_t> coef((size_t)totals[0]);
  if (danhip_jpeg_encode_pixels_host(descs.data(), B, coef.data(), totals[0]) != 0) return 1;
  const size_t need = danhip_jpeg_encode_scan_staging_bytes(B);
  void* staging = aligned_alloc(16, (need + 15) & ~(size_t)15);
  std::vector<int32_t> prepared((size_t)B), status((size_t)B);
  std::vector<int64_t> sizes((size_t)B), hsizes((size_t)B);
  int bad = 0;
  if (danhip_jpeg_encode_scan_prepare(descs.data(), B, totals[0], totals[2], staging, need, prepared.data()) != 0) bad = 1;
  std::vector<uint8_t> files((size_t)totals[2], (uint8_t)0xc3), hfiles((size_t)totals[2], (uint8_t)0xc3);
  int64_t errors = 0;
  if (!bad && danhip_jpeg_encode_entropy_emulate_batch(staging, need, descs.data(), B, coef.data(), totals[0], files.data(), totals[2], sizes.data(),
                                                       status.data(), &errors) != 0)
    bad = 1;
  free(staging);
  if (danhip_jpeg_encode_entropy_batch(coef.data(), totals[0], descs.data(), B, 1, hfiles.data(), totals[2], hsizes.data()) != 0) bad = 1;
  for (int32_t i = 0; i < B && !bad; ++i) {
    const bool equal = sizes[(size_t)i] == hsizes[(size_t)i] &&
                       memcmp(files.data() + descs[(size_t)i].file_offset, hfiles.data() + descs[(size_t)i].file_offset, (size_t)hsizes[(size_t)i]) == 0;
    if (prepared[(size_t)i] != 0 || status[(size_t)i] != 0 || !equal) {
      printf("mode %d quality %d image %d (%d x %d): prepare %d device %d size %lld host %lld%s\n", mode, quality, i, images[(size_t)i]->w,
             images[(size_t)i]->h, prepared[(size_t)i], status[(size_t)i], (long long)sizes[(size_t)i], (long long)hsizes[(size_t)i],
             equal ? "" : "  DIFFERENT");
      bad = 1;
    }
  }
  if (errors) { printf("%lld indices refused by the checked accessors\n", (long long)errors); bad = 1; }
  return bad;
}

int main(int argc, char** argv) {
  std::vector<Image> images;
  for (int i = 1; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) { perror(argv[i]); return 2; }
    Image im;
    int32_t hw[2];
    if (fread(hw, 4, 2, f) != 2 || hw[0] < 1 || hw[1] < 1 || hw[0] > DANHIP_JPEG_MAX_DIM || hw[1] > DANHIP_JPEG_MAX_DIM) { fprintf(stderr, "%s: bad header\n", argv[i]); return 2; }
    im.h = hw[0]; im.w = hw[1];
    im.rgb.resize((size_t)im.h * im.w * 3);
    if (fread(im.rgb.data(), 1, im.rgb.size(), f) != im.rgb.size()) { fprintf(stderr, "%s: short file\n", argv[i]); return 2; }
    fclose(f);
    images.push_back(im);
  }
  if (images.empty()) { fprintf(stderr, "usage: %s image.rgb [...]\n", argv[0]); return 2; }
  int bad = 0, runs = 0;
  const int32_t modes[2] = {DANHIP_JPEG_420, DANHIP_JPEG_444}, qualities[3] = {10, 75, 100};
  std::vector<const Image*> all;
  for (const Image& im : images) all.push_back(&im);
  for (int32_t mode : modes)
    for (int32_t q : qualities) {
      for (const Image& im : images) { bad |= run({&im}, mode, q); ++runs; }
      bad |= run(all, mode, q);
      ++runs;
    }
  printf("%d runs over %d images: %s\n", runs, (int)images.size(), bad ? "FAILED" : "ok");
  return bad;
}
