// Stand-alone host program for the Huffman stage's routines (csrc/jpeg_huffman.h) under AddressSanitizer: it links the host source alone,
// has its own main, and runs on a CPU - nothing here touches a GPU or a Python process.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/jpeg_emulate_asan.cpp dan_amd/csrc/jpeg_entropy.cpp -lpthread -o jpeg_emulate_asan
//   ./jpeg_emulate_asan stream.jpg [stream.jpg ...]
//
// Every file is prepared and emulated alone and all together in one batch, with exactly-sized heap buffers so that a byte out of range is a
// report.  For every image the program prints the prepare status, the device status and the host stage's status, and fails (exit 1) when an
// image ends with device status 0 and coefficients that differ from the host stage's, when the host stage refuses an image that the
// emulation passes, or when a checked accessor refused an index.
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

static int run(const std::vector<std::vector<uint8_t>>& files) {
  const int32_t B = (int32_t)files.size();
  std::vector<const uint8_t*> datas;
  std::vector<int64_t> sizes;
  int64_t capacity = 0;
  for (const auto& f : files) {
    datas.push_back(f.data());
    sizes.push_back((int64_t)f.size());
    danhip_jpeg_info info;
    if (danhip_jpeg_inspect(f.data(), (int64_t)f.size(), &info) == 0) capacity += info.coef_count;
  }
  const size_t need = danhip_jpeg_scan_staging_bytes(datas.data(), sizes.data(), B);
  void* staging = aligned_alloc(16, (need + 15) & ~(size_t)15);
  std::vector<danhip_jpeg_desc> descs((size_t)B), hdescs((size_t)B);
  std::vector<int32_t> status((size_t)B), dev((size_t)B), hstatus((size_t)B);
  if (danhip_jpeg_scan_prepare_batch(datas.data(), sizes.data(), B, staging, need, capacity, descs.data(), status.data()) != 0) return 1;
  const size_t used = danhip_jpeg_scan_device_bytes(staging);
  void* exact = aligned_alloc(16, (used + 15) & ~(size_t)15);               // the used prefix alone: what the device would be given
  memcpy(exact, staging, used);
  free(staging);
  std::vector<int16_t> coef((size_t)capacity, (int16_t)-21846), hcoef((size_t)capacity, (int16_t)-21846);
  int64_t errors = 0;
  int bad = 0;
  if (danhip_jpeg_entropy_emulate_batch(exact, used, B, descs.data(), coef.data(), capacity, -1, dev.data(), &errors) != 0) bad = 1;
  free(exact);
  danhip_jpeg_entropy_decode_batch(datas.data(), sizes.data(), B, 1, hcoef.data(), capacity, hdescs.data(), hstatus.data());
  int64_t at = 0;
  for (int32_t i = 0; i < B; ++i) {
    danhip_jpeg_info info;
    const int64_t n = danhip_jpeg_inspect(datas[(size_t)i], sizes[(size_t)i], &info) == 0 ? info.coef_count : 0;
    const bool passed = status[(size_t)i] == 0 && dev[(size_t)i] == 0;
    const bool equal = n == 0 || memcmp(coef.data() + at, hcoef.data() + at, (size_t)n * 2) == 0;
    printf("image %d: prepare %d device %d host %d%s\n", i, status[(size_t)i], dev[(size_t)i], hstatus[(size_t)i], passed && !equal ? "  DIFFERENT" : "");
    if (passed && (!equal || hstatus[(size_t)i] != 0)) bad = 1;
    if (status[(size_t)i] > 0 && status[(size_t)i] != hstatus[(size_t)i]) bad = 1;
    at += n;
  }
  if (errors) { printf("%lld indices refused by the checked accessors\n", (long long)errors); bad = 1; }
  return bad;
}

int main(int argc, char** argv) {
  std::vector<std::vector<uint8_t>> files;
  for (int i = 1; i < argc; ++i) {
    FILE* f = fopen(argv[i], "rb");
    if (!f) { perror(argv[i]); return 2; }
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    files.push_back(d);
  }
  if (files.empty()) { fprintf(stderr, "usage: %s stream.jpg [...]\n", argv[0]); return 2; }
  int bad = 0;
  for (const auto& f : files) bad |= run({f});
  bad |= run(files);
  printf(bad ? "FAILED\n" : "ok\n");
  return bad;
}
