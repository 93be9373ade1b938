// Stand-alone driver of the host JPEG entropy stage (dan_amd/csrc/jpeg_entropy.cpp, which makes no HIP call) for a sanitizer build:
//     g++ -std=c++17 -O0 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -static-libasan -static-libubsan \
//         tests/jpeg_progressive_fuzz.cpp dan_amd/csrc/jpeg_entropy.cpp
// argv[1]: a file of streams (int32 count, then per stream int32 size and the bytes), argv[2]: the most mutations per stream and kind.
// Every stream and a fixed, seeded set of mutations of it - truncation at and around every marker, single-byte changes in the marker
// segments and in the scans, Se / Ah / Al rewrites in every SOS - go through the three _ex entry points with the progressive flag, the
// coefficient buffer allocated at exactly the size the inspection names, so that a write outside the slot is a heap overflow the
// sanitizer reports.  Passes (exit 0) when every call returns, inspection and batch call agree, and the sanitizer stays silent.
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

void danhip_set_error(const char* fmt, ...) { (void)fmt; }          // csrc/capi.cpp keeps the message; nobody reads it here

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {                                             // xorshift64*: the same mutations on every run
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static long calls = 0, accepted = 0;
static long reasons[32];

static int run_one(const std::vector<uint8_t>& v) {
  const uint8_t* data = v.data();
  const int64_t n = (int64_t)v.size();
  for (uint32_t flags = 0; flags <= 1; ++flags) {
    danhip_jpeg_info info;
    const int reason = danhip_jpeg_inspect_ex(data, n, flags, &info);
    if (reason < 0 || reason != info.reason) { fprintf(stderr, "inspect: %d against info.reason %d\n", reason, info.reason); return 1; }
    std::vector<int16_t> coef((size_t)info.coef_count);               // exactly the slot: nothing may be written outside it
    danhip_jpeg_desc desc;
    int32_t status = -99;
    const int rc = danhip_jpeg_entropy_decode_batch_ex(&data, &n, 1, 1, flags, coef.data(), info.coef_count, &desc, &status);
    if (rc != DANHIP_OK || status < 0 || status > 18 || desc.status != status) { fprintf(stderr, "batch: rc %d status %d\n", rc, status); return 1; }
    if (reason != 0 && status != reason) { fprintf(stderr, "batch gives %d where the inspection gave %d\n", status, reason); return 1; }
    if (status == 0 && (desc.width != info.width || desc.height != info.height || desc.mode != info.mode || desc.coef_count != info.coef_count)) {
      fprintf(stderr, "descriptor and inspection disagree\n");
      return 1;
    }
    const uint8_t* const datas[1] = {data};
    const size_t need = danhip_jpeg_scan_staging_bytes(datas, &n, 1);
    std::vector<uint8_t> staging(need + 16);
    void* st = (void*)(((uintptr_t)staging.data() + 15) & ~(uintptr_t)15);
    int32_t pstatus = -99;
    const int prc = danhip_jpeg_scan_prepare_batch_ex(datas, &n, 1, flags, st, need, info.coef_count, &desc, &pstatus);
    if (prc != DANHIP_OK || (reason != 0 && pstatus != reason)) { fprintf(stderr, "prepare: rc %d status %d, inspection %d\n", prc, pstatus, reason); return 1; }
    if (flags) { ++calls; accepted += status == 0; ++reasons[status]; }
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s streams.bin mutations_per_kind\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const int cap = atoi(argv[2]);
  int32_t count = 0;
  if (fread(&count, 4, 1, f) != 1 || count < 1 || count > 4096) return 2;
  for (int32_t i = 0; i < count; ++i) {
    int32_t size = 0;
    if (fread(&size, 4, 1, f) != 1 || size < 0 || size > (1 << 24)) return 2;
    std::vector<uint8_t> base((size_t)size);
    if (size && fread(base.data(), 1, (size_t)size, f) != (size_t)size) return 2;
    if (run_one(base)) return 1;
    // the markers: FF followed by neither 00 nor FF
    std::vector<int64_t> marks, sos;
    for (int64_t p = 0; p + 1 < size; ++p)
      if (base[(size_t)p] == 0xFF && base[(size_t)p + 1] != 0x00 && base[(size_t)p + 1] != 0xFF) {
        marks.push_back(p);
        if (base[(size_t)p + 1] == 0xDA) sos.push_back(p);
      }
    for (size_t k = 0; k < marks.size(); ++k)                           // truncation at every marker, inside it and just behind it
      for (int64_t off : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)5}) {
        const int64_t cut = marks[k] + off;
        if (cut > size) continue;
        std::vector<uint8_t> v(base.begin(), base.begin() + cut);
        if (run_one(v)) return 1;
        v.push_back(0xFF); v.push_back(0xD9);                          // ... and the same with an EOI appended
        if (run_one(v)) return 1;
      }
    for (size_t k = 0; k < sos.size(); ++k) {                           // Se, Ah and Al of every scan header
      const int64_t p = sos[k];
      if (p + 4 >= size) continue;
      const int ns = base[(size_t)p + 4];
      const int64_t se = p + 6 + 2 * ns, ahal = p + 7 + 2 * ns;
      if (ahal >= size) continue;
      for (int val : {0, 1, 5, 62, 63, 64, 255}) {
        std::vector<uint8_t> v = base;
        v[(size_t)se] = (uint8_t)val;
        if (run_one(v)) return 1;
      }
      for (int j = 0; j < cap && j < 256; ++j) {
        std::vector<uint8_t> v = base;
        v[(size_t)ahal] = (uint8_t)(cap >= 256 ? j : rnd() & 255);
        if (run_one(v)) return 1;
      }
    }
    const int64_t first_sos = sos.empty() ? size : sos[0];
    for (int j = 0; j < cap && size > 2; ++j) {                         // single bytes: one in the header segments, one anywhere behind them
      std::vector<uint8_t> v = base;
      v[(size_t)(2 + rnd() % (uint32_t)(first_sos > 2 ? first_sos - 2 : 1))] ^= (uint8_t)(1u << (rnd() & 7));
      if (run_one(v)) return 1;
      v = base;
      const int64_t at = first_sos < size ? first_sos + rnd() % (uint32_t)(size - first_sos) : size - 1;
      v[(size_t)at] = (j & 1) ? (uint8_t)rnd() : (uint8_t)(v[(size_t)at] ^ (1u << (rnd() & 7)));
      if (run_one(v)) return 1;
    }
  }
  fclose(f);
  printf("%ld streams through the three entry points, %ld decoded; by reason:", calls, accepted);
  for (int r = 0; r < 32; ++r)
    if (reasons[r]) printf(" %d:%ld", r, reasons[r]);
  printf("\n%s\n", FUZZ_ASAN ? "sanitizers: address (this build is instrumented)" : "sanitizers: none");
  return 0;
}
