// CRC-32C on the host: danhip_crc32c_host (slicing-by-8 tables; the SSE4.2 instruction where the CPU has it) and danhip_crc32c_combine.
// No HIP call: both work in a process without a GPU.  Little-endian hosts only (as the checkpoint format itself).
#include <cstring>

#include "../../include/danhip.h"
#include "crc32c.h"

namespace {
constexpr crc32c::Consts kC = crc32c::make_consts();

uint32_t crc_tables(const uint8_t* p, size_t n, uint32_t c) {
  const auto& T = kC.slice;
  for (; n >= 8; n -= 8, p += 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = T[7][lo & 255] ^ T[6][(lo >> 8) & 255] ^ T[5][(lo >> 16) & 255] ^ T[4][lo >> 24] ^ T[3][hi & 255] ^ T[2][(hi >> 8) & 255] ^
        T[1][(hi >> 16) & 255] ^ T[0][hi >> 24];
  }
  for (; n; --n, ++p) c = T[0][(c ^ *p) & 255] ^ (c >> 8);
  return c;
}

#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#define DANHIP_CRC_SSE42 1
__attribute__((target("sse4.2"))) uint32_t crc_sse42(const uint8_t* p, size_t n, uint32_t c) {
  uint64_t c64 = c;
  for (; n >= 8; n -= 8, p += 8) {
    uint64_t w;
    memcpy(&w, p, 8);
    c64 = __builtin_ia32_crc32di(c64, w);
  }
  c = (uint32_t)c64;
  for (; n; --n, ++p) c = __builtin_ia32_crc32qi(c, *p);
  return c;
}
bool have_sse42() {
  static const bool v = __builtin_cpu_supports("sse4.2");
  return v;
}
#endif
}  // namespace

// form: 0 the fastest the CPU has, 1 the portable tables (tests compare the two)
extern "C" uint32_t danhip_crc32c_host_form(const void* data, size_t n, uint32_t crc, int32_t form) {
  if (!data || n == 0) return crc;
  uint32_t c = crc ^ 0xFFFFFFFFu;
#ifdef DANHIP_CRC_SSE42
  if (form == 0 && have_sse42()) return crc_sse42((const uint8_t*)data, n, c) ^ 0xFFFFFFFFu;
#endif
  return crc_tables((const uint8_t*)data, n, c) ^ 0xFFFFFFFFu;
}

extern "C" uint32_t danhip_crc32c_host(const void* data, size_t n, uint32_t crc) { return danhip_crc32c_host_form(data, n, crc, 0); }

extern "C" uint32_t danhip_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
  return crc32c::mul(crc_a, crc32c::pow_bytes(kC.pow8, len_b)) ^ crc_b;
}
