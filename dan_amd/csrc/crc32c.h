// CRC-32C (Castagnoli) arithmetic shared by the host entry points (crc32c.cpp) and the batch kernels (crc32c_exact.hip).
//
// Everything is in the REFLECTED representation the byte-wise loop uses: bit 31 of a word is the coefficient of x^0, bit 0 that of x^31,
// P = 0x82F63B78 is the polynomial without its x^32 term.  The register after feeding a message M into a zero register is
// raw(M) = M(x) * x^32 mod P, which is linear over GF(2):
//     raw(A || B) = raw(A) * x^(8 * len B)  ^  raw(B)
//     crc(M)      = raw(M)  ^  0xFFFFFFFF * x^(8 * len M)  ^  0xFFFFFFFF         (the init and the final xor)
// and because the init / final-xor terms of A, B and A || B cancel, the first line also holds for finished CRCs (danhip_crc32c_combine).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRC_HD __host__ __device__
#else
#define CRC_HD
#endif

namespace crc32c {

constexpr uint32_t kPoly = 0x82F63B78u;
constexpr uint32_t kOne = 0x80000000u;                 // x^0

// a * b mod P: 32 fixed steps (b runs through b * x^i, added where a has the coefficient of x^i)
CRC_HD constexpr uint32_t mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
  }
  return p;
}

// one byte through the register, without a table
CRC_HD constexpr uint32_t step_byte(uint32_t c, uint32_t byte) {
  c ^= byte;
  for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (kPoly & (0u - (c & 1u)));
  return c;
}

constexpr int kChunk = 128;                            // bytes one lane of the batch kernel walks
constexpr int kGroup = 256 * kChunk;                   // bytes one workgroup (256 lanes) covers: 32 KiB

struct Consts {
  uint32_t pow8[64];                                   // x^(8 * 2^i): byte counts as exponents, every bit of a 64-bit length
  uint32_t chunk_pow[kGroup / kChunk];                 // x^(8 * kChunk * h)
  uint32_t byte_pow[kChunk];                           // x^(8 * l)
  uint32_t slice[8][256];                              // slice[0] the byte table; slice[k][i] = slice[0][i] followed by k zero bytes
};

constexpr Consts make_consts() {
  Consts c{};
  c.pow8[0] = kOne >> 8;
  for (int i = 1; i < 64; ++i) c.pow8[i] = mul(c.pow8[i - 1], c.pow8[i - 1]);
  c.chunk_pow[0] = kOne;
  for (int h = 1; h < kGroup / kChunk; ++h) c.chunk_pow[h] = mul(c.chunk_pow[h - 1], c.pow8[7]);     // 2^7 = kChunk
  c.byte_pow[0] = kOne;
  for (int l = 1; l < kChunk; ++l) c.byte_pow[l] = mul(c.byte_pow[l - 1], c.pow8[0]);
  for (uint32_t i = 0; i < 256; ++i) c.slice[0][i] = step_byte(0, i);
  for (int k = 1; k < 8; ++k)
    for (int i = 0; i < 256; ++i) c.slice[k][i] = c.slice[0][c.slice[k - 1][i] & 255u] ^ (c.slice[k - 1][i] >> 8);
  return c;
}
static_assert(kChunk == 128 && kGroup == 32768, "chunk_pow is built from pow8[7]; the kernel's staging assumes 256 lanes of 8 16-byte lines");

// x^(8 * bytes) from the table of squares
CRC_HD inline uint32_t pow_bytes(const uint32_t* pow8, uint64_t bytes) {
  uint32_t r = kOne;
  for (int i = 0; bytes; ++i, bytes >>= 1)
    if (bytes & 1) r = mul(r, pow8[i]);
  return r;
}

CRC_HD inline uint32_t mask(uint32_t c) { return ((c >> 15) | (c << 17)) + 0xa282ead8u; }   // TensorFlow's crc32c::Mask

}  // namespace crc32c
