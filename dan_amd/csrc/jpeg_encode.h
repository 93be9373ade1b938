// Integer arithmetic of the baseline JPEG encoder (include/danhip.h, "Baseline JPEG encode"), shared by the host entry points
// (jpeg_encode.cpp) and the device pixel stage (jpeg_encode_exact.hip) so that both run the same text.  Every line restates libjpeg-turbo:
// jccolor.c (RGB -> YCbCr, 16-bit fixed point), jcsample.c (h2v2 downsample), jcprepct.c / jccoefct.c (edges), jfdctint.c ("islow" forward
// DCT, CONST_BITS 13, PASS1_BITS 2) and jcdctmgr.c (quantisation by a 16-bit reciprocal).
//
// Where the textbook statement and libjpeg-turbo part, libjpeg-turbo is the specification (Pillow's bytes are the contract):
//   edges     a component is padded to ITS OWN whole blocks (width_in_blocks, height_in_blocks), not to whole MCUs: the right edge by
//             repeating the last column of the input, the bottom edge by repeating the last input row up to an even row count (4:2:0) and,
//             after the downsample, the last row of the component.  The luma blocks that only fill up the last MCU (an odd block count in a
//             4:2:0 image) are "dummy blocks": every AC coefficient 0, the DC coefficient that of the previous block of the MCU
//             (jccoefct.c compress_data), which the DC difference then codes as 0.  dh_jenc_block_source names that block.
//   quantiser the quotient (|c| + d/2) / d is taken as ((|c| + corr) * recip) >> shift with the 16-bit reciprocal of jcdctmgr.c
//             compute_reciprocal; d = 8 q >= 8, so its divisor-1 special case never occurs.  For the |c| a DCT of 8-bit samples can give the
//             two agree; the reciprocal form is what is computed.
//   quality   jpeg_quality_scaling: 5000 / q below 50, 200 - 2 q from 50 on; (base * scale + 50) / 100 clamped to [1, 255]
//             (force_baseline), so quality 100 gives tables of ones.
//   APP0      JFIF 1.01, density unit 0 with a 1 : 1 aspect (Pillow passes no dpi), no thumbnail.
//   optimize  the tables of save(optimize=True) are jchuff.c jpeg_gen_optimal_table's, not the textbook Huffman code (dh_jenc_optimal_table):
//             a 257th pseudo-symbol of count 1 keeps the all-ones code free; of two equal counts the LARGER symbol is merged first; the
//             lengths are cut to 16 by the counting rule of T.81 K.2 figure K.3, which is not an optimal length-limited code; and the DHT
//             lists the symbols by the length they had BEFORE that cut, then by value, so a symbol can stand in front of one whose final
//             code is shorter.  libjpeg skips counts above 10^9; no image here reaches them.  The statistics are those of the scan as it is
//             written: dummy blocks count (a DC difference of 0 and EOB each), ZRL and EOB are symbols 0xF0 and 0x00 of the AC tables.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DH_JENC_HD __host__ __device__ static inline __attribute__((always_inline))
#else
#define DH_JENC_HD static inline
#endif

// jccolor.c rgb_ycc_convert: FIX(x) = (int)(x * 65536 + 0.5); the chroma offset 128 and the rounding ONE_HALF - 1 sit in the blue / red term
DH_JENC_HD void dh_jenc_ycc(int r, int g, int b, int* y, int* cb, int* cr) {
  *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  *cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  *cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jcsample.c h2v2_downsample: the bias alternates 1, 2 along the OUTPUT row, starting with 1
DH_JENC_HD int dh_jenc_h2v2(int a, int b, int c, int d, int out_col) { return (a + b + c + d + 1 + (out_col & 1)) >> 2; }

// One 8-point pass of jfdctint.c's jpeg_fdct_islow.  first != 0: pass 1 (rows; results scaled up by 2^PASS1_BITS), else pass 2 (columns;
// the PASS1_BITS scaling removed, the factor 8 of the DCT stays for the quantiser).
DH_JENC_HD void dh_jenc_fdct_1d(int x[8], const int first) {
  const int t0 = x[0] + x[7], t7 = x[0] - x[7], t1 = x[1] + x[6], t6 = x[1] - x[6];
  const int t2 = x[2] + x[5], t5 = x[2] - x[5], t3 = x[3] + x[4], t4 = x[3] - x[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int sh = first ? 11 : 15;                         // CONST_BITS - PASS1_BITS | CONST_BITS + PASS1_BITS
  const int rnd = 1 << (sh - 1);
  if (first) {
    x[0] = (t10 + t11) * 4;                               // << PASS1_BITS (a product: the operand may be negative)
    x[4] = (t10 - t11) * 4;
  } else {
    x[0] = (t10 + t11 + 2) >> 2;
    x[4] = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  x[2] = (z1 + t13 * 6270 + rnd) >> sh;
  x[6] = (z1 + t12 * (-15137) + rnd) >> sh;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int o4 = t4 * 2446, o5 = t5 * 16819, o6 = t6 * 25172, o7 = t7 * 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  x[7] = (o4 + z1 + z3 + rnd) >> sh;
  x[5] = (o5 + z2 + z4 + rnd) >> sh;
  x[3] = (o6 + z2 + z3 + rnd) >> sh;
  x[1] = (o7 + z1 + z4 + rnd) >> sh;
}

// jcdctmgr.c quantize(): recip / corr are 16-bit, shift = r of compute_reciprocal (the C text shifts by (r - 16) + 16)
DH_JENC_HD int dh_jenc_quant(int coef, unsigned recip, unsigned corr, unsigned shift) {
  const unsigned a = (unsigned)(coef < 0 ? -coef : coef);
  const int q = (int)(((a + corr) * recip) >> shift);
  return coef < 0 ? -q : q;
}

// jcdctmgr.c compute_reciprocal for a divisor >= 2 (here 8 q, 8 .. 2040)
static inline void dh_jenc_reciprocal(unsigned divisor, uint16_t* recip, uint16_t* corr, uint8_t* shift) {
  int b = 0;
  while ((2u << b) <= divisor) ++b;                       // flss(divisor) - 1
  int r = 16 + b;
  unsigned fq = (1u << r) / divisor;
  const unsigned fr = (1u << r) % divisor;
  unsigned c = divisor / 2;
  if (fr == 0) {
    fq >>= 1;
    --r;
  } else if (fr <= divisor / 2) {
    ++c;
  } else {
    ++fq;
  }
  *recip = (uint16_t)fq; *corr = (uint16_t)c; *shift = (uint8_t)r;
}

// The block whose samples block (by, bx) of component c is transformed from, and whether the block is a dummy block (DC only).
// real_bw / real_bh: the component's own block grid, ceil(comp_w / 8) x ceil(comp_h / 8); the MCU is hs x vs luma blocks.
DH_JENC_HD int dh_jenc_block_source(int by, int bx, int real_bw, int real_bh, int* sy, int* sx) {
  *sy = by; *sx = bx;
  if (by >= real_bh) {                                    // a row of dummy blocks: all take the DC of the MCU's last block one row up
    *sy = by - 1;
    *sx = (bx | 1) < real_bw ? (bx | 1) : (bx & ~1);
    return 1;
  }
  if (bx >= real_bw) {
    *sx = bx - 1;
    return 1;
  }
  return 0;
}

// ---- optimize=True: jchuff.c jpeg_gen_optimal_table over the counts of one table ----
// counts[257]: occurrences of symbol 0 .. 255 (entry 256 is not read: it is the pseudo-symbol, whose count is 1 by rule); their sum stays
// below 2^31 (a 16384 x 16384 image has 2^28 coefficients).  bits[17]: bits[l] = codes of length l, bits[0] = 0; vals[256]: the symbols in
// DHT order, zero behind the last.  work: DH_JENC_TABLE_WORK int32 of scratch (LDS in a kernel).  Returns 0 - bits and vals all zero - when
// a merge chain is longer than libjpeg's 32 (it raises JERR_HUFF_CLEN_OVERFLOW there), else 1.
#define DH_JENC_TABLE_WORK (3 * 257 + 33)
DH_JENC_HD int dh_jenc_optimal_table(const int32_t* counts, uint8_t* bits, uint8_t* vals, int32_t* work) {
  int32_t* freq = work;
  int32_t* others = work + 257;
  int32_t* codesize = work + 2 * 257;
  int32_t* nbits = work + 3 * 257;                          // [33]
  for (int i = 0; i < 256; ++i) freq[i] = counts[i] > 0 ? counts[i] : 0;
  freq[256] = 1;                                            // step 1: the reserved symbol, so that no code is all ones
  for (int i = 0; i < 257; ++i) { others[i] = -1; codesize[i] = 0; }
  for (int i = 0; i < 33; ++i) nbits[i] = 0;
  for (int i = 0; i < 17; ++i) bits[i] = 0;
  for (int i = 0; i < 256; ++i) vals[i] = 0;
  for (;;) {                                                // step 2: merge the two smallest; "<=" lets the larger index win a tie
    int c1 = -1, c2 = -1;
    int32_t v = 0x7fffffff;
    for (int i = 0; i < 257; ++i)
      if (freq[i] && freq[i] <= v) { v = freq[i]; c1 = i; }
    v = 0x7fffffff;
    for (int i = 0; i < 257; ++i)
      if (freq[i] && freq[i] <= v && i != c1) { v = freq[i]; c2 = i; }
    if (c2 < 0) break;
    freq[c1] += freq[c2];
    freq[c2] = 0;
    ++codesize[c1];                                         // step 3: every symbol of both chains moves one level down
    while (others[c1] >= 0) { c1 = others[c1]; ++codesize[c1]; }
    others[c1] = c2;
    ++codesize[c2];
    while (others[c2] >= 0) { c2 = others[c2]; ++codesize[c2]; }
  }
  for (int i = 0; i < 257; ++i)
    if (codesize[i]) {
      if (codesize[i] > 32) return 0;
      ++nbits[codesize[i]];
    }
  for (int i = 32; i > 16; --i)                             // step 4, figure K.3: a pair of length i becomes one of length i - 1 and a
    while (nbits[i] > 0) {                                  // shorter code (from i - 2, or the next length up that has one) grows by one bit
      int j = i - 2;
      while (j > 0 && nbits[j] == 0) --j;
      if (j == 0) return 0;                                 // cannot happen for lengths of a prefix code
      nbits[i] -= 2; ++nbits[i - 1]; nbits[j + 1] += 2; --nbits[j];
    }
  int last = 16;
  while (last > 0 && nbits[last] == 0) --last;
  if (last > 0) --nbits[last];                              // step 5: the pseudo-symbol holds the longest code
  for (int i = 1; i <= 16; ++i) bits[i] = (uint8_t)nbits[i];
  int p = 0;
  for (int l = 1; l <= 32; ++l)                             // step 6: by the length before the cut, then by value
    for (int j = 0; j < 256; ++j)
      if (codesize[j] == l) vals[p++] = (uint8_t)j;
  return 1;
}
