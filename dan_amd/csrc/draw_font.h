// The score label of the debug images (include/danhip.h, "Box drawing"): the project's own 5 x 7 bitmap font for '0' - '9', '.' and '%',
// and the rule that turns a score into its string.  Host and device run these same inline functions: the kernel of draw_exact.hip, the
// exports danhip_draw_glyph / danhip_draw_format_score, and through them the CPU tests.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DRAW_FONT_HD __host__ __device__
#else
#define DRAW_FONT_HD
#endif

#define DRAW_FONT_GLYPHS 12      // 0 - 9 the digits, 10 '.', 11 '%'
#define DRAW_FONT_W 5
#define DRAW_FONT_H 7            // text_h
#define DRAW_FONT_ADVANCE 6      // n characters are 6 n - 1 pixels wide
#define DRAW_FONT_BASELINE 2
#define DRAW_GLYPH_DOT 10
#define DRAW_GLYPH_PERCENT 11

// Row r (0 = top) of glyph g: bit 4 is the left column, bit 0 the right one; bits 5 - 7 are never set.
DRAW_FONT_HD inline uint8_t draw_font_row(int g, int r) {
  constexpr uint8_t rows[DRAW_FONT_GLYPHS][DRAW_FONT_H] = {
      {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E},   // 0
      {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E},   // 1
      {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},   // 2
      {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E},   // 3
      {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02},   // 4
      {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},   // 5
      {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E},   // 6
      {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08},   // 7
      {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},   // 8
      {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C},   // 9
      {0x00, 0x00, 0x00, 0x00, 0x00, 0x0C, 0x0C},   // .
      {0x18, 0x19, 0x02, 0x04, 0x08, 0x13, 0x03},   // %
  };
  return rows[g][r];
}

// The label of a score, packed: bits 4k .. 4k+3 the glyph index of character k (k < 6), bits 24 .. 26 the number of characters; 0 when no
// label is drawn.  v = score * 100 is ONE float32 multiply (what numpy computes for a float32 score); tenths = v * 10 rounded to the nearest
// integer, ties to even, on the exact value: the product of a 24-bit and a 4-bit significand is exact in double, and rint rounds it once
// (v * 10 in float32 would round a second time and print another digit for some scores).  Drawn when 0 <= tenths <= 9999 (NaN and the
// infinities fail the comparison; -0 and the negatives that round to it pass and print as 0.0%): the digits of tenths / 10, '.', tenths % 10, '%'.
DRAW_FONT_HD inline uint32_t draw_format_score(float score) {
  const float v = score * 100.0f;
  const double tenths = rint((double)v * 10.0);
  if (!(tenths >= 0.0 && tenths <= 9999.0)) return 0u;
  const uint32_t t = (uint32_t)tenths, whole = t / 10u;
  uint32_t text = 0u, n = 0u;
  if (whole >= 100u) text |= (whole / 100u) << (4u * n++);
  if (whole >= 10u) text |= ((whole / 10u) % 10u) << (4u * n++);
  text |= (whole % 10u) << (4u * n++);
  text |= (uint32_t)DRAW_GLYPH_DOT << (4u * n++);
  text |= (t % 10u) << (4u * n++);
  text |= (uint32_t)DRAW_GLYPH_PERCENT << (4u * n++);
  return text | (n << 24);
}
