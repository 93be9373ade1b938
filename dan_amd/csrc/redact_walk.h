// Face redaction (include/danhip.h, "Face redaction"): the index arithmetic of the item walk as plain functions.  redact_exact.hip's
// kernels call them on the device, its danhip_redact_extent / _item_count / _tile / _window / _cell / _in_shape export them to the host
// (tests/test_redact_cpu.py holds them to the Python rule without a device), and the header compiles alone with any C++ compiler.
// Integers only.  A rectangle is (x1, y1, x2, y2), inclusive, inside its H x W image, with sides <= 32768; 1 <= e <= 255.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define REDACT_FN __host__ __device__ inline
#else
#define REDACT_FN inline
#endif

constexpr int kRedactMaxExtent = 255, kRedactBlur = 0, kRedactMosaic = 1, kRedactFill = 2, kRedactRect = 0, kRedactEllipse = 1;

// e = clamp(max(wc, hc) * strength_pm / 1000, 1, 255): sides <= 32768 and strength_pm <= 1000 keep the product below 2^25
REDACT_FN int redact_extent(int wc, int hc, int strength_pm) {
  const int e = (wc > hc ? wc : hc) * strength_pm / 1000;
  return e < 1 ? 1 : e > kRedactMaxExtent ? kRedactMaxExtent : e;
}

REDACT_FN int redact_cell_side(int e) { return e < 2 ? 2 : e; }

REDACT_FN int redact_units(int side, int unit) { return (side + unit - 1) / unit; }     // pieces of `unit` that cover `side`

// piece `index` of the inclusive range [a, b] cut into pieces of `unit` from a: [*lo, *hi], the last one short
REDACT_FN void redact_piece(int a, int b, int unit, int index, int* lo, int* hi) {
  *lo = a + index * unit;
  *hi = *lo + unit - 1 < b ? *lo + unit - 1 : b;
}

// [p - e, p + e] (or a range [a - e, b + e]) intersected with 0 .. n-1
REDACT_FN void redact_grow(int a, int b, int e, int n, int* lo, int* hi) {
  *lo = a - e < 0 ? 0 : a - e;
  *hi = b + e > n - 1 ? n - 1 : b + e;
}

// work items of a rectangle: tiles of band rows x strip columns (blur, fill), row-major; cells of side c = max(2, e) (mosaic), row-major
REDACT_FN int64_t redact_item_count(int mode, const int* rect, int e, int band, int strip) {
  const int wc = rect[2] - rect[0] + 1, hc = rect[3] - rect[1] + 1;
  if (mode == kRedactMosaic) {
    const int c = redact_cell_side(e);
    return (int64_t)redact_units(wc, c) * redact_units(hc, c);
  }
  return (int64_t)redact_units(wc, strip) * redact_units(hc, band);
}

// tile `item` of a rectangle: t = (tx1, ty1, tx2, ty2), and s = what a blur item of extent e reads, the tile grown by e inside the image
REDACT_FN void redact_tile(int H, int W, const int* rect, int e, int band, int strip, int64_t item, int* t, int* s) {
  const int strips = redact_units(rect[2] - rect[0] + 1, strip);
  const int by = (int)(item / strips), bx = (int)(item - (int64_t)by * strips);
  redact_piece(rect[0], rect[2], strip, bx, &t[0], &t[2]);
  redact_piece(rect[1], rect[3], band, by, &t[1], &t[3]);
  redact_grow(t[0], t[2], e, W, &s[0], &s[2]);
  redact_grow(t[1], t[3], e, H, &s[1], &s[3]);
}

// cell `cell` of a rectangle cut into cells of side c from its top-left corner: (cx1, cy1, cx2, cy2), clipped to the rectangle
REDACT_FN void redact_cell(const int* rect, int c, int64_t cell, int* out) {
  const int cells_x = redact_units(rect[2] - rect[0] + 1, c);
  const int cy = (int)(cell / cells_x), cx = (int)(cell - (int64_t)cy * cells_x);
  redact_piece(rect[0], rect[2], c, cx, &out[0], &out[2]);
  redact_piece(rect[1], rect[3], c, cy, &out[1], &out[3]);
}

// pixel (px, py) of the rectangle lies in its shape.  |2 * d + 1 - side| < 2^15 + ..., sides <= 2^15: each product is below 2^61
REDACT_FN bool redact_in_shape(int shape, const int* rect, int px, int py) {
  if (px < rect[0] || px > rect[2] || py < rect[1] || py > rect[3]) return false;
  if (shape == kRedactRect) return true;
  const int64_t wc = rect[2] - rect[0] + 1, hc = rect[3] - rect[1] + 1;
  const int64_t u = 2 * (int64_t)(px - rect[0]) + 1 - wc, v = 2 * (int64_t)(py - rect[1]) + 1 - hc;
  return u * u * hc * hc + v * v * wc * wc <= wc * wc * hc * hc;
}
