// The rectangle of a detection row (include/danhip.h, "Face chips"): integers only after the corners are truncated, 64-bit intermediates.
// Shared by face_chips_exact.hip and redact_exact.hip, so that a face chip and a redacted region of one row are the same rectangle.
#pragma once
#include "common.h"

// draw_exact.hip's corner: int() of the float, toward zero, clamped to +-2^30; false for NaN and the infinities
__device__ __forceinline__ bool chip_corner(float v, long* out) {
  if (!(fabsf(v) <= 3.0e38f)) return false;
  v = fminf(fmaxf(v, -1073741824.0f), 1073741824.0f);
  *out = (long)(int)v;
  return true;
}

// The rectangle of a detection row before it meets the image (corners, w / h test, margin, squaring), or false.  |corner| <= 2^30,
// margin_pm <= 4000: every product is below 2^44.
__device__ __forceinline__ bool face_chip_rect_unclipped(const float* __restrict__ row, int margin_pm, bool square, long* r) {
  long x1, y1, x2, y2;
  if (!(chip_corner(row[0], &x1) && chip_corner(row[1], &y1) && chip_corner(row[2], &x2) && chip_corner(row[3], &y2))) return false;
  long w = x2 - x1 + 1, h = y2 - y1 + 1;
  if (w < 1 || h < 1) return false;
  const long mx = w * margin_pm / 1000, my = h * margin_pm / 1000;      // non-negative operands: floor
  x1 -= mx; x2 += mx; y1 -= my; y2 += my;
  w += 2 * mx; h += 2 * my;
  if (square) {
    const long s = w > h ? w : h;
    x1 -= (s - w) / 2; x2 = x1 + s - 1;
    y1 -= (s - h) / 2; y2 = y1 + s - 1;
  }
  r[0] = x1; r[1] = y1; r[2] = x2; r[3] = y2;
  return true;
}

// The rectangle of a detection row in an H x W image (clipped to it), or false.
__device__ __forceinline__ bool face_chip_rect(const float* __restrict__ row, int H, int W, int margin_pm, bool square, int* rect) {
  long r[4];
  if (!face_chip_rect_unclipped(row, margin_pm, square, r)) return false;
  long x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  x1 = x1 < 0 ? 0 : x1; y1 = y1 < 0 ? 0 : y1;
  x2 = x2 > W - 1 ? W - 1 : x2; y2 = y2 > H - 1 ? H - 1 : y2;
  if (x1 > x2 || y1 > y2) return false;
  rect[0] = (int)x1; rect[1] = (int)y1; rect[2] = (int)x2; rect[3] = (int)y2;
  return true;
}

// danhip_face_chips_u8_ex's rectangle: pad keeps the unclipped corners (an empty intersection with the image still gives none); no chip
// when a side of what is kept exceeds DANHIP_FACE_CHIPS_MAX_SIDE.  Unclipped corners of a kept rectangle lie within +-(2^31 - 1): a side
// <= 32768 that meets the image has x1 > -32768 and x2 < W + 32768.
__device__ __forceinline__ bool face_chip_rect_ex(const float* __restrict__ row, int H, int W, int margin_pm, bool square, bool pad, int* rect) {
  long r[4];
  if (!face_chip_rect_unclipped(row, margin_pm, square, r)) return false;
  long x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
  if (x2 < 0 || y2 < 0 || x1 > W - 1 || y1 > H - 1) return false;
  if (!pad) {
    x1 = x1 < 0 ? 0 : x1; y1 = y1 < 0 ? 0 : y1;
    x2 = x2 > W - 1 ? W - 1 : x2; y2 = y2 > H - 1 ? H - 1 : y2;
  }
  if (x2 - x1 + 1 > DANHIP_FACE_CHIPS_MAX_SIDE || y2 - y1 + 1 > DANHIP_FACE_CHIPS_MAX_SIDE) return false;
  rect[0] = (int)x1; rect[1] = (int)y1; rect[2] = (int)x2; rect[3] = (int)y2;
  return true;
}
