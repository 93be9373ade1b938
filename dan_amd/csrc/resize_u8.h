// The per-pixel arithmetic of cv2.resize(..., INTER_LINEAR) on an 8-bit HWC image, shared by resize_u8_linear_kernel (evalpipe_exact.hip) and
// resize_u8_linear_batch_kernel (evalpipe_ragged_exact.hip): OpenCV's generic fixed-point path (11-bit coefficients, two integer passes),
// restated in oracle/evalpipe.py:cv2_resize_linear_u8.  Both files are compiled with -ffp-contract=off.
#pragma once
#include "common.h"

__device__ __forceinline__ int cv_round_to_short(float v) {      // saturate_cast<short>(float) = cvRound (half to even) + clamp
  int r = __float2int_rn(v);
  return r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
}

// Output pixel (dy, dx), all C channels, to out[0 .. C): both passes recomputed from the four source bytes (the integer formulas make that
// exact).  src is read byte by byte (any alignment); a source row starts every `pitch` bytes.  mirror: the source is read as if its columns
// were reversed (column x of the image that is resized = column W-1-x of src), i.e. the result of resizing image.flip(1).
__device__ __forceinline__ void resize_u8_linear_pixel(const uint8_t* __restrict__ src, long pitch, int H, int W, int C, bool mirror, double scale_x,
                                                       double scale_y, int dy, int dx, uint8_t* __restrict__ out) {
  float fx = (float)(((double)dx + 0.5) * scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  bool xedge = false;                                          // dx >= xmax: horizontal pass copies S[sx] * ONE
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= W - 1) { fx = 0.f; sx = W - 1; xedge = true; }
  float fy = (float)(((double)dy + 0.5) * scale_y - 0.5);
  int sy = (int)floorf(fy);
  fy -= (float)sy;
  const int a0 = cv_round_to_short((1.f - fx) * 2048.f), a1 = cv_round_to_short(fx * 2048.f);
  const int b0 = cv_round_to_short((1.f - fy) * 2048.f), b1 = cv_round_to_short(fy * 2048.f);
  int sy0 = sy, sy1 = sy + 1;                                  // rows are clamped (BORDER_REPLICATE), coefficients kept
  sy0 = sy0 < 0 ? 0 : (sy0 > H - 1 ? H - 1 : sy0);
  sy1 = sy1 < 0 ? 0 : (sy1 > H - 1 ? H - 1 : sy1);
  int sx1 = xedge ? sx : sx + 1;
  if (mirror) { sx = W - 1 - sx; sx1 = W - 1 - sx1; }
  const uint8_t* row0 = src + (long)sy0 * pitch;
  const uint8_t* row1 = src + (long)sy1 * pitch;
  for (int c = 0; c < C; ++c) {
    const int p00 = row0[(long)sx * C + c], p01 = row0[(long)sx1 * C + c];
    const int p10 = row1[(long)sx * C + c], p11 = row1[(long)sx1 * C + c];
    const int r0 = xedge ? p00 * 2048 : p00 * a0 + p01 * a1;
    const int r1 = xedge ? p10 * 2048 : p10 * a0 + p11 * a1;
    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    out[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}

// The fetch variant (face_chips_exact.hip, zero-padded chips): the same arithmetic on an H x W, 3-channel image that exists only through
// fetch(y, x, c) -> 0 .. 255, 0 <= y < H, 0 <= x < W: a rectangle that may leave the real image, where the fetch answers a constant.
// resize_u8_linear_pixel above is left as it is for its callers; the two are held together by the tests (pad off: the same bytes).
template <typename Fetch>
__device__ __forceinline__ void resize_u8_linear_pixel_fetch(Fetch fetch, int H, int W, double scale_x, double scale_y, int dy, int dx,
                                                             uint8_t* __restrict__ out) {
  float fx = (float)(((double)dx + 0.5) * scale_x - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  bool xedge = false;
  if (sx < 0) { fx = 0.f; sx = 0; }
  if (sx >= W - 1) { fx = 0.f; sx = W - 1; xedge = true; }
  float fy = (float)(((double)dy + 0.5) * scale_y - 0.5);
  int sy = (int)floorf(fy);
  fy -= (float)sy;
  const int a0 = cv_round_to_short((1.f - fx) * 2048.f), a1 = cv_round_to_short(fx * 2048.f);
  const int b0 = cv_round_to_short((1.f - fy) * 2048.f), b1 = cv_round_to_short(fy * 2048.f);
  int sy0 = sy, sy1 = sy + 1;
  sy0 = sy0 < 0 ? 0 : (sy0 > H - 1 ? H - 1 : sy0);
  sy1 = sy1 < 0 ? 0 : (sy1 > H - 1 ? H - 1 : sy1);
  const int sx1 = xedge ? sx : sx + 1;
  for (int c = 0; c < 3; ++c) {
    const int p00 = fetch(sy0, sx, c), p01 = fetch(sy0, sx1, c);
    const int p10 = fetch(sy1, sx, c), p11 = fetch(sy1, sx1, c);
    const int r0 = xedge ? p00 * 2048 : p00 * a0 + p01 * a1;
    const int r1 = xedge ? p10 * 2048 : p10 * a0 + p11 * a1;
    const int v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
    out[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
  }
}
