// Box drawing on uint8 [H,W,3] device images (include/danhip.h, "Box drawing"): the rectangles of utility/draw_toolbox.py
// bboxes_draw_on_img for a list of images of any sizes in ONE launch, a (workgroup, image) grid through the item table.  One lane per
// pixel; the image's boxes are turned into integer rectangles once per workgroup and staged in LDS, 256 at a time; a lane paints its pixel
// when any box's band covers it.  One colour, no atomics: the result does not depend on the order of the boxes.  The rule (the project's
// own, restated in numpy by dan_amd/utility/draw_toolbox.py draw_reference):
//   skipped: classes[i] < 1, a coordinate that is not finite, x2 < x1 or y2 < y1 after truncation toward zero (clamped to +-2^30);
//   painted: x1 - t/2 <= x <= x2 + t/2 and y1 - t/2 <= y <= y2 + t/2, unless x1 + h <= x <= x2 - h and y1 + h <= y <= y2 - h, h = (t+1)/2.
// danhip_draw_boxes_labels_u8 is the same grid with the score label on a filled tab above each box (draw_boxes_labels_kernel below).
#include "common.h"
#include "draw_font.h"

namespace {

#define DRAW_CHUNK 256

__device__ __forceinline__ bool draw_corner(float v, int* out) {
  if (!(fabsf(v) <= 3.0e38f)) return false;                     // NaN or infinite
  v = fminf(fmaxf(v, -1073741824.0f), 1073741824.0f);
  *out = (int)v;                                                // toward zero
  return true;
}

__global__ __launch_bounds__(256) void draw_boxes_kernel(const danhip_draw_item* __restrict__ items, const float* __restrict__ boxes,
                                                         const int32_t* __restrict__ classes, int thickness) {
  const danhip_draw_item* it = items + blockIdx.y;
  if ((int)blockIdx.x >= it->groups) return;                     // uniform
  __shared__ int outer[DRAW_CHUNK][4];
  __shared__ int inner[DRAW_CHUNK][4];
  const int W = it->width, H = it->height;
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = pix < (long)W * H;
  const int y = live ? (int)(pix / W) : -1, x = live ? (int)(pix - (long)y * W) : -1;
  const int lo = thickness / 2, h = (thickness + 1) / 2;
  bool paint = false;
  for (int base = 0; base < it->num_boxes; base += DRAW_CHUNK) {
    const int n = min(DRAW_CHUNK, it->num_boxes - base);
    if ((int)threadIdx.x < n) {
      const long i = (long)it->first_box + base + threadIdx.x;
      const float* b = boxes + i * 4;
      int x1 = 0, y1 = 0, x2 = -1, y2 = -1;
      const bool ok = classes[i] >= 1 && draw_corner(b[0], &x1) && draw_corner(b[1], &y1) && draw_corner(b[2], &x2) && draw_corner(b[3], &y2) &&
                      x2 >= x1 && y2 >= y1;
      int* o = outer[threadIdx.x];
      int* q = inner[threadIdx.x];
      if (ok) {
        o[0] = x1 - lo; o[1] = y1 - lo; o[2] = x2 + lo; o[3] = y2 + lo;
        q[0] = x1 + h; q[1] = y1 + h; q[2] = x2 - h; q[3] = y2 - h;
      } else {
        o[0] = 0; o[1] = 0; o[2] = -1; o[3] = -1;               // covers no pixel
        q[0] = 0; q[1] = 0; q[2] = -1; q[3] = -1;
      }
    }
    __syncthreads();
    if (live && !paint) {
      for (int k = 0; k < n; ++k) {
        const bool in_outer = x >= outer[k][0] && y >= outer[k][1] && x <= outer[k][2] && y <= outer[k][3];
        const bool in_inner = x >= inner[k][0] && y >= inner[k][1] && x <= inner[k][2] && y <= inner[k][3];
        paint = paint || (in_outer && !in_inner);
      }
    }
    __syncthreads();
  }
  if (paint) {
    uint8_t* p = it->image + pix * 3;
    p[0] = 203; p[1] = 71; p[2] = 119;                           // colors_tableau[1]
  }
}

// The same grid with the score label (the rule: include/danhip.h, "Box drawing", and csrc/draw_font.h).  Two colours, so the order of the
// boxes decides: every lane walks ALL staged boxes in index order and keeps what the last box that touches its pixel paints there
// (0 nothing, 1 the colour, 2 white); within a box the text beats the tab beats the band.  The staging lane formats the score once per box;
// the per-pixel glyph test is one row byte from LDS and a bit test.  LDS: 3 x 4 KiB of rectangles + 1 KiB of text + the 96-byte font.
__global__ __launch_bounds__(256) void draw_boxes_labels_kernel(const danhip_draw_item* __restrict__ items, const float* __restrict__ boxes,
                                                                const int32_t* __restrict__ classes, const float* __restrict__ scores,
                                                                int thickness) {
  const danhip_draw_item* it = items + blockIdx.y;
  if ((int)blockIdx.x >= it->groups) return;                     // uniform
  __shared__ int4 outer[DRAW_CHUNK];
  __shared__ int4 inner[DRAW_CHUNK];
  __shared__ int4 tab[DRAW_CHUNK];
  __shared__ uint32_t text[DRAW_CHUNK];
  __shared__ uint8_t font[DRAW_FONT_GLYPHS][8];
  if (threadIdx.x < DRAW_FONT_GLYPHS * 8) {                      // read after the first barrier of the loop
    const int g = threadIdx.x >> 3, r = threadIdx.x & 7;
    font[g][r] = r < DRAW_FONT_H ? draw_font_row(g, r) : (uint8_t)0;
  }
  const int W = it->width, H = it->height;
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = pix < (long)W * H;
  const int y = live ? (int)(pix / W) : -1, x = live ? (int)(pix - (long)y * W) : -1;
  const int lo = thickness / 2, h = (thickness + 1) / 2;
  const int text_top = DRAW_FONT_H + DRAW_FONT_H - DRAW_FONT_BASELINE - 1;     // the top glyph row is y1 - 11, the bottom one y1 - 5
  int state = 0;
  for (int base = 0; base < it->num_boxes; base += DRAW_CHUNK) {
    const int n = min(DRAW_CHUNK, it->num_boxes - base);
    if ((int)threadIdx.x < n) {
      const long i = (long)it->first_box + base + threadIdx.x;
      const float* b = boxes + i * 4;
      int x1 = 0, y1 = 0, x2 = -1, y2 = -1;
      const bool ok = classes[i] >= 1 && draw_corner(b[0], &x1) && draw_corner(b[1], &y1) && draw_corner(b[2], &x2) && draw_corner(b[3], &y2) &&
                      x2 >= x1 && y2 >= y1;
      const uint32_t label = ok ? draw_format_score(scores[i]) : 0u;
      const int4 nothing = make_int4(0, 0, -1, -1);              // covers no pixel
      outer[threadIdx.x] = ok ? make_int4(x1 - lo, y1 - lo, x2 + lo, y2 + lo) : nothing;
      inner[threadIdx.x] = ok ? make_int4(x1 + h, y1 + h, x2 - h, y2 - h) : nothing;
      const int chars = (int)(label >> 24);
      // the tab keeps x1 and y1 for the text: the left glyph column is tab.x + lo, the top glyph row tab.w - text_top
      tab[threadIdx.x] = chars ? make_int4(x1 - lo, y1 - DRAW_FONT_H - thickness - DRAW_FONT_BASELINE, x1 + DRAW_FONT_ADVANCE * chars - 1, y1)
                               : nothing;
      text[threadIdx.x] = label;
    }
    __syncthreads();
    if (live) {
      for (int k = 0; k < n; ++k) {
        const int4 o = outer[k], q = inner[k], tb = tab[k];
        const uint32_t label = text[k];
        const bool in_outer = x >= o.x && y >= o.y && x <= o.z && y <= o.w;
        const bool in_inner = x >= q.x && y >= q.y && x <= q.z && y <= q.w;
        const bool in_tab = x >= tb.x && y >= tb.y && x <= tb.z && y <= tb.w;
        const unsigned dx = (unsigned)(x - (tb.x + lo)), dy = (unsigned)(y - (tb.w - text_top));
        bool white = false;
        if (dy < (unsigned)DRAW_FONT_H && dx < (unsigned)DRAW_FONT_ADVANCE * (label >> 24)) {   // no label: 0 characters
          const unsigned c = dx / DRAW_FONT_ADVANCE, col = dx - c * DRAW_FONT_ADVANCE;          // col 5 is the gap between characters
          const unsigned row = font[(label >> (4 * c)) & 15u][dy];
          white = col < (unsigned)DRAW_FONT_W && ((row >> (DRAW_FONT_W - 1 - col)) & 1u);
        }
        if ((in_outer && !in_inner) || in_tab || white) state = white ? 2 : 1;
      }
    }
    __syncthreads();
  }
  if (state) {
    uint8_t* p = it->image + pix * 3;
    if (state == 2) { p[0] = 255; p[1] = 255; p[2] = 255; }
    else            { p[0] = 203; p[1] = 71; p[2] = 119; }       // colors_tableau[1]
  }
}

}  // namespace

extern "C" size_t danhip_draw_item_bytes(void) { return sizeof(danhip_draw_item); }

extern "C" int danhip_draw_boxes_u8(const danhip_draw_item* items_host, const danhip_draw_item* items_dev, int32_t n_images,
                                    const float* boxes_dev, const int32_t* classes_dev, int64_t n_boxes, int32_t thickness, void* stream) {
  DH_REQUIRE(items_host && items_dev && n_images >= 1 && n_images <= 65535 && n_boxes >= 0, DANHIP_EINVAL,
             "draw_boxes_u8: bad arguments (1 <= n_images <= 65535, items in host and device memory)");
  DH_REQUIRE(thickness >= 1 && thickness <= 64, DANHIP_EINVAL, "draw_boxes_u8: thickness %d outside 1 .. 64", thickness);
  DH_REQUIRE(n_boxes == 0 || (boxes_dev && classes_dev), DANHIP_EINVAL, "draw_boxes_u8: NULL boxes / classes");
  int max_groups = 0;
  bool any = false;
  for (int32_t i = 0; i < n_images; ++i) {
    const danhip_draw_item* it = items_host + i;
    DH_REQUIRE(it->image && it->width >= 1 && it->height >= 1 && (int64_t)it->width * it->height <= ((int64_t)1 << 30), DANHIP_EINVAL,
               "draw_boxes_u8: item %d: NULL image or a size outside 1 .. 2^30 pixels", i);
    DH_REQUIRE(it->first_box >= 0 && it->num_boxes >= 0 && (int64_t)it->first_box + it->num_boxes <= n_boxes, DANHIP_EINVAL,
               "draw_boxes_u8: item %d: boxes [%d, +%d) leave the %lld rows", i, it->first_box, it->num_boxes, (long long)n_boxes);
    DH_REQUIRE(it->groups == (int32_t)(((int64_t)it->width * it->height + 255) / 256), DANHIP_EINVAL,
               "draw_boxes_u8: item %d: groups does not fit the size", i);
    max_groups = it->groups > max_groups ? it->groups : max_groups;
    any = any || it->num_boxes > 0;
  }
  if (!any) return DANHIP_OK;                                    // nothing to draw: nothing is launched
  hipLaunchKernelGGL(draw_boxes_kernel, dim3((unsigned)max_groups, (unsigned)n_images), dim3(256), 0, (hipStream_t)stream, items_dev, boxes_dev,
                     classes_dev, (int)thickness);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_draw_boxes_labels_u8(const danhip_draw_item* items_host, const danhip_draw_item* items_dev, int32_t n_images,
                                           const float* boxes_dev, const int32_t* classes_dev, const float* scores_dev, int64_t n_boxes,
                                           int32_t thickness, void* stream) {
  DH_REQUIRE(items_host && items_dev && n_images >= 1 && n_images <= 65535 && n_boxes >= 0, DANHIP_EINVAL,
             "draw_boxes_labels_u8: bad arguments (1 <= n_images <= 65535, items in host and device memory)");
  DH_REQUIRE(thickness >= 1 && thickness <= 64, DANHIP_EINVAL, "draw_boxes_labels_u8: thickness %d outside 1 .. 64", thickness);
  DH_REQUIRE(n_boxes == 0 || (boxes_dev && classes_dev && scores_dev), DANHIP_EINVAL, "draw_boxes_labels_u8: NULL boxes / classes / scores");
  int max_groups = 0;
  bool any = false;
  for (int32_t i = 0; i < n_images; ++i) {
    const danhip_draw_item* it = items_host + i;
    DH_REQUIRE(it->image && it->width >= 1 && it->height >= 1 && (int64_t)it->width * it->height <= ((int64_t)1 << 30), DANHIP_EINVAL,
               "draw_boxes_labels_u8: item %d: NULL image or a size outside 1 .. 2^30 pixels", i);
    DH_REQUIRE(it->first_box >= 0 && it->num_boxes >= 0 && (int64_t)it->first_box + it->num_boxes <= n_boxes, DANHIP_EINVAL,
               "draw_boxes_labels_u8: item %d: boxes [%d, +%d) leave the %lld rows", i, it->first_box, it->num_boxes, (long long)n_boxes);
    DH_REQUIRE(it->groups == (int32_t)(((int64_t)it->width * it->height + 255) / 256), DANHIP_EINVAL,
               "draw_boxes_labels_u8: item %d: groups does not fit the size", i);
    max_groups = it->groups > max_groups ? it->groups : max_groups;
    any = any || it->num_boxes > 0;
  }
  if (!any) return DANHIP_OK;                                    // nothing to draw: nothing is launched
  hipLaunchKernelGGL(draw_boxes_labels_kernel, dim3((unsigned)max_groups, (unsigned)n_images), dim3(256), 0, (hipStream_t)stream, items_dev,
                     boxes_dev, classes_dev, scores_dev, (int)thickness);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_draw_glyph(int32_t index, uint8_t rows_out[7]) {
  DH_REQUIRE(rows_out && index >= 0 && index < DRAW_FONT_GLYPHS, DANHIP_EINVAL, "draw_glyph: index %d outside 0 .. %d or NULL rows", index,
             DRAW_FONT_GLYPHS - 1);
  for (int r = 0; r < DRAW_FONT_H; ++r) rows_out[r] = draw_font_row(index, r);
  return DANHIP_OK;
}

extern "C" int danhip_draw_format_score(float score, char out[8]) {
  DH_REQUIRE(out, DANHIP_EINVAL, "draw_format_score: NULL out");
  const uint32_t label = draw_format_score(score);
  const int n = (int)(label >> 24);
  for (int k = 0; k < n; ++k) out[k] = "0123456789.%"[(label >> (4 * k)) & 15u];
  out[n] = '\0';
  return DANHIP_OK;
}
