// Geometry of a decodable JPEG image, derived from (width, height, mode) alone: shared by the host decoder that fills the descriptors
// (jpeg_entropy.cpp) and by the launcher that re-derives and checks them before the device sees one (jpeg_exact.hip).  Host code.
#pragma once
#include <stdint.h>

#include "../../include/danhip.h"

#define DH_JPEG_IDCT_BLOCKS_PER_GROUP 32      /* launch 1: 256 threads, 8 lanes per block */
#define DH_JPEG_RGB_ITEMS_PER_GROUP 256       /* launch 2: 256 lanes, each 8 pixels of one row */

struct DhJpegGeom {
  int32_t ncomp, hs, vs;                      // luma sampling factors (chroma is 1x1)
  int32_t blocks_w[3], blocks_h[3], comp_w[3], comp_h[3];
  int64_t blocks, coef_count, plane_bytes[3], out_bytes;
  int32_t idct_groups, rgb_groups;
};

static inline int64_t dh_jpeg_align(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

// false: (width, height, mode) is outside what the decoder accepts
static inline bool dh_jpeg_geometry(int32_t width, int32_t height, int32_t mode, DhJpegGeom* g) {
  if (width < 1 || height < 1 || width > DANHIP_JPEG_MAX_DIM || height > DANHIP_JPEG_MAX_DIM) return false;
  if (mode < DANHIP_JPEG_GREY || mode > DANHIP_JPEG_420) return false;
  g->ncomp = mode == DANHIP_JPEG_GREY ? 1 : 3;
  g->hs = (mode == DANHIP_JPEG_422 || mode == DANHIP_JPEG_420) ? 2 : 1;
  g->vs = mode == DANHIP_JPEG_420 ? 2 : 1;
  const int32_t mcus_x = (width + 8 * g->hs - 1) / (8 * g->hs), mcus_y = (height + 8 * g->vs - 1) / (8 * g->vs);
  g->blocks = 0;
  for (int c = 0; c < 3; ++c) {
    const int32_t h = c == 0 ? g->hs : 1, v = c == 0 ? g->vs : 1;
    const bool on = c < g->ncomp;
    g->blocks_w[c] = on ? mcus_x * h : 0;
    g->blocks_h[c] = on ? mcus_y * v : 0;
    g->comp_w[c] = on ? (width * h + g->hs - 1) / g->hs : 0;
    g->comp_h[c] = on ? (height * v + g->vs - 1) / g->vs : 0;
    g->plane_bytes[c] = (int64_t)g->blocks_w[c] * g->blocks_h[c] * 64;
    g->blocks += (int64_t)g->blocks_w[c] * g->blocks_h[c];
  }
  g->coef_count = g->blocks * 64;
  g->out_bytes = (int64_t)width * height * 3;
  g->idct_groups = (int32_t)((g->blocks + DH_JPEG_IDCT_BLOCKS_PER_GROUP - 1) / DH_JPEG_IDCT_BLOCKS_PER_GROUP);
  g->rgb_groups = (int32_t)(((int64_t)height * ((width + 7) / 8) + DH_JPEG_RGB_ITEMS_PER_GROUP - 1) / DH_JPEG_RGB_ITEMS_PER_GROUP);
  return true;
}

// Checks every field of a decodable descriptor against the geometry and the buffer sizes.  NULL = fine, else what is wrong.
static inline const char* dh_jpeg_desc_check(const danhip_jpeg_desc* d, int64_t coef_count, int64_t out_bytes, int64_t workspace_bytes) {
  DhJpegGeom g;
  if (!dh_jpeg_geometry(d->width, d->height, d->mode, &g)) return "size or mode outside the accepted range";
  if (d->ncomp != g.ncomp) return "component count does not fit the mode";
  for (int c = 0; c < 3; ++c) {
    if (d->blocks_w[c] != g.blocks_w[c] || d->blocks_h[c] != g.blocks_h[c] || d->comp_w[c] != g.comp_w[c] || d->comp_h[c] != g.comp_h[c])
      return "block grid does not fit the size";
    if (d->quant_index[c] < 0 || d->quant_index[c] > 3) return "quantisation table index outside [0, 3]";
    if (c < g.ncomp && (d->plane_offset[c] < 0 || d->plane_offset[c] % 256 || d->plane_offset[c] > workspace_bytes ||
                        g.plane_bytes[c] > workspace_bytes - d->plane_offset[c]))
      return "component plane leaves the workspace";
  }
  if (d->idct_groups != g.idct_groups || d->rgb_groups != g.rgb_groups) return "workgroup counts do not fit the size";
  if (d->coef_count != g.coef_count || d->coef_offset < 0 || d->coef_offset % 64 || d->coef_offset > coef_count ||
      g.coef_count > coef_count - d->coef_offset)
    return "coefficients leave the buffer";
  if (d->out_offset < 0 || d->out_offset % 256 || d->out_offset > out_bytes || g.out_bytes > out_bytes - d->out_offset)
    return "image leaves the output buffer";
  return nullptr;
}
