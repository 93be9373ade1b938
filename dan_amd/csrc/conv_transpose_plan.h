// Host planning of the transposed convolution 4x4 / stride 2 (conv_transpose.hip): shape checks, the weight gradient's slab split and its
// workspace layout.  Plain C++ with no device code, so that a stand-alone program can run it under the host sanitizers
// (tools/conv_transpose_plan_asan.cpp).  Every number here is a function of the call's shape alone - never of the device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define CT_BM 128          /* rows (pixels) of a forward / data-gradient tile */
#define CT_BN 64           /* columns (output channels of the product) of every tile */
#define CT_BK 64           /* K step: 64 channels (forward, data gradient) or 64 pixels (weight gradient) */
#define CT_WG_TARGET_BLOCKS 1024   /* the weight gradient splits its pixels until it has about this many workgroups ... */
#define CT_WG_MIN_STEPS 2          /* ... but a slab never gets fewer K steps than this */
#define CT_WG_MAX_SLABS 64         /* ... and never more slabs than the ordered reduction sums sequentially (DANHIP_ORDERED_REDUCE_SEQ_MAX) */
#define CT_DB_MAX_ROWS 512         /* partial rows of the bias gradient */
#define CT_DB_PIXELS_PER_ROW 64    /* at least this many output pixels per partial row */

// 0 = supported; else a message (static string).  Channels: multiples of 64 up to 1024; Ho in {2 Hi - 1, 2 Hi}, Wo likewise; pixel counts
// that 32-bit row indices hold (element offsets are computed in 64 bits).
static inline const char* ct_shape_error(int64_t N, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo, int64_t Cin, int64_t Cout) {
  if (N < 1 || Hi < 1 || Wi < 1) return "N, Hi, Wi must be positive";
  if (Cin < 64 || Cin > 1024 || Cin % 64 != 0 || Cout < 64 || Cout > 1024 || Cout % 64 != 0) return "unsupported channel count (Cin and Cout: multiples of 64 up to 1024)";
  if (!(Ho == 2 * Hi || Ho == 2 * Hi - 1) || !(Wo == 2 * Wi || Wo == 2 * Wi - 1)) return "Ho / Wo must be 2 Hi / 2 Wi or one less (the top-left crop)";
  if (N * Hi * Wi >= ((int64_t)1 << 31) / 4 || N * Ho * Wo >= ((int64_t)1 << 31)) return "more pixels than 32-bit row indices hold";
  return 0;
}

struct CtWgradPlan {
  int64_t pixels;          // N Hi Wi: length of the reduction
  int steps;               // ceil(pixels / CT_BK)
  int tiles;               // 16 taps x (Cout / 64) x (Cin / 64) workgroups per slab
  int slabs;               // partial sums of dW, each over steps_per_slab K steps (the last one may be shorter, never empty)
  int steps_per_slab;
  int64_t dw_elems;        // 16 Cout Cin
  int db_rows;             // partial rows of db, each over db_pixels output pixels (the last one may be shorter, never empty)
  int64_t db_pixels;
  size_t db_off;           // byte offset of the [db_rows][Cout] rows behind the [slabs][dw_elems] slabs
  size_t bytes;
};

static inline CtWgradPlan ct_wgrad_plan(int64_t N, int64_t Hi, int64_t Wi, int64_t Ho, int64_t Wo, int64_t Cin, int64_t Cout) {
  CtWgradPlan p;
  p.pixels = N * Hi * Wi;
  p.steps = (int)((p.pixels + CT_BK - 1) / CT_BK);
  p.tiles = (int)(16 * (Cout / CT_BN) * (Cin / CT_BN));
  int want = (CT_WG_TARGET_BLOCKS + p.tiles - 1) / p.tiles;
  const int most = (p.steps + CT_WG_MIN_STEPS - 1) / CT_WG_MIN_STEPS;
  if (want > most) want = most;
  if (want > CT_WG_MAX_SLABS) want = CT_WG_MAX_SLABS;
  if (want < 1) want = 1;
  p.steps_per_slab = (p.steps + want - 1) / want;
  p.slabs = (p.steps + p.steps_per_slab - 1) / p.steps_per_slab;
  p.dw_elems = 16 * Cout * Cin;
  const int64_t out_pixels = N * Ho * Wo;
  int64_t rows = (out_pixels + CT_DB_PIXELS_PER_ROW - 1) / CT_DB_PIXELS_PER_ROW;
  if (rows > CT_DB_MAX_ROWS) rows = CT_DB_MAX_ROWS;
  p.db_pixels = (out_pixels + rows - 1) / rows;
  p.db_rows = (int)((out_pixels + p.db_pixels - 1) / p.db_pixels);
  p.db_off = (size_t)p.slabs * (size_t)p.dw_elems * sizeof(float);
  p.bytes = p.db_off + (size_t)p.db_rows * (size_t)Cout * sizeof(float);
  return p;
}
