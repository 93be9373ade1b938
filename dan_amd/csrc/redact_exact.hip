// Face redaction (include/danhip.h, "Face redaction"), compiled with -ffp-contract=off: every detection of every image of a ragged list
// blurred, pixelated or filled, out of place, in THREE launches, nothing read back, no atomics, integers only.
//   * redact_select : ONE workgroup of 1024 lanes loops over the n_images * rows_per_image slots, 1024 at a time (face_chips_select's
//                     scheme), applies face_rect.h's rectangle rule and redact_walk.h's extent, and writes per valid slot, in (image, row)
//                     order, a table row (image, row, x1, y1, x2, y2, e, 0) and first[k] = the work items of the rows before it (64-bit).
//                     Both running numbers come from an exclusive scan inside the workgroup: lane 0 of each wave scans its 64 entries in
//                     LDS, the 16 wave totals are added by every lane.  *count = valid rows, *total = work items.
//   * redact_copy   : every row of every image, source to destination: dwords where the destination is 4-byte aligned and the source
//                     has the same phase, bytes at the ragged ends and for a source of another phase.
//   * ONE work launch of the mode.  Workgroups of 256 lanes stride over the work items; an item finds its rectangle by a binary search
//     of first[] (uniform, scalar loads).  Per item the later valid rectangles of the same image that meet the item's tile are listed in
//     LDS (ballots and 4 wave counts; up to kLater, beyond that the table itself is walked), and a pixel is written only if it lies in
//     the row's shape and in none of theirs: every destination byte has one writer.
//       redact_blur   : item = kBand output rows x kStrip columns.  vs[] holds one uint32 vertical sum per byte column of the strip and
//                       its halo (<= (256 + 510) * 3 columns, each owned by one lane): 2e + 1 start-up rows, then per output row the
//                       entering source row is added and the leaving one subtracted, consecutive lanes on consecutive bytes.  An
//                       exclusive prefix scan of vs per channel (<= 3 columns per lane, a wave scan by shuffles, 4 wave totals in LDS)
//                       gives every pixel's window sum as a difference of two LDS reads.  One rounding, (S + A / 2) / A in uint32
//                       (S <= 255 * 511 * 511).  The work per pixel does not depend on e; what does is the start-up and the halo.
//       redact_mosaic : item = one cell: the 256 lanes sum its bytes per channel, the sums are reduced by shuffles and through LDS,
//                       every lane rounds the three means and the cell is written.
//       redact_fill   : the blur's tiles and the ownership walk alone.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "face_rect.h"
#include "redact_walk.h"

namespace {

constexpr int kSelThreads = 1024, kThreads = 256, kBand = DANHIP_REDACT_BAND, kStrip = DANHIP_REDACT_STRIP, kMaxMargin = 4000;
constexpr int kMaxGrid = 2048;                                   // 8 work workgroups per compute unit: what 19 KB of LDS each allows
constexpr int kHalo = kStrip + 2 * kRedactMaxExtent;             // columns a blur item reads: 766
constexpr int kLater = 64;                                       // later rectangles listed in LDS per item
constexpr int kEntry = 8;                                        // int32 per table row
typedef unsigned long long u64;

static_assert(kRedactMaxExtent == DANHIP_REDACT_MAX_EXTENT && kRedactBlur == DANHIP_REDACT_BLUR && kRedactMosaic == DANHIP_REDACT_MOSAIC &&
              kRedactFill == DANHIP_REDACT_FILL && kRedactRect == DANHIP_REDACT_RECT && kRedactEllipse == DANHIP_REDACT_ELLIPSE,
              "redact_walk.h and include/danhip.h state the same constants");
static_assert(kThreads * 3 >= kHalo, "a lane scans at most 3 columns of the halo");

__global__ __launch_bounds__(kSelThreads) void redact_select_kernel(const danhip_resize_item* __restrict__ images, int n_images,
                                                                    const float* __restrict__ dets, const int32_t* __restrict__ num, int rows,
                                                                    int mode, int strength_pm, int margin_pm, float threshold,
                                                                    int32_t* __restrict__ table, u64* __restrict__ first,
                                                                    u64* __restrict__ total, int32_t* __restrict__ count) {
  __shared__ u64 items_s[kSelThreads];
  __shared__ int valid_s[kSelThreads];
  __shared__ u64 wave_items[kSelThreads / 64];
  __shared__ int wave_valid[kSelThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int slots = n_images * rows;                             // <= 2^24 (the entry point checks)
  int base = 0;                                                  // valid slots before this round
  u64 item_base = 0;                                             // work items before this round
  for (int first_slot = 0; first_slot < slots; first_slot += kSelThreads) {
    const int slot = first_slot + t;
    int rect[4] = {0, 0, 0, 0};
    int image = 0, row = 0, e = 0;
    bool ok = false;
    if (slot < slots) {
      image = slot / rows;
      row = slot - image * rows;
      if (row < num[image]) {
        const float* d = dets + (size_t)slot * 5;
        ok = !(d[4] < threshold) && face_chip_rect_ex(d, images[image].H, images[image].W, margin_pm, false, false, rect);
      }
    }
    u64 items = 0;
    if (ok) {
      e = redact_extent(rect[2] - rect[0] + 1, rect[3] - rect[1] + 1, strength_pm);
      items = (u64)redact_item_count(mode, rect, e, kBand, kStrip);
    }
    valid_s[t] = ok ? 1 : 0;
    items_s[t] = items;
    __syncthreads();
    if (lane == 0) {                                             // exclusive scan of this wave's 64 entries, in place
      int v = 0;
      u64 it = 0;
      for (int j = wave * 64; j < wave * 64 + 64; ++j) {
        const int a = valid_s[j];
        const u64 b = items_s[j];
        valid_s[j] = v; items_s[j] = it;
        v += a; it += b;
      }
      wave_valid[wave] = v; wave_items[wave] = it;
    }
    __syncthreads();
    int before = 0, round_valid = 0;
    u64 items_before = 0, round_items = 0;
#pragma unroll
    for (int j = 0; j < kSelThreads / 64; ++j) {
      const int v = wave_valid[j];
      const u64 it = wave_items[j];
      before += j < wave ? v : 0; items_before += j < wave ? it : 0;
      round_valid += v; round_items += it;
    }
    if (ok) {
      const int index = base + before + valid_s[t];              // < slots: the table has room for every slot
      int32_t* o = table + (size_t)index * kEntry;
      o[0] = image; o[1] = row; o[2] = rect[0]; o[3] = rect[1]; o[4] = rect[2]; o[5] = rect[3]; o[6] = e; o[7] = 0;
      first[index] = item_base + items_before + items_s[t];
    }
    base += round_valid;
    item_base += round_items;
    __syncthreads();                                             // the LDS arrays are rewritten in the next round
  }
  if (t == 0) { *count = base; *total = item_base; }
}

__global__ __launch_bounds__(kThreads) void redact_copy_kernel(const danhip_resize_item* __restrict__ images,
                                                               const danhip_resize_item* __restrict__ dst_items, int n_images,
                                                               const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
  const int t = threadIdx.x;
  for (int image = blockIdx.y; image < n_images; image += gridDim.y) {
    const int H = images[image].H, rb = 3 * images[image].W;
    const long pitch = images[image].pitch, dpitch = dst_items[image].pitch;
    const uint8_t* s0 = src + images[image].src_offset;
    uint8_t* d0 = dst + dst_items[image].src_offset;
    for (int y = blockIdx.x; y < H; y += gridDim.x) {
      const uint8_t* s = s0 + (long)y * pitch;
      uint8_t* d = d0 + (long)y * dpitch;
      int head = (int)((4u - ((uintptr_t)d & 3u)) & 3u);         // bytes in front of the first aligned destination dword
      head = head < rb ? head : rb;
      const int nw = (rb - head) / 4, tail = rb - head - 4 * nw;
      if (t < head) d[t] = s[t];
      if (t < tail) d[head + 4 * nw + t] = s[head + 4 * nw + t];
      const uint8_t* sb = s + head;
      uint32_t* dw = (uint32_t*)(d + head);
      if (((uintptr_t)sb & 3u) == 0) {
        const uint32_t* sw = (const uint32_t*)sb;
        for (int i = t; i < nw; i += kThreads) dw[i] = sw[i];
      } else {                                                   // the source row has another phase: bytes in, dwords out
        for (int i = t; i < nw; i += kThreads) {
          const uint8_t* p = sb + 4 * i;
          dw[i] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
      }
    }
  }
}

// the table row that owns work item `item`: the largest k of 0 .. n-1 with first[k] <= item (first[] ascends strictly: a row has >= 1 item)
__device__ __forceinline__ int redact_find(const u64* __restrict__ first, int n, u64 item) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (first[mid] <= item) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The later rows of row k's image whose rectangle meets `tile`, listed in LDS.  later[4 * i ..] = rectangle i of min(n_later, kLater);
// n_later > kLater: the list is not whole and `covered` walks table rows k+1 .. end-1 (the rows of the same image) instead.
struct later_rows {
  int n_later, end;
};

__device__ __forceinline__ later_rows redact_list_later(const int32_t* __restrict__ table, int n, int k, const int* tile, int* later,
                                                        int* wave_cnt) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int image = table[(size_t)k * kEntry];
  later_rows out = {0, k + 1};
  for (int j0 = k + 1;; j0 += kThreads) {
    const int j = j0 + t;
    int r[4] = {0, 0, 0, 0};
    bool same = false, hit = false;
    if (j < n) {
      const int32_t* g = table + (size_t)j * kEntry;
      same = g[0] == image;                                      // the table ascends in (image, row): once false, false for the rest
      if (same) {
        r[0] = g[2]; r[1] = g[3]; r[2] = g[4]; r[3] = g[5];
        hit = r[0] <= tile[2] && r[2] >= tile[0] && r[1] <= tile[3] && r[3] >= tile[1];
      }
    }
    const u64 mh = __ballot(hit), ms = __ballot(same);
    if (lane == 0) { wave_cnt[wave] = __popcll(mh); wave_cnt[4 + wave] = __popcll(ms); }
    __syncthreads();
    int before = 0, hits = 0, sames = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      before += w < wave ? wave_cnt[w] : 0;
      hits += wave_cnt[w];
      sames += wave_cnt[4 + w];
    }
    const int pos = out.n_later + before + __popcll(mh & ((1ull << lane) - 1ull));
    if (hit && pos < kLater) { later[4 * pos] = r[0]; later[4 * pos + 1] = r[1]; later[4 * pos + 2] = r[2]; later[4 * pos + 3] = r[3]; }
    out.n_later += hits;
    out.end += sames;
    __syncthreads();                                             // the list is whole; wave_cnt is rewritten in the next round
    if (sames < kThreads) break;                                 // uniform: a row of another image, or the table's end, was met
  }
  return out;
}

__device__ __forceinline__ bool redact_covered(const int32_t* __restrict__ table, int k, later_rows l, const int* later, int shape, int px,
                                               int py) {
  if (l.n_later <= kLater) {
    for (int i = 0; i < l.n_later; ++i)
      if (redact_in_shape(shape, later + 4 * i, px, py)) return true;
    return false;
  }
  for (int j = k + 1; j < l.end; ++j) {                          // uniform addresses
    const int32_t* g = table + (size_t)j * kEntry;
    const int r[4] = {g[2], g[3], g[4], g[5]};
    if (redact_in_shape(shape, r, px, py)) return true;
  }
  return false;
}

__global__ __launch_bounds__(kThreads) void redact_blur_kernel(const danhip_resize_item* __restrict__ images,
                                                               const danhip_resize_item* __restrict__ dst_items,
                                                               const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               const int32_t* __restrict__ table, const u64* __restrict__ first,
                                                               const u64* __restrict__ total_p, const int32_t* __restrict__ count_p, int shape) {
  __shared__ uint32_t vs[kHalo * 3];                             // vertical window sums per byte column: 9192 bytes
  __shared__ uint32_t pre[(kHalo + 1) * 3];                      // their exclusive prefix per channel: 9204 bytes
  __shared__ uint32_t wave_tot[(kThreads / 64) * 3];
  __shared__ int later[kLater * 4];
  __shared__ int wave_cnt[8];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = *count_p;
  const u64 total = *total_p;
  for (u64 item = blockIdx.x; item < total; item += gridDim.x) {
    const int k = redact_find(first, n, item);
    const int32_t* g = table + (size_t)k * kEntry;               // uniform per workgroup
    const int rect[4] = {g[2], g[3], g[4], g[5]};
    const int e = g[6];
    const danhip_resize_item* im = images + g[0];
    const int H = im->H, W = im->W;
    const long pitch = im->pitch, dpitch = dst_items[g[0]].pitch;
    uint8_t* dimg = dst + dst_items[g[0]].src_offset;
    int tile[4], s[4];
    redact_tile(H, W, rect, e, kBand, kStrip, (int64_t)(item - first[k]), tile, s);
    const later_rows l = redact_list_later(table, n, k, tile, later, wave_cnt);
    const int nh = s[2] - s[0] + 1, nb = nh * 3;                 // columns read (<= kHalo) and their bytes
    const uint8_t* sbase = src + im->src_offset + (long)s[0] * 3;
    int wlo, whi;
    redact_grow(tile[1], tile[1], e, H, &wlo, &whi);             // the first output row's window rows: the start-up
    for (int b = t; b < nb; b += kThreads) {                     // lane t owns byte columns t, t + 256, ...
      uint32_t a = 0;
      for (int y = wlo; y <= whi; ++y) a += sbase[(long)y * pitch + b];
      vs[b] = a;
    }
    const int cpt = (nh + kThreads - 1) / kThreads;              // columns a lane scans: 1 .. 3
    const int j0 = t * cpt < nh ? t * cpt : nh, j1 = j0 + cpt < nh ? j0 + cpt : nh;
    const int ncols = tile[2] - tile[0] + 1;
    for (int py = tile[1]; py <= tile[3]; ++py) {
      if (py > tile[1]) {
        const int enter = py + e, leave = py - e - 1;            // rows of the image or outside it
        for (int b = t; b < nb; b += kThreads) {
          uint32_t v = vs[b];
          if (enter < H) v += sbase[(long)enter * pitch + b];
          if (leave >= 0) v -= sbase[(long)leave * pitch + b];
          vs[b] = v;
        }
      }
      __syncthreads();                                           // vs is whole; the previous row's reads of pre are done
      uint32_t own[3] = {0u, 0u, 0u};
      for (int j = j0; j < j1; ++j) { own[0] += vs[3 * j]; own[1] += vs[3 * j + 1]; own[2] += vs[3 * j + 2]; }
      uint32_t inc[3] = {own[0], own[1], own[2]};
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const uint32_t u = __shfl_up(inc[c], d);
          if (lane >= d) inc[c] += u;
        }
      }
      if (lane == 63) { wave_tot[3 * wave] = inc[0]; wave_tot[3 * wave + 1] = inc[1]; wave_tot[3 * wave + 2] = inc[2]; }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint32_t x = inc[c] - own[c];
        for (int w = 0; w < wave; ++w) x += wave_tot[3 * w + c];
        for (int j = j0; j < j1; ++j) { pre[3 * j + c] = x; x += vs[3 * j + c]; }
        if (j0 < nh && j1 == nh) pre[3 * nh + c] = x;            // the lane of the last column writes the total
      }
      __syncthreads();
      int ylo, yhi;
      redact_grow(py, py, e, H, &ylo, &yhi);
      const uint32_t rows_in = (uint32_t)(yhi - ylo + 1);
      for (int ob = t; ob < ncols * 3; ob += kThreads) {
        const int q = ob / 3, c = ob - 3 * q, px = tile[0] + q;
        if (!redact_in_shape(shape, rect, px, py) || redact_covered(table, k, l, later, shape, px, py)) continue;
        int lo, hi;
        redact_grow(px, px, e, W, &lo, &hi);
        const uint32_t S = pre[3 * (hi + 1 - s[0]) + c] - pre[3 * (lo - s[0]) + c];
        const uint32_t A = (uint32_t)(hi - lo + 1) * rows_in;
        dimg[(long)py * dpitch + (long)px * 3 + c] = (uint8_t)((S + A / 2u) / A);
      }
    }
    __syncthreads();                                             // the list and the sums are rewritten by the next item
  }
}

__global__ __launch_bounds__(kThreads) void redact_mosaic_kernel(const danhip_resize_item* __restrict__ images,
                                                                 const danhip_resize_item* __restrict__ dst_items,
                                                                 const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                 const int32_t* __restrict__ table, const u64* __restrict__ first,
                                                                 const u64* __restrict__ total_p, const int32_t* __restrict__ count_p, int shape) {
  __shared__ uint32_t wave_tot[(kThreads / 64) * 3];
  __shared__ int later[kLater * 4];
  __shared__ int wave_cnt[8];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n = *count_p;
  const u64 total = *total_p;
  for (u64 item = blockIdx.x; item < total; item += gridDim.x) {
    const int k = redact_find(first, n, item);
    const int32_t* g = table + (size_t)k * kEntry;
    const int rect[4] = {g[2], g[3], g[4], g[5]};
    const danhip_resize_item* im = images + g[0];
    const long pitch = im->pitch, dpitch = dst_items[g[0]].pitch;
    uint8_t* dimg = dst + dst_items[g[0]].src_offset;
    int cell[4];
    redact_cell(rect, redact_cell_side(g[6]), (int64_t)(item - first[k]), cell);
    const later_rows l = redact_list_later(table, n, k, cell, later, wave_cnt);
    const int cw = cell[2] - cell[0] + 1, ch = cell[3] - cell[1] + 1, rb = cw * 3;      // <= 255 x 255: 195075 bytes
    const uint8_t* corner = src + im->src_offset + (long)cell[1] * pitch + (long)cell[0] * 3;
    uint32_t a[3] = {0u, 0u, 0u};                                // <= 255 * 65025 per channel
    for (int idx = t; idx < ch * rb; idx += kThreads) {          // consecutive lanes, consecutive bytes of a cell row
      const int r = idx / rb, b = idx - r * rb, c = b % 3;
      const uint32_t v = corner[(long)r * pitch + b];
      a[0] += c == 0 ? v : 0u; a[1] += c == 1 ? v : 0u; a[2] += c == 2 ? v : 0u;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c] += __shfl_down(a[c], d);
    }
    if (lane == 0) { wave_tot[3 * wave] = a[0]; wave_tot[3 * wave + 1] = a[1]; wave_tot[3 * wave + 2] = a[2]; }
    __syncthreads();
    const uint32_t A = (uint32_t)(cw * ch);
    uint8_t mean[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t S = 0;
      for (int w = 0; w < kThreads / 64; ++w) S += wave_tot[3 * w + c];
      mean[c] = (uint8_t)((S + A / 2u) / A);
    }
    for (int idx = t; idx < cw * ch; idx += kThreads) {
      const int qy = idx / cw, px = cell[0] + idx - qy * cw, py = cell[1] + qy;
      if (!redact_in_shape(shape, rect, px, py) || redact_covered(table, k, l, later, shape, px, py)) continue;
      uint8_t* o = dimg + (long)py * dpitch + (long)px * 3;
      o[0] = mean[0]; o[1] = mean[1]; o[2] = mean[2];
    }
    __syncthreads();                                             // the list and the wave sums are rewritten by the next item
  }
}

__global__ __launch_bounds__(kThreads) void redact_fill_kernel(const danhip_resize_item* __restrict__ images,
                                                               const danhip_resize_item* __restrict__ dst_items, uint8_t* __restrict__ dst,
                                                               const int32_t* __restrict__ table, const u64* __restrict__ first,
                                                               const u64* __restrict__ total_p, const int32_t* __restrict__ count_p, int shape,
                                                               uint32_t fill) {
  __shared__ int later[kLater * 4];
  __shared__ int wave_cnt[8];
  const int t = threadIdx.x;
  const int n = *count_p;
  const u64 total = *total_p;
  for (u64 item = blockIdx.x; item < total; item += gridDim.x) {
    const int k = redact_find(first, n, item);
    const int32_t* g = table + (size_t)k * kEntry;
    const int rect[4] = {g[2], g[3], g[4], g[5]};
    const danhip_resize_item* im = images + g[0];
    const long dpitch = dst_items[g[0]].pitch;
    uint8_t* dimg = dst + dst_items[g[0]].src_offset;
    int tile[4], s[4];
    redact_tile(im->H, im->W, rect, g[6], kBand, kStrip, (int64_t)(item - first[k]), tile, s);
    const later_rows l = redact_list_later(table, n, k, tile, later, wave_cnt);
    const int tw = tile[2] - tile[0] + 1, th = tile[3] - tile[1] + 1;
    for (int idx = t; idx < tw * th; idx += kThreads) {
      const int qy = idx / tw, px = tile[0] + idx - qy * tw, py = tile[1] + qy;
      if (!redact_in_shape(shape, rect, px, py) || redact_covered(table, k, l, later, shape, px, py)) continue;
      uint8_t* o = dimg + (long)py * dpitch + (long)px * 3;
      o[0] = (uint8_t)(fill & 255u); o[1] = (uint8_t)((fill >> 8) & 255u); o[2] = (uint8_t)((fill >> 16) & 255u);
    }
    __syncthreads();                                             // the list is rewritten by the next item
  }
}

bool rect_ok(const int32_t* rect) {
  return rect && rect[0] >= 0 && rect[1] >= 0 && rect[2] >= rect[0] && rect[3] >= rect[1] && rect[2] - rect[0] < DANHIP_FACE_CHIPS_MAX_SIDE &&
         rect[3] - rect[1] < DANHIP_FACE_CHIPS_MAX_SIDE;
}

struct span {
  int64_t lo, hi;                                                // [lo, hi) in bytes
  int image;
};

}  // namespace

extern "C" int danhip_redact_workspace(int32_t n_images, int32_t rows_per_image, size_t* bytes) {
  DH_REQUIRE(bytes, DANHIP_EINVAL, "redact_workspace: NULL bytes");
  DH_REQUIRE(n_images >= 0 && rows_per_image >= 0 && (int64_t)n_images * rows_per_image <= (1 << 24), DANHIP_EINVAL,
             "redact_workspace: n_images %d x rows_per_image %d outside 0 .. 2^24 slots", n_images, rows_per_image);
  const size_t slots = (size_t)n_images * (size_t)rows_per_image;
  *bytes = 16 + slots * (8 + 4 * kEntry);                        // the item total, first[slots] (64-bit), the table
  return DANHIP_OK;
}

extern "C" int danhip_redact_u8(const danhip_resize_item* images_host, const danhip_resize_item* images_dev, int32_t n_images,
                                const uint8_t* src, int64_t src_bytes, const float* dets, const int32_t* num, int32_t rows_per_image,
                                int32_t mode, int32_t shape, int32_t strength_pm, int32_t margin_pm, float score_threshold,
                                const uint8_t fill_rgb[3], const danhip_resize_item* dst_items_host, const danhip_resize_item* dst_items_dev,
                                uint8_t* dst, int64_t dst_bytes, int32_t* count_out, void* workspace, size_t workspace_bytes, void* stream) {
  DH_REQUIRE(mode == DANHIP_REDACT_BLUR || mode == DANHIP_REDACT_MOSAIC || mode == DANHIP_REDACT_FILL, DANHIP_EINVAL,
             "redact_u8: mode %d is not 0 (blur), 1 (mosaic) or 2 (fill)", mode);
  DH_REQUIRE(shape == DANHIP_REDACT_RECT || shape == DANHIP_REDACT_ELLIPSE, DANHIP_EINVAL, "redact_u8: shape %d is neither 0 (rect) nor 1 (ellipse)",
             shape);
  DH_REQUIRE(strength_pm >= 1 && strength_pm <= 1000, DANHIP_EINVAL, "redact_u8: strength_pm %d outside 1 .. 1000", strength_pm);
  DH_REQUIRE(margin_pm >= 0 && margin_pm <= kMaxMargin, DANHIP_EINVAL, "redact_u8: margin_pm %d outside 0 .. %d", margin_pm, kMaxMargin);
  DH_REQUIRE(!std::isnan(score_threshold), DANHIP_EINVAL, "redact_u8: score_threshold is NaN");
  size_t need = 0;
  if (danhip_redact_workspace(n_images, rows_per_image, &need) != DANHIP_OK) return DANHIP_EINVAL;
  DH_REQUIRE(fill_rgb, DANHIP_EINVAL, "redact_u8: NULL fill_rgb");
  DH_REQUIRE(count_out, DANHIP_EINVAL, "redact_u8: NULL count_out");
  if (n_images == 0) return DANHIP_OK;
  DH_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7u) == 0, DANHIP_EINVAL,
             "redact_u8: workspace of %zu bytes, %zu needed at an 8-byte aligned address", workspace_bytes, need);
  DH_REQUIRE(images_host && images_dev && src && dst_items_host && dst_items_dev && dst, DANHIP_EINVAL,
             "redact_u8: NULL images / src / dst_items / dst");
  DH_REQUIRE(rows_per_image == 0 || (dets && num), DANHIP_EINVAL, "redact_u8: NULL dets / num");
  std::vector<span> from((size_t)n_images), to((size_t)n_images);
  for (int32_t i = 0; i < n_images; ++i) {
    const danhip_resize_item& it = images_host[i];
    const danhip_resize_item& ot = dst_items_host[i];
    DH_REQUIRE(it.H >= 1 && it.W >= 1 && (int64_t)it.pitch >= 3 * (int64_t)it.W && it.src_offset >= 0, DANHIP_EINVAL,
               "redact_u8: image %d: a non-positive size, pitch below 3 * W or a negative offset", i);
    const int64_t bytes = (int64_t)(it.H - 1) * it.pitch + 3 * (int64_t)it.W;
    DH_REQUIRE(it.src_offset <= src_bytes - bytes, DANHIP_EINVAL, "redact_u8: image %d reads past the source buffer", i);
    DH_REQUIRE(ot.H == it.H && ot.W == it.W, DANHIP_EINVAL, "redact_u8: destination %d is %d x %d, its source %d x %d", i, ot.H, ot.W, it.H,
               it.W);
    DH_REQUIRE((int64_t)ot.pitch >= 3 * (int64_t)ot.W && ot.src_offset >= 0, DANHIP_EINVAL,
               "redact_u8: destination %d: pitch below 3 * W or a negative offset", i);
    const int64_t out_bytes = (int64_t)(ot.H - 1) * ot.pitch + 3 * (int64_t)ot.W;
    DH_REQUIRE(ot.src_offset <= dst_bytes - out_bytes, DANHIP_EINVAL, "redact_u8: destination %d writes past the destination buffer", i);
    from[i] = {(int64_t)(uintptr_t)src + it.src_offset, (int64_t)(uintptr_t)src + it.src_offset + bytes, i};
    to[i] = {(int64_t)(uintptr_t)dst + ot.src_offset, (int64_t)(uintptr_t)dst + ot.src_offset + out_bytes, i};
  }
  const auto by_lo = [](const span& a, const span& b) { return a.lo < b.lo; };
  std::sort(to.begin(), to.end(), by_lo);
  for (size_t i = 1; i < to.size(); ++i)
    DH_REQUIRE(to[i - 1].hi <= to[i].lo, DANHIP_EINVAL, "redact_u8: destinations %d and %d overlap", to[i - 1].image, to[i].image);
  std::sort(from.begin(), from.end(), by_lo);
  for (size_t i = 0, j = 0; i < from.size(); ++i) {              // sources may overlap one another; destinations are disjoint and sorted
    while (j > 0 && to[j - 1].hi > from[i].lo) --j;
    while (j < to.size() && to[j].hi <= from[i].lo) ++j;
    DH_REQUIRE(j == to.size() || to[j].lo >= from[i].hi, DANHIP_EINVAL, "redact_u8: destination %d overlaps source image %d",
               j < to.size() ? to[j].image : -1, from[i].image);
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t slots = (size_t)n_images * (size_t)rows_per_image;
  u64* total = (u64*)workspace;
  u64* first = (u64*)((char*)workspace + 16);
  int32_t* table = (int32_t*)((char*)workspace + 16 + 8 * slots);
  hipLaunchKernelGGL(redact_select_kernel, dim3(1), dim3(kSelThreads), 0, s, images_dev, (int)n_images, dets, num, (int)rows_per_image, (int)mode,
                     (int)strength_pm, (int)margin_pm, score_threshold, table, first, total, count_out);
  DH_LAUNCH_CHECK();
  const int gy = n_images < 256 ? n_images : 256, gx = kMaxGrid / gy;
  hipLaunchKernelGGL(redact_copy_kernel, dim3(gx, gy), dim3(kThreads), 0, s, images_dev, dst_items_dev, (int)n_images, src, dst);
  DH_LAUNCH_CHECK();
  const int grid = slots == 0 ? 1 : kMaxGrid;                    // the item total is known on the device only
  if (mode == DANHIP_REDACT_BLUR)
    hipLaunchKernelGGL(redact_blur_kernel, dim3(grid), dim3(kThreads), 0, s, images_dev, dst_items_dev, src, dst, table, first, total, count_out,
                       (int)shape);
  else if (mode == DANHIP_REDACT_MOSAIC)
    hipLaunchKernelGGL(redact_mosaic_kernel, dim3(grid), dim3(kThreads), 0, s, images_dev, dst_items_dev, src, dst, table, first, total,
                       count_out, (int)shape);
  else
    hipLaunchKernelGGL(redact_fill_kernel, dim3(grid), dim3(kThreads), 0, s, images_dev, dst_items_dev, dst, table, first, total, count_out,
                       (int)shape, (uint32_t)fill_rgb[0] | ((uint32_t)fill_rgb[1] << 8) | ((uint32_t)fill_rgb[2] << 16));
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

// ------------------------------------------------------------------------------------------------ the walk's arithmetic for the host
extern "C" int danhip_redact_extent(int32_t wc, int32_t hc, int32_t strength_pm) {
  DH_REQUIRE(wc >= 1 && hc >= 1 && wc <= DANHIP_FACE_CHIPS_MAX_SIDE && hc <= DANHIP_FACE_CHIPS_MAX_SIDE && strength_pm >= 1 && strength_pm <= 1000,
             DANHIP_EINVAL, "redact_extent: sides %d x %d outside 1 .. %d or strength_pm %d outside 1 .. 1000", wc, hc,
             DANHIP_FACE_CHIPS_MAX_SIDE, strength_pm);
  return redact_extent(wc, hc, strength_pm);
}

extern "C" int64_t danhip_redact_item_count(int32_t mode, const int32_t rect[4], int32_t e, int32_t band, int32_t strip) {
  if (!(mode >= 0 && mode <= 2 && rect_ok(rect) && e >= 1 && e <= kRedactMaxExtent && band >= 1 && strip >= 1)) {
    danhip_set_error("redact_item_count: a mode, rectangle, extent, band or strip outside the rule");
    return -1;
  }
  return redact_item_count(mode, rect, e, band, strip);
}

extern "C" int danhip_redact_tile(int32_t H, int32_t W, const int32_t rect[4], int32_t e, int32_t band, int32_t strip, int64_t item,
                                  int32_t out[8]) {
  DH_REQUIRE(out && rect_ok(rect) && rect[2] < W && rect[3] < H && e >= 1 && e <= kRedactMaxExtent && band >= 1 && strip >= 1, DANHIP_EINVAL,
             "redact_tile: a rectangle outside the image, or an extent, band or strip outside the rule");
  DH_REQUIRE(item >= 0 && item < redact_item_count(kRedactBlur, rect, e, band, strip), DANHIP_EINVAL, "redact_tile: item %lld outside the rectangle's",
             (long long)item);
  redact_tile(H, W, rect, e, band, strip, item, out, out + 4);
  return DANHIP_OK;
}

extern "C" int danhip_redact_window(int32_t H, int32_t W, int32_t e, int32_t px, int32_t py, int32_t out[5]) {
  DH_REQUIRE(out && H >= 1 && W >= 1 && e >= 1 && e <= kRedactMaxExtent && px >= 0 && px < W && py >= 0 && py < H, DANHIP_EINVAL,
             "redact_window: a pixel outside the image or an extent outside 1 .. %d", kRedactMaxExtent);
  redact_grow(px, px, e, W, &out[0], &out[2]);
  redact_grow(py, py, e, H, &out[1], &out[3]);
  out[4] = (out[2] - out[0] + 1) * (out[3] - out[1] + 1);
  return DANHIP_OK;
}

extern "C" int danhip_redact_cell(const int32_t rect[4], int32_t c, int64_t cell, int32_t out[5]) {
  DH_REQUIRE(out && rect_ok(rect) && c >= 2 && c <= kRedactMaxExtent, DANHIP_EINVAL, "redact_cell: a rectangle or a cell side outside the rule");
  DH_REQUIRE(cell >= 0 && cell < (int64_t)redact_units(rect[2] - rect[0] + 1, c) * redact_units(rect[3] - rect[1] + 1, c), DANHIP_EINVAL,
             "redact_cell: cell %lld outside the rectangle's", (long long)cell);
  redact_cell(rect, c, cell, out);
  out[4] = (out[2] - out[0] + 1) * (out[3] - out[1] + 1);
  return DANHIP_OK;
}

extern "C" int danhip_redact_in_shape(int32_t shape, const int32_t rect[4], int32_t px, int32_t py) {
  DH_REQUIRE((shape == DANHIP_REDACT_RECT || shape == DANHIP_REDACT_ELLIPSE) && rect_ok(rect), DANHIP_EINVAL,
             "redact_in_shape: a shape or a rectangle outside the rule");
  return redact_in_shape(shape, rect, px, py) ? 1 : 0;
}
