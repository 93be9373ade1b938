// Face chips (include/danhip.h, "Face chips"), compiled with -ffp-contract=off: every detection of every image of a ragged list cropped
// and resized to S x S in TWO launches, nothing read back.
//   * face_chips_select : ONE workgroup of 1024 lanes loops over the n_images * rows_per_image slots, 1024 at a time, applies the
//                         rectangle rule (face_rect.h's face_chip_rect: integers only, 64-bit intermediates) and numbers the valid slots in
//                         (image, row) order by an exclusive prefix sum (wave ballots + 16 wave totals in LDS + a running base).  A single
//                         looping workgroup instead of chained ones: slot counts are a few thousand (8 images x 750 rows = 6 rounds), the
//                         order then needs no counter in memory, no spinning on another workgroup and no atomics, and a 0-byte workspace.
//                         It writes chip_src rows of the first max_chips valid slots and the TRUE total to *count.
//   * face_chips_resize : workgroups walk (chip, tile) items, a tile = 256 runs of 4 consecutive output pixels of one row (12 bytes per lane,
//                         three dword stores where the run is whole and its address 4-byte aligned, single bytes otherwise), and leave at
//                         chip >= min(*count, max_chips).  The pixel arithmetic is resize_u8.h's with the crop's top-left byte as the source,
//                         the image's pitch, the crop's size and scale = crop / S in double.  The chip's geometry is uniform per workgroup
//                         (scalar loads); per lane there are only dy, dx and the 12 result bytes.  No LDS, no atomics.
// danhip_face_chips_u8_ex (zero-padded rectangles, area downscale) adds three kernels and leaves the two above as they are:
//   * face_chips_select_ex : the select launch with the extended rectangle rule (pad: the unclipped rectangle; the side cap).
//   * face_chips_resize_fetch : the resize launch for filter LINEAR with pad: the same items and stores, resize_u8.h's arithmetic through a
//                         fetch that answers the fill colour outside the image.  (LINEAR without pad launches face_chips_resize itself.)
//   * face_chips_area   : filter AREA, integers only.  Workgroups walk (chip, output row, 256 output columns) items.  Per item the source
//                         rows of the output row are taken in bands of up to 8 rows and pieces of up to 4096 pixels: a piece is copied to
//                         LDS with consecutive lanes on consecutive bytes (fill outside the image), each (row, output column) owner lane
//                         adds its weighted span of the piece to an exact uint32 horizontal sum in LDS (<= 255 * 32768 < 2^23), and once
//                         a band is whole every lane adds weight * sum of up to 3 (column, channel) outputs into 64-bit registers.  One
//                         rounding, (sum + D / 2) / D with D = Dx * Dy <= 2^30, at the store.  36 KB of LDS, no atomics, no floats.
#include <cmath>

#include "common.h"
#include "face_rect.h"
#include "resize_u8.h"

namespace {

constexpr int kSelThreads = 1024, kRun = 4, kTileThreads = 256, kMaxS = 1024, kMaxMargin = 4000, kMaxGrid = 1024;     // 4 resize workgroups per compute unit
constexpr int kAreaThreads = 256, kAreaCols = 256, kAreaRows = 8, kAreaPiece = 4096;     // face_chips_area: output columns per item, band rows, piece pixels

__global__ __launch_bounds__(kSelThreads) void face_chips_select_kernel(const danhip_resize_item* __restrict__ images, int n_images,
                                                                        const float* __restrict__ dets, const int32_t* __restrict__ num,
                                                                        int rows, int margin_pm, int square, float threshold,
                                                                        int32_t* __restrict__ chip_src, int32_t* __restrict__ count, int max_chips) {
  __shared__ int wave_total[kSelThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int slots = n_images * rows;                             // < 2^24 (the entry point checks)
  int base = 0;                                                  // valid slots before this round
  for (int first = 0; first < slots; first += kSelThreads) {
    const int slot = first + t;
    int rect[4] = {0, 0, 0, 0};
    int image = 0, row = 0;
    bool ok = false;
    if (slot < slots) {
      image = slot / rows;
      row = slot - image * rows;
      if (row < num[image]) {
        const float* d = dets + (size_t)slot * 5;
        ok = !(d[4] < threshold) && face_chip_rect(d, images[image].H, images[image].W, margin_pm, square != 0, rect);
      }
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < kSelThreads / 64; ++j) {
      const int v = wave_total[j];
      before += j < wave ? v : 0;
      total += v;
    }
    const int index = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (ok && index < max_chips) {
      int32_t* o = chip_src + (size_t)index * 6;
      o[0] = image; o[1] = row; o[2] = rect[0]; o[3] = rect[1]; o[4] = rect[2]; o[5] = rect[3];
    }
    base += total;
    __syncthreads();                                             // wave_total is rewritten in the next round
  }
  if (t == 0) *count = base;
}

__global__ __launch_bounds__(kTileThreads) void face_chips_resize_kernel(const danhip_resize_item* __restrict__ images,
                                                                         const uint8_t* __restrict__ src, const int32_t* __restrict__ chip_src,
                                                                         const int32_t* __restrict__ count, int max_chips, int S,
                                                                         int runs_per_row, int tiles_per_chip, uint8_t* __restrict__ chips) {
  const int total = *count, n = total < max_chips ? total : max_chips;
  const int runs = S * runs_per_row;                             // <= 1024 * 256
  for (long item = blockIdx.x; item < (long)n * tiles_per_chip; item += gridDim.x) {
    const int chip = (int)(item / tiles_per_chip), tile = (int)(item - (long)chip * tiles_per_chip);
    const int r = tile * kTileThreads + (int)threadIdx.x;
    if (r >= runs) continue;
    const int32_t* g = chip_src + (size_t)chip * 6;              // uniform per workgroup
    const danhip_resize_item* im = images + g[0];
    const int xc1 = g[2], yc1 = g[3], cw = g[4] - xc1 + 1, ch = g[5] - yc1 + 1;
    const long pitch = im->pitch;
    const uint8_t* crop = src + im->src_offset + (long)yc1 * pitch + (long)xc1 * 3;
    const double scale_x = (double)cw / (double)S, scale_y = (double)ch / (double)S;
    const int dy = r / runs_per_row, dx0 = (r - dy * runs_per_row) * kRun;
    uint8_t px[kRun * 3];
#pragma unroll
    for (int p = 0; p < kRun; ++p) {
      const int dx = dx0 + p < S ? dx0 + p : S - 1;              // the tail repeats the last pixel; it is not stored
      resize_u8_linear_pixel(crop, pitch, ch, cw, 3, false, scale_x, scale_y, dy, dx, px + 3 * p);
    }
    uint8_t* o = chips + ((size_t)chip * S * S + (size_t)dy * S + dx0) * 3;
    if (dx0 + kRun <= S && ((uintptr_t)o & 3u) == 0) {
      uint32_t* o4 = (uint32_t*)o;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int p = 0; p < kRun; ++p)
        if (dx0 + p < S) { o[3 * p] = px[3 * p]; o[3 * p + 1] = px[3 * p + 1]; o[3 * p + 2] = px[3 * p + 2]; }
    }
  }
}

// face_chips_select_kernel with face_chip_rect_ex: the same single looping workgroup and numbering (kept apart so that the old entry
// point launches the kernel it always launched).
__global__ __launch_bounds__(kSelThreads) void face_chips_select_ex_kernel(const danhip_resize_item* __restrict__ images, int n_images,
                                                                           const float* __restrict__ dets, const int32_t* __restrict__ num,
                                                                           int rows, int margin_pm, int square, int pad, float threshold,
                                                                           int32_t* __restrict__ chip_src, int32_t* __restrict__ count,
                                                                           int max_chips) {
  __shared__ int wave_total[kSelThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int slots = n_images * rows;
  int base = 0;
  for (int first = 0; first < slots; first += kSelThreads) {
    const int slot = first + t;
    int rect[4] = {0, 0, 0, 0};
    int image = 0, row = 0;
    bool ok = false;
    if (slot < slots) {
      image = slot / rows;
      row = slot - image * rows;
      if (row < num[image]) {
        const float* d = dets + (size_t)slot * 5;
        ok = !(d[4] < threshold) && face_chip_rect_ex(d, images[image].H, images[image].W, margin_pm, square != 0, pad != 0, rect);
      }
    }
    const unsigned long long m = __ballot(ok);
    if (lane == 0) wave_total[wave] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < kSelThreads / 64; ++j) {
      const int v = wave_total[j];
      before += j < wave ? v : 0;
      total += v;
    }
    const int index = base + before + __popcll(m & ((1ull << lane) - 1ull));
    if (ok && index < max_chips) {
      int32_t* o = chip_src + (size_t)index * 6;
      o[0] = image; o[1] = row; o[2] = rect[0]; o[3] = rect[1]; o[4] = rect[2]; o[5] = rect[3];
    }
    base += total;
    __syncthreads();
  }
  if (t == 0) *count = base;
}

// face_chips_resize_kernel for a rectangle that may leave the image: the crop is the whole rectangle, a position outside the image is `fill`
// (byte c of the word = channel c).
__global__ __launch_bounds__(kTileThreads) void face_chips_resize_fetch_kernel(const danhip_resize_item* __restrict__ images,
                                                                               const uint8_t* __restrict__ src,
                                                                               const int32_t* __restrict__ chip_src,
                                                                               const int32_t* __restrict__ count, int max_chips, int S,
                                                                               int runs_per_row, int tiles_per_chip, uint32_t fill,
                                                                               uint8_t* __restrict__ chips) {
  const int total = *count, n = total < max_chips ? total : max_chips;
  const int runs = S * runs_per_row;
  for (long item = blockIdx.x; item < (long)n * tiles_per_chip; item += gridDim.x) {
    const int chip = (int)(item / tiles_per_chip), tile = (int)(item - (long)chip * tiles_per_chip);
    const int r = tile * kTileThreads + (int)threadIdx.x;
    if (r >= runs) continue;
    const int32_t* g = chip_src + (size_t)chip * 6;              // uniform per workgroup
    const danhip_resize_item* im = images + g[0];
    const int x1 = g[2], y1 = g[3], cw = g[4] - x1 + 1, ch = g[5] - y1 + 1, H = im->H, W = im->W;
    const long pitch = im->pitch;
    const uint8_t* image = src + im->src_offset;
    const auto fetch = [=](int y, int x, int c) -> int {         // (y, x) in the rectangle; |y1 + y|, |x1 + x| < 2^31 (face_chip_rect_ex)
      const int iy = y1 + y, ix = x1 + x;
      return iy >= 0 && iy < H && ix >= 0 && ix < W ? (int)image[(long)iy * pitch + (long)ix * 3 + c] : (int)((fill >> (8 * c)) & 255u);
    };
    const double scale_x = (double)cw / (double)S, scale_y = (double)ch / (double)S;
    const int dy = r / runs_per_row, dx0 = (r - dy * runs_per_row) * kRun;
    uint8_t px[kRun * 3];
#pragma unroll
    for (int p = 0; p < kRun; ++p) {
      const int dx = dx0 + p < S ? dx0 + p : S - 1;
      resize_u8_linear_pixel_fetch(fetch, ch, cw, scale_x, scale_y, dy, dx, px + 3 * p);
    }
    uint8_t* o = chips + ((size_t)chip * S * S + (size_t)dy * S + dx0) * 3;
    if (dx0 + kRun <= S && ((uintptr_t)o & 3u) == 0) {
      uint32_t* o4 = (uint32_t*)o;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int p = 0; p < kRun; ++p)
        if (dx0 + p < S) { o[3 * p] = px[3 * p]; o[3 * p + 1] = px[3 * p + 1]; o[3 * p + 2] = px[3 * p + 2]; }
    }
  }
}

// One axis of the area rule: n source positions (1 .. 32768), S outputs (1 .. 1024), output j.  Every product is below 2^26.
struct area_axis {
  int n, S, j, c0, c1, f;                                        // n <= S: the two taps c0 <= c1 and the weight f of c1
  __device__ __forceinline__ area_axis(int n_, int S_, int j_) : n(n_), S(S_), j(j_), c0(0), c1(0), f(0) {
    if (n <= S) {
      const int t = (2 * j + 1) * n - S;                         // > -S: floor(t / 2S) is -1 when t < 0
      const int i0 = t < 0 ? -1 : t / (2 * S);
      f = t - 2 * S * i0;
      c0 = i0 < 0 ? 0 : i0;                                      // i0 <= n - 1
      c1 = i0 + 1 > n - 1 ? n - 1 : i0 + 1;
    }
  }
  __device__ __forceinline__ int lo() const { return n > S ? j * n / S : c0; }                   // first position with a weight
  __device__ __forceinline__ int end() const { return n > S ? ((j + 1) * n - 1) / S + 1 : c1 + 1; }   // one past the last
  __device__ __forceinline__ int divisor() const { return n > S ? n : 2 * S; }
  __device__ __forceinline__ int weight(int i) const {
    if (n > S) {
      const int a = j * n > i * S ? j * n : i * S, b = (j + 1) * n < (i + 1) * S ? (j + 1) * n : (i + 1) * S;
      return b > a ? b - a : 0;
    }
    return (i == c0 ? 2 * S - f : 0) + (i == c1 ? f : 0);
  }
};

__global__ __launch_bounds__(kAreaThreads) void face_chips_area_kernel(const danhip_resize_item* __restrict__ images,
                                                                       const uint8_t* __restrict__ src, const int32_t* __restrict__ chip_src,
                                                                       const int32_t* __restrict__ count, int max_chips, int S, int col_tiles,
                                                                       uint32_t fill, uint8_t* __restrict__ chips) {
  __shared__ uint8_t piece[kAreaPiece * 3];                                  // rows x width <= kAreaPiece pixels: 12 KB
  __shared__ uint32_t hsum[kAreaRows * kAreaCols * 3];                       // [row][column][channel]: 24 KB
  const int t = threadIdx.x;
  const int total = *count, n_chips = total < max_chips ? total : max_chips;
  const int items_per_chip = S * col_tiles;
  for (long item = blockIdx.x; item < (long)n_chips * items_per_chip; item += gridDim.x) {
    const int chip = (int)(item / items_per_chip), rem = (int)(item - (long)chip * items_per_chip);
    const int jy = rem / col_tiles, jx0 = (rem - jy * col_tiles) * kAreaCols;
    const int ncols = S - jx0 < kAreaCols ? S - jx0 : kAreaCols;
    const int32_t* g = chip_src + (size_t)chip * 6;              // uniform per workgroup
    const danhip_resize_item* im = images + g[0];
    const int x1 = g[2], y1 = g[3], nx = g[4] - x1 + 1, ny = g[5] - y1 + 1, H = im->H, W = im->W;
    const long pitch = im->pitch;
    const uint8_t* image = src + im->src_offset;
    const area_axis ay(ny, S, jy);
    const int ylo = ay.lo(), yend = ay.end();
    const int xlo = area_axis(nx, S, jx0).lo(), xend = area_axis(nx, S, jx0 + ncols - 1).end();
    const int width = xend - xlo < kAreaPiece ? xend - xlo : kAreaPiece;       // pixels of a piece
    const int band = kAreaPiece / width < kAreaRows ? kAreaPiece / width : kAreaRows;   // rows of a band: band * width <= kAreaPiece
    unsigned long long acc[3] = {0ull, 0ull, 0ull};              // outputs t, t + 256, t + 512 of the ncols * 3 (column, channel) pairs
    for (int y0 = ylo; y0 < yend; y0 += band) {
      const int rows = yend - y0 < band ? yend - y0 : band;
      for (int w = t; w < rows * ncols; w += kAreaThreads) { hsum[3 * w] = 0u; hsum[3 * w + 1] = 0u; hsum[3 * w + 2] = 0u; }   // by its owner
      for (int xc = xlo; xc < xend; xc += width) {
        const int cw = xend - xc < width ? xend - xc : width;
        __syncthreads();                                         // the previous piece has been read
        for (int r = 0; r < rows; ++r) {
          const int iy = y1 + y0 + r;
          const bool row_in = iy >= 0 && iy < H;
          const uint8_t* line = image + (long)(row_in ? iy : 0) * pitch;
          for (int b = t; b < cw * 3; b += kAreaThreads) {       // consecutive lanes, consecutive bytes
            const int px = b / 3, c = b - 3 * px, ix = x1 + xc + px;
            piece[r * cw * 3 + b] = row_in && ix >= 0 && ix < W ? line[(long)ix * 3 + c] : (uint8_t)((fill >> (8 * c)) & 255u);
          }
        }
        __syncthreads();
        for (int w = t; w < rows * ncols; w += kAreaThreads) {   // the owner of (row r, column jx) adds its span's part of this piece
          const int r = w / ncols, jx = jx0 + (w - r * ncols);
          const area_axis ax(nx, S, jx);
          const int a = ax.lo() > xc ? ax.lo() : xc, e = ax.end() < xc + cw ? ax.end() : xc + cw;
          uint32_t s0 = 0u, s1 = 0u, s2 = 0u;
          for (int i = a; i < e; ++i) {
            const uint32_t wt = (uint32_t)ax.weight(i);
            const uint8_t* p = piece + (r * cw + (i - xc)) * 3;
            s0 += wt * p[0]; s1 += wt * p[1]; s2 += wt * p[2];
          }
          hsum[3 * w] += s0; hsum[3 * w + 1] += s1; hsum[3 * w + 2] += s2;
        }
      }
      __syncthreads();                                           // the band's sums are whole
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int o = t + k * kAreaThreads;
        if (o < ncols * 3)
          for (int r = 0; r < rows; ++r) acc[k] += (unsigned long long)ay.weight(y0 + r) * hsum[r * ncols * 3 + o];
      }
      __syncthreads();                                           // hsum is rewritten by the next band
    }
    const unsigned long long D = (unsigned long long)area_axis(nx, S, jx0).divisor() * (unsigned long long)ay.divisor();
    uint8_t* out = chips + ((size_t)chip * S * S + (size_t)jy * S + jx0) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int o = t + k * kAreaThreads;
      if (o < ncols * 3) out[o] = (uint8_t)((acc[k] + D / 2) / D);
    }
  }
}

}  // namespace

extern "C" int danhip_face_chips_workspace(int32_t n_images, int32_t rows_per_image, size_t* bytes) {
  DH_REQUIRE(bytes, DANHIP_EINVAL, "face_chips_workspace: NULL bytes");
  DH_REQUIRE(n_images >= 0 && rows_per_image >= 0 && (int64_t)n_images * rows_per_image <= (1 << 24), DANHIP_EINVAL,
             "face_chips_workspace: n_images %d x rows_per_image %d outside 0 .. 2^24 slots", n_images, rows_per_image);
  *bytes = 0;                                                    // the select launch is one looping workgroup: nothing is kept between workgroups
  return DANHIP_OK;
}

extern "C" int danhip_face_chips_u8(const danhip_resize_item* images_host, const danhip_resize_item* images_dev, int32_t n_images,
                                    const uint8_t* src, int64_t src_bytes, const float* dets, const int32_t* num, int32_t rows_per_image,
                                    int32_t S, int32_t margin_pm, int32_t square, float score_threshold, uint8_t* chips_out,
                                    int32_t* chip_src_out, int32_t* count_out, int32_t max_chips, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  DH_REQUIRE(S >= 1 && S <= kMaxS, DANHIP_EINVAL, "face_chips_u8: S %d outside 1 .. %d", S, kMaxS);
  DH_REQUIRE(margin_pm >= 0 && margin_pm <= kMaxMargin, DANHIP_EINVAL, "face_chips_u8: margin_pm %d outside 0 .. %d", margin_pm, kMaxMargin);
  DH_REQUIRE(square == 0 || square == 1, DANHIP_EINVAL, "face_chips_u8: square is 0 or 1");
  DH_REQUIRE(!std::isnan(score_threshold), DANHIP_EINVAL, "face_chips_u8: score_threshold is NaN");
  DH_REQUIRE(max_chips >= 0, DANHIP_EINVAL, "face_chips_u8: max_chips %d is negative", max_chips);
  size_t need = 0;
  if (danhip_face_chips_workspace(n_images, rows_per_image, &need) != DANHIP_OK) return DANHIP_EINVAL;
  DH_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), DANHIP_EINVAL, "face_chips_u8: workspace of %zu bytes, %zu needed",
             workspace_bytes, need);
  DH_REQUIRE(count_out, DANHIP_EINVAL, "face_chips_u8: NULL count_out");
  hipStream_t s = (hipStream_t)stream;
  if (n_images == 0 || rows_per_image == 0) return danhip_zero_async(count_out, 4, s);
  DH_REQUIRE(images_host && images_dev && src && dets && num, DANHIP_EINVAL, "face_chips_u8: NULL images / src / dets / num");
  DH_REQUIRE(max_chips == 0 || (chips_out && chip_src_out), DANHIP_EINVAL, "face_chips_u8: NULL chips_out / chip_src_out");
  for (int32_t i = 0; i < n_images; ++i) {
    const danhip_resize_item& it = images_host[i];
    DH_REQUIRE(it.H >= 1 && it.W >= 1 && (int64_t)it.pitch >= 3 * (int64_t)it.W && it.src_offset >= 0, DANHIP_EINVAL,
               "face_chips_u8: image %d: a non-positive size, pitch below 3 * W or a negative offset", i);
    DH_REQUIRE(it.src_offset + (int64_t)(it.H - 1) * it.pitch + 3 * (int64_t)it.W <= src_bytes, DANHIP_EINVAL,
               "face_chips_u8: image %d reads past the source buffer", i);
  }
  hipLaunchKernelGGL(face_chips_select_kernel, dim3(1), dim3(kSelThreads), 0, s, images_dev, (int)n_images, dets, num, (int)rows_per_image,
                     (int)margin_pm, (int)square, score_threshold, chip_src_out, count_out, (int)max_chips);
  DH_LAUNCH_CHECK();
  if (max_chips == 0) return DANHIP_OK;
  const int runs_per_row = cdiv(S, kRun), tiles_per_chip = cdiv((long)S * runs_per_row, kTileThreads);
  const int64_t cap = (int64_t)n_images * rows_per_image < max_chips ? (int64_t)n_images * rows_per_image : max_chips;
  const int grid = dh_grid_for(cap * tiles_per_chip, 1, kMaxGrid);
  hipLaunchKernelGGL(face_chips_resize_kernel, dim3(grid), dim3(kTileThreads), 0, s, images_dev, src, chip_src_out, count_out, (int)max_chips,
                     (int)S, runs_per_row, tiles_per_chip, chips_out);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_face_chips_ex_workspace(int32_t n_images, int32_t rows_per_image, int32_t S, int32_t filter, size_t* bytes) {
  DH_REQUIRE(S >= 1 && S <= kMaxS, DANHIP_EINVAL, "face_chips_ex_workspace: S %d outside 1 .. %d", S, kMaxS);
  DH_REQUIRE(filter == DANHIP_FACE_CHIPS_LINEAR || filter == DANHIP_FACE_CHIPS_AREA, DANHIP_EINVAL,
             "face_chips_ex_workspace: filter %d is neither 0 (linear) nor 1 (area)", filter);
  return danhip_face_chips_workspace(n_images, rows_per_image, bytes);       // 0: the area form's band of horizontal sums lives in LDS
}

extern "C" int danhip_face_chips_u8_ex(const danhip_resize_item* images_host, const danhip_resize_item* images_dev, int32_t n_images,
                                       const uint8_t* src, int64_t src_bytes, const float* dets, const int32_t* num, int32_t rows_per_image,
                                       int32_t S, int32_t margin_pm, int32_t square, float score_threshold, uint8_t* chips_out,
                                       int32_t* chip_src_out, int32_t* count_out, int32_t max_chips, void* workspace, size_t workspace_bytes,
                                       void* stream, int32_t filter, int32_t pad, const uint8_t fill_rgb[3]) {
  DH_REQUIRE(filter == DANHIP_FACE_CHIPS_LINEAR || filter == DANHIP_FACE_CHIPS_AREA, DANHIP_EINVAL,
             "face_chips_u8_ex: filter %d is neither 0 (linear) nor 1 (area)", filter);
  DH_REQUIRE(pad == 0 || pad == 1, DANHIP_EINVAL, "face_chips_u8_ex: pad is 0 or 1");
  DH_REQUIRE(S >= 1 && S <= kMaxS, DANHIP_EINVAL, "face_chips_u8_ex: S %d outside 1 .. %d", S, kMaxS);
  DH_REQUIRE(margin_pm >= 0 && margin_pm <= kMaxMargin, DANHIP_EINVAL, "face_chips_u8_ex: margin_pm %d outside 0 .. %d", margin_pm, kMaxMargin);
  DH_REQUIRE(square == 0 || square == 1, DANHIP_EINVAL, "face_chips_u8_ex: square is 0 or 1");
  DH_REQUIRE(!std::isnan(score_threshold), DANHIP_EINVAL, "face_chips_u8_ex: score_threshold is NaN");
  DH_REQUIRE(max_chips >= 0, DANHIP_EINVAL, "face_chips_u8_ex: max_chips %d is negative", max_chips);
  size_t need = 0;
  if (danhip_face_chips_ex_workspace(n_images, rows_per_image, S, filter, &need) != DANHIP_OK) return DANHIP_EINVAL;
  DH_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), DANHIP_EINVAL, "face_chips_u8_ex: workspace of %zu bytes, %zu needed",
             workspace_bytes, need);
  DH_REQUIRE(count_out, DANHIP_EINVAL, "face_chips_u8_ex: NULL count_out");
  hipStream_t s = (hipStream_t)stream;
  if (n_images == 0 || rows_per_image == 0) return danhip_zero_async(count_out, 4, s);
  DH_REQUIRE(images_host && images_dev && src && dets && num, DANHIP_EINVAL, "face_chips_u8_ex: NULL images / src / dets / num");
  DH_REQUIRE(max_chips == 0 || (chips_out && chip_src_out), DANHIP_EINVAL, "face_chips_u8_ex: NULL chips_out / chip_src_out");
  for (int32_t i = 0; i < n_images; ++i) {
    const danhip_resize_item& it = images_host[i];
    DH_REQUIRE(it.H >= 1 && it.W >= 1 && (int64_t)it.pitch >= 3 * (int64_t)it.W && it.src_offset >= 0, DANHIP_EINVAL,
               "face_chips_u8_ex: image %d: a non-positive size, pitch below 3 * W or a negative offset", i);
    DH_REQUIRE(it.src_offset + (int64_t)(it.H - 1) * it.pitch + 3 * (int64_t)it.W <= src_bytes, DANHIP_EINVAL,
               "face_chips_u8_ex: image %d reads past the source buffer", i);
  }
  const uint32_t fill = fill_rgb ? (uint32_t)fill_rgb[0] | ((uint32_t)fill_rgb[1] << 8) | ((uint32_t)fill_rgb[2] << 16) : 0u;
  hipLaunchKernelGGL(face_chips_select_ex_kernel, dim3(1), dim3(kSelThreads), 0, s, images_dev, (int)n_images, dets, num, (int)rows_per_image,
                     (int)margin_pm, (int)square, (int)pad, score_threshold, chip_src_out, count_out, (int)max_chips);
  DH_LAUNCH_CHECK();
  if (max_chips == 0) return DANHIP_OK;
  const int64_t cap = (int64_t)n_images * rows_per_image < max_chips ? (int64_t)n_images * rows_per_image : max_chips;
  if (filter == DANHIP_FACE_CHIPS_AREA) {
    const int col_tiles = cdiv(S, kAreaCols);
    const int grid = dh_grid_for(cap * S * col_tiles, 1, kMaxGrid);
    hipLaunchKernelGGL(face_chips_area_kernel, dim3(grid), dim3(kAreaThreads), 0, s, images_dev, src, chip_src_out, count_out, (int)max_chips,
                       (int)S, col_tiles, fill, chips_out);
  } else {
    const int runs_per_row = cdiv(S, kRun), tiles_per_chip = cdiv((long)S * runs_per_row, kTileThreads);
    const int grid = dh_grid_for(cap * tiles_per_chip, 1, kMaxGrid);
    if (pad)
      hipLaunchKernelGGL(face_chips_resize_fetch_kernel, dim3(grid), dim3(kTileThreads), 0, s, images_dev, src, chip_src_out, count_out,
                         (int)max_chips, (int)S, runs_per_row, tiles_per_chip, fill, chips_out);
    else                                                         // the clipped rectangle: the old entry point's kernel, the same bytes
      hipLaunchKernelGGL(face_chips_resize_kernel, dim3(grid), dim3(kTileThreads), 0, s, images_dev, src, chip_src_out, count_out,
                         (int)max_chips, (int)S, runs_per_row, tiles_per_chip, chips_out);
  }
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}
