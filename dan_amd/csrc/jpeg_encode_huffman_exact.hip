// Huffman stage of the JPEG encoder on the device (include/danhip.h, "JPEG encode: Huffman stage on the device"): six launches per BATCH
// over the staging buffer that danhip_jpeg_encode_scan_prepare filled.  Every per-lane step is a call into jpeg_encode_huffman.h, the text
// danhip_jpeg_encode_entropy_emulate_batch runs on the host (jpeg_encode.cpp); what is here is the context over device memory, the
// workgroup sums and prefix sums between the lanes, and the launcher.
//   1 jpeg_enc_huff_length_kernel   (workgroup, image): a lane's block length, the workgroup's sum | invalid flag, zero fill of the
//                                   workgroup's share of the unstuffed buffer
//   2 jpeg_enc_huff_offsets_kernel  (image): prefix sum of the workgroup sums -> 64-bit bit offsets, the scan's bits, status[i]
//   3 jpeg_enc_huff_write_kernel    (workgroup, image): the length again, prefix sum over the lanes, the codes OR-ed in at the bit offset
//   4 jpeg_enc_huff_count_kernel    (chunk, image): FF bytes of a chunk of the unstuffed scan
//   5 jpeg_enc_huff_finish_kernel   (image): prefix sum of the chunk counts, markers in front, EOI behind, sizes[i], the capacity flag
//   6 jpeg_enc_huff_stuff_kernel    (chunk, image): prefix sum over the lanes, bytes scattered with 00 behind every FF
// Grids 1, 3, 4 and 6 are sized by the batch's largest image from the host-derived worst case; a workgroup beyond its image's count, or
// beyond the scan's actual bytes, leaves at once.  No workgroup waits for another inside a launch; the only atomics are integer ORs.
//
// A staging buffer prepared with DANHIP_JPEG_ENC_OPTIMIZE (include/danhip.h, "JPEG encode: optimised Huffman tables") puts three launches
// in front, over the image's region at the head of the workspace (jpeg_encode_huffman.h, DH_JHUF_OPT_*):
//   a jpeg_enc_huff_clear_kernel      (image): zeroes the region
//   b jpeg_enc_huff_histogram_kernel  (work item, image): the symbols of DH_JHUF_HIST_BLOCKS blocks, counted per wave in LDS, the non-zero
//                                     sums added into the image's 4 x 257 table (integer atomics: the sums do not depend on the order)
//   c jpeg_enc_huff_tables_kernel     (image): a wave per table runs dh_jenc_optimal_table (jpeg_encode.h) in its first lane, then all
//                                     lanes write bits / vals, the code | length table and the markers with the image's DHT segments
// The six launches read their tables and markers through ImageSource: the staged standard ones, or the image's region.
#include "common.h"
#include "jpeg_encode.h"
#include "jpeg_encode_huffman.h"

// jpeg_encode.cpp: NULL = the staging buffer is what the prepare call makes of these descriptors and buffer sizes
extern "C" const char* danhip_jpeg_encode_scan_check(const void* staging, size_t staging_bytes, const danhip_jpeg_enc_desc* descs, int32_t B,
                                                     int64_t coef_count, int64_t file_bytes);

namespace {

typedef __attribute__((ext_vector_type(8))) short s16x8;

struct DevCtx {                    // the context of jpeg_encode_huffman.h over device memory; an index outside its range is dropped
  const int16_t* coef;
  int64_t coef_count;
  const uint32_t* tabs;            // 4 x 256, in LDS for launches 1 and 3
  uint8_t* ws;
  uint8_t* files;
  const uint8_t* header;           // the image's markers, im.header_len of them
  __device__ __forceinline__ void load_block(int64_t el, int16_t v[64]) {
    if (el < 0 || el + 64 > coef_count) {
#pragma unroll
      for (int k = 0; k < 64; ++k) v[k] = 0;
      return;
    }
    const s16x8* p = reinterpret_cast<const s16x8*>(coef + el);     // el is a multiple of 64, the buffer 16-byte aligned
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const s16x8 x = p[j];
#pragma unroll
      for (int r = 0; r < 8; ++r) v[j * 8 + r] = x[r];
    }
  }
  __device__ __forceinline__ int dc(int64_t el) { return el >= 0 && el < coef_count ? coef[el] : 0; }
  __device__ __forceinline__ uint32_t tab(int t, int sym) { return tabs[((t & 3) << 8) | (sym & 255)]; }
  __device__ __forceinline__ void or_word(const DhJencImage& im, int64_t w, uint32_t v) {
    if (v == 0 || w < 0 || w >= im.bits_bytes / 4) return;
    atomicOr(reinterpret_cast<unsigned*>(ws + im.ws_bits) + w, __builtin_bswap32(v));
  }
  __device__ __forceinline__ uint32_t ubyte(const DhJencImage& im, int64_t i) { return i >= 0 && i < im.bits_bytes ? ws[im.ws_bits + i] : 0; }
  __device__ __forceinline__ void file_store(const DhJencImage& im, int64_t i, uint32_t b) {
    if (i >= 0 && i < im.file_capacity) files[im.file_offset + i] = (uint8_t)b;
  }
  __device__ __forceinline__ uint32_t header_byte(const DhJencImage& im, int i) { return i >= 0 && i < im.header_len ? header[i] : 0; }
};

__device__ __forceinline__ const DhJencImage* image_of(const uint8_t* staging, int i) {
  const DhJencHeader* H = reinterpret_cast<const DhJencHeader*>(staging);
  return reinterpret_cast<const DhJencImage*>(staging + H->off_images) + i;
}

// where image i's code tables and markers lie: staged (the standard tables), or in the image's region of the workspace (optimize).
// *im is the caller's copy of the staged image: its header_len becomes the length the tables launch wrote.
struct ImageSource {
  const uint32_t* tabs;
  const uint8_t* header;
};

__device__ __forceinline__ ImageSource source_of(const uint8_t* staging, const uint8_t* ws, int i, DhJencImage* im) {
  const DhJencHeader* H = reinterpret_cast<const DhJencHeader*>(staging);
  if (!H->optimize) return ImageSource{reinterpret_cast<const uint32_t*>(staging + H->off_tabs), staging + im->header_off};
  const uint8_t* region = ws + (int64_t)i * DH_JHUF_OPT_STRIDE;
  const int32_t len = *reinterpret_cast<const int32_t*>(region + DH_JHUF_OPT_WORDS);
  im->header_len = len < 0 ? 0 : (len > DH_JHUF_OPT_HEADER_MAX ? DH_JHUF_OPT_HEADER_MAX : len);
  return ImageSource{reinterpret_cast<const uint32_t*>(region + DH_JHUF_OPT_TABS), region + DH_JHUF_OPT_HEADER};
}

__device__ __forceinline__ void load_tabs(const uint32_t* t, uint32_t* lds) {
#pragma unroll
  for (int k = 0; k < 4; ++k) lds[k * DH_JHUF_GROUP + threadIdx.x] = t[k * DH_JHUF_GROUP + threadIdx.x];
  __syncthreads();
}

// exclusive prefix sum of v over the workgroup's 256 lanes through lds[256]; *total: the workgroup's sum.  Every lane calls it.
template <class T>
__device__ __forceinline__ T group_scan(T v, T* lds, T* total) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < DH_JHUF_GROUP; off <<= 1) {
    const T x = t >= off ? lds[t - off] : (T)0;
    __syncthreads();
    lds[t] += x;
    __syncthreads();
  }
  *total = lds[DH_JHUF_GROUP - 1];
  const T r = lds[t] - v;
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_length_kernel(const uint8_t* __restrict__ staging, const int16_t* __restrict__ coef,
                                                                             int64_t coef_count, uint8_t* __restrict__ ws) {
  DhJencImage im = *image_of(staging, blockIdx.y);
  if (!im.prepared || (int)blockIdx.x >= im.len_groups) return;       // uniform: an image smaller than the batch's largest
  __shared__ uint32_t tabs[4 * 256];
  __shared__ uint64_t sums[DH_JHUF_GROUP];
  __shared__ uint32_t flags;
  if (threadIdx.x == 0) flags = 0;
  const ImageSource src = source_of(staging, ws, blockIdx.y, &im);
  load_tabs(src.tabs, tabs);
  DevCtx c{coef, coef_count, tabs, ws, nullptr, src.header};
  const int64_t s = (int64_t)blockIdx.x * DH_JHUF_GROUP + threadIdx.x;
  uint64_t len = 0;
  if (s < im.nblocks) len = dh_jhuf_lane_length(c, im, s);
  if (len & DH_JHUF_INVALID) {
    atomicOr(&flags, 1u);                                             // LDS
    len = 0;
  }
  uint64_t total;
  group_scan<uint64_t>(len, sums, &total);                            // its barriers also order the flag
  if (threadIdx.x == 0) reinterpret_cast<uint64_t*>(ws + im.ws_gsum)[blockIdx.x] = total | (flags ? DH_JHUF_INVALID : 0);
  // the workgroup's share of the unstuffed buffer: DH_JHUF_GROUP * DH_JHUF_BLOCK_BYTES bytes, the shares tile bits_bytes
  uint4* z = reinterpret_cast<uint4*>(ws + im.ws_bits + (int64_t)blockIdx.x * DH_JHUF_GROUP * DH_JHUF_BLOCK_BYTES);
  for (int k = threadIdx.x; k < DH_JHUF_GROUP * DH_JHUF_BLOCK_BYTES / 16; k += DH_JHUF_GROUP) z[k] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_offsets_kernel(const uint8_t* __restrict__ staging, uint8_t* __restrict__ ws,
                                                                              int64_t* __restrict__ sizes, int32_t* __restrict__ status) {
  const DhJencImage im = *image_of(staging, blockIdx.x);
  if (!im.prepared) {
    if (threadIdx.x == 0) { status[blockIdx.x] = DANHIP_JPEG_HOSTONLY; sizes[blockIdx.x] = 0; }
    return;
  }
  __shared__ uint64_t sums[DH_JHUF_GROUP];
  const uint64_t* gsum = reinterpret_cast<const uint64_t*>(ws + im.ws_gsum);
  uint64_t* goff = reinterpret_cast<uint64_t*>(ws + im.ws_goff);
  const int per = (im.len_groups + DH_JHUF_GROUP - 1) / DH_JHUF_GROUP;
  const int g0 = min((int)threadIdx.x * per, im.len_groups), g1 = min(g0 + per, im.len_groups);
  uint64_t mine = 0, flag = 0;
  for (int g = g0; g < g1; ++g) {
    const uint64_t v = gsum[g];
    flag |= v & DH_JHUF_INVALID;
    mine += v & ~DH_JHUF_INVALID;
  }
  uint64_t total;
  uint64_t at = group_scan<uint64_t>(mine, sums, &total);
  for (int g = g0; g < g1; ++g) {
    goff[g] = at;
    at += gsum[g] & ~DH_JHUF_INVALID;
  }
  if (threadIdx.x == 0) goff[im.len_groups] = total;
  const int any = __syncthreads_or(flag != 0);
  if (threadIdx.x == 0) status[blockIdx.x] = any ? DANHIP_JPEG_ENC_DEV_RANGE : 0;
}

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_write_kernel(const uint8_t* __restrict__ staging, const int16_t* __restrict__ coef,
                                                                            int64_t coef_count, uint8_t* __restrict__ ws) {
  DhJencImage im = *image_of(staging, blockIdx.y);
  if (!im.prepared || (int)blockIdx.x >= im.len_groups) return;
  __shared__ uint32_t tabs[4 * 256];
  __shared__ uint64_t sums[DH_JHUF_GROUP];
  const ImageSource src = source_of(staging, ws, blockIdx.y, &im);
  load_tabs(src.tabs, tabs);
  DevCtx c{coef, coef_count, tabs, ws, nullptr, src.header};
  const int64_t s = (int64_t)blockIdx.x * DH_JHUF_GROUP + threadIdx.x;
  uint64_t len = 0;
  if (s < im.nblocks) len = dh_jhuf_lane_length(c, im, s);
  uint64_t total;
  const uint64_t before = group_scan<uint64_t>(len & ~DH_JHUF_INVALID, sums, &total);
  if (s < im.nblocks) dh_jhuf_lane_write(c, im, s, reinterpret_cast<const uint64_t*>(ws + im.ws_goff)[blockIdx.x] + before, len);
}

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_count_kernel(const uint8_t* __restrict__ staging, uint8_t* __restrict__ ws) {
  const DhJencImage im = *image_of(staging, blockIdx.y);
  if (!im.prepared || (int)blockIdx.x >= im.stuff_groups) return;
  const int64_t scan_bytes = dh_jhuf_scan_bytes(im, reinterpret_cast<const uint64_t*>(ws + im.ws_goff)[im.len_groups]);
  if ((int64_t)blockIdx.x * DH_JHUF_CHUNK_BYTES >= scan_bytes) return;             // uniform: the worst case is rarely reached
  __shared__ uint32_t sums[DH_JHUF_GROUP];
  DevCtx c{nullptr, 0, nullptr, ws, nullptr, nullptr};                             // no marker is read here
  const uint32_t n = dh_jhuf_lane_ffcount(c, im, scan_bytes, (int64_t)blockIdx.x * DH_JHUF_CHUNK_BYTES + (int64_t)threadIdx.x * DH_JHUF_LANE_BYTES);
  uint32_t total;
  group_scan<uint32_t>(n, sums, &total);
  if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(ws + im.ws_ff)[blockIdx.x] = total;
}

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_finish_kernel(const uint8_t* __restrict__ staging, uint8_t* __restrict__ ws,
                                                                             uint8_t* __restrict__ files, int64_t* __restrict__ sizes,
                                                                             int32_t* __restrict__ status) {
  DhJencImage im = *image_of(staging, blockIdx.x);
  if (!im.prepared) return;
  const ImageSource src = source_of(staging, ws, blockIdx.x, &im);
  __shared__ uint32_t sums[DH_JHUF_GROUP];
  const int64_t scan_bytes = dh_jhuf_scan_bytes(im, reinterpret_cast<const uint64_t*>(ws + im.ws_goff)[im.len_groups]);
  const int chunks = (int)min((scan_bytes + DH_JHUF_CHUNK_BYTES - 1) / DH_JHUF_CHUNK_BYTES, (int64_t)im.stuff_groups);
  const uint32_t* ff = reinterpret_cast<const uint32_t*>(ws + im.ws_ff);
  uint32_t* ffoff = reinterpret_cast<uint32_t*>(ws + im.ws_ffoff);
  const int per = (chunks + DH_JHUF_GROUP - 1) / DH_JHUF_GROUP;
  const int g0 = min((int)threadIdx.x * per, chunks), g1 = min(g0 + per, chunks);
  uint32_t mine = 0;
  for (int g = g0; g < g1; ++g) mine += ff[g];
  uint32_t total_ff;
  uint32_t at = group_scan<uint32_t>(mine, sums, &total_ff);
  for (int g = g0; g < g1; ++g) {
    ffoff[g] = at;
    at += ff[g];
  }
  const bool fits = (int64_t)im.header_len + scan_bytes + total_ff + 2 <= im.file_capacity;
  DevCtx c{nullptr, 0, nullptr, ws, files, src.header};
  int64_t size = 0;
  if (fits) size = dh_jhuf_lane_finish(c, im, scan_bytes, total_ff, (int)threadIdx.x, DH_JHUF_GROUP);
  if (threadIdx.x == 0) {
    const int32_t st = status[blockIdx.x] | (fits ? 0 : DANHIP_JPEG_ENC_DEV_CAPACITY);       // launch 2 wrote the word
    status[blockIdx.x] = st;
    sizes[blockIdx.x] = st ? 0 : size;
  }
}

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_stuff_kernel(const uint8_t* __restrict__ staging, uint8_t* __restrict__ ws,
                                                                            uint8_t* __restrict__ files, const int32_t* __restrict__ status) {
  DhJencImage im = *image_of(staging, blockIdx.y);
  if (!im.prepared || (int)blockIdx.x >= im.stuff_groups) return;
  if (status[blockIdx.y] & DANHIP_JPEG_ENC_DEV_CAPACITY) return;
  const ImageSource src = source_of(staging, ws, blockIdx.y, &im);                 // the markers' length: where the scan starts
  const int64_t scan_bytes = dh_jhuf_scan_bytes(im, reinterpret_cast<const uint64_t*>(ws + im.ws_goff)[im.len_groups]);
  if ((int64_t)blockIdx.x * DH_JHUF_CHUNK_BYTES >= scan_bytes) return;
  __shared__ uint32_t sums[DH_JHUF_GROUP];
  DevCtx c{nullptr, 0, nullptr, ws, files, src.header};
  const int64_t byte0 = (int64_t)blockIdx.x * DH_JHUF_CHUNK_BYTES + (int64_t)threadIdx.x * DH_JHUF_LANE_BYTES;
  const uint32_t n = dh_jhuf_lane_ffcount(c, im, scan_bytes, byte0);
  uint32_t total;
  const uint32_t before = group_scan<uint32_t>(n, sums, &total);
  dh_jhuf_lane_scatter(c, im, scan_bytes, byte0, reinterpret_cast<const uint32_t*>(ws + im.ws_ffoff)[blockIdx.x] + before);
}

// ---- optimize: the three launches in front ----

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_clear_kernel(uint8_t* __restrict__ ws) {
  uint4* z = reinterpret_cast<uint4*>(ws + (int64_t)blockIdx.x * DH_JHUF_OPT_STRIDE);
  for (int k = threadIdx.x; k < DH_JHUF_OPT_STRIDE / 16; k += DH_JHUF_GROUP) z[k] = make_uint4(0, 0, 0, 0);
}

constexpr int kWaves = DH_JHUF_GROUP / 64;                // a wave's own table keeps the DC and EOB bins of the other waves out of its way
static_assert(DH_JHUF_GROUP % 64 == 0, "whole waves");

struct LdsHistogram {              // dh_jhuf_symbols' sink: t < 4 and sym < 256 by the walk's own range checks, masked once more
  uint32_t* h;                     // [4][257] of this lane's wave
  __device__ __forceinline__ void add(int t, int sym) { atomicAdd(&h[(t & 3) * 257 + (sym & 255)], 1u); }
};

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_histogram_kernel(const uint8_t* __restrict__ staging, const int16_t* __restrict__ coef,
                                                                                int64_t coef_count, uint8_t* __restrict__ ws) {
  const DhJencImage im = *image_of(staging, blockIdx.y);
  const int64_t first = (int64_t)blockIdx.x * DH_JHUF_HIST_BLOCKS;
  if (!im.prepared || first >= im.nblocks) return;                    // uniform
  __shared__ uint32_t hist[kWaves][4 * 257];
  for (int k = threadIdx.x; k < kWaves * 4 * 257; k += DH_JHUF_GROUP) (&hist[0][0])[k] = 0;
  __syncthreads();
  DevCtx c{coef, coef_count, nullptr, ws, nullptr, nullptr};          // no table and no marker is read here
  LdsHistogram sink{hist[threadIdx.x >> 6]};
  for (int r = 0; r < DH_JHUF_HIST_ROUNDS; ++r) {
    const int64_t s = first + (int64_t)r * DH_JHUF_GROUP + threadIdx.x;
    if (s < im.nblocks) dh_jhuf_lane_symbols(c, im, s, sink);         // a value out of range: the length launch flags the image
  }
  __syncthreads();
  unsigned* counts = reinterpret_cast<unsigned*>(ws + (int64_t)blockIdx.y * DH_JHUF_OPT_STRIDE + DH_JHUF_OPT_COUNTS);
  for (int k = threadIdx.x; k < 4 * 257; k += DH_JHUF_GROUP) {
    uint32_t n = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) n += hist[w][k];
    if (n) atomicAdd(&counts[k], n);
  }
}

// staging == NULL: regions whose counts the caller filled (danhip_jpeg_optimal_tables_device); the markers are then left alone
__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_tables_kernel(const uint8_t* __restrict__ staging, uint8_t* __restrict__ ws) {
  static_assert(kWaves == 4, "a wave per table");
  DhJencImage im;
  if (staging) {
    im = *image_of(staging, blockIdx.x);
    if (!im.prepared) return;
  }
  uint8_t* region = ws + (int64_t)blockIdx.x * DH_JHUF_OPT_STRIDE;
  __shared__ int32_t work[4][DH_JENC_TABLE_WORK];
  __shared__ int32_t counts[4][257];
  __shared__ uint8_t bits[4][17];
  __shared__ uint8_t vals[4][256];
  __shared__ uint32_t tabs[4][256];
  __shared__ int32_t nvals[4];
  const int t = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t* gcounts = reinterpret_cast<const uint32_t*>(region + DH_JHUF_OPT_COUNTS);
  for (int k = threadIdx.x; k < 4 * 257; k += DH_JHUF_GROUP) {
    const uint32_t n = gcounts[k];
    (&counts[0][0])[k] = n > 0x7fffffffu ? 0x7fffffff : (int32_t)n;
  }
  for (int k = threadIdx.x; k < 4 * 256; k += DH_JHUF_GROUP) (&tabs[0][0])[k] = 0;
  __syncthreads();
  int ok = 1;
  if (lane == 0) {
    int64_t sum = 0;
    for (int k = 0; k < 256; ++k) sum += counts[t][k];
    ok = sum < 0x7fffffff && dh_jenc_optimal_table(counts[t], bits[t], vals[t], work[t]);
    int n = 0;
    if (ok) {                                                         // the codes of T.81 C.2 from bits / vals
      unsigned code = 0;
      for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[t][l]; ++i, ++n, ++code) tabs[t][vals[t][n]] = code | ((uint32_t)l << 16);
        code <<= 1;
      }
    }
    nvals[t] = n;
  }
  const int all_ok = __syncthreads_and(ok);
  // a table that cannot be made leaves all four empty: every block then fails its DC lookup and the length launch flags the image
  uint32_t* gtabs = reinterpret_cast<uint32_t*>(region + DH_JHUF_OPT_TABS);
  for (int k = threadIdx.x; k < 4 * 256; k += DH_JHUF_GROUP) gtabs[k] = all_ok ? (&tabs[0][0])[k] : 0u;
  uint8_t* gbv = region + DH_JHUF_OPT_BITSVALS;
  for (int k = threadIdx.x; k < 4 * 273; k += DH_JHUF_GROUP) {
    const int tt = k / 273, j = k - tt * 273;
    gbv[k] = !all_ok ? 0 : (j < 17 ? bits[tt][j] : vals[tt][j - 17]);
  }
  if (!staging) return;
  // the markers: the staged ones up to the first DHT, the four segments (marker, length, table id, 16 counts, the symbols), the staged SOS
  const uint8_t* staged = staging + im.header_off;
  const int std_dht = im.header_len - DH_JHUF_HEADER_PRE - DH_JHUF_HEADER_SOS;
  uint8_t* out = region + DH_JHUF_OPT_HEADER;
  for (int k = threadIdx.x; k < DH_JHUF_HEADER_PRE; k += DH_JHUF_GROUP) out[k] = staged[k];
  int at = DH_JHUF_HEADER_PRE;
  for (int tt = 0; tt < 4; ++tt) {
    const int n = all_ok ? nvals[tt] : 0;                             // at most 256: the segment fits its share of DH_JHUF_OPT_HEADER_MAX
    const int seg = 2 + 2 + 1 + 16 + n;
    for (int k = threadIdx.x; k < seg; k += DH_JHUF_GROUP) {
      uint32_t b;
      if (k == 0) b = 0xff;
      else if (k == 1) b = 0xc4;
      else if (k == 2) b = (uint32_t)(seg - 2) >> 8;
      else if (k == 3) b = (uint32_t)(seg - 2) & 255;
      else if (k == 4) b = (uint32_t)(((tt & 1) << 4) | (tt >> 1));
      else if (k < 21) b = all_ok ? bits[tt][k - 4] : 0;               // bits[1 .. 16]
      else b = vals[tt][k - 21];
      out[at + k] = (uint8_t)b;
    }
    at += seg;
  }
  for (int k = threadIdx.x; k < DH_JHUF_HEADER_SOS; k += DH_JHUF_GROUP) out[at + k] = staged[DH_JHUF_HEADER_PRE + std_dht + k];
  if (threadIdx.x == 0) *reinterpret_cast<int32_t*>(region + DH_JHUF_OPT_WORDS) = at + DH_JHUF_HEADER_SOS;
}

}  // namespace

extern "C" int danhip_jpeg_optimal_tables_device(void* regions_dev, int32_t n, void* stream) {
  DH_REQUIRE(regions_dev && n >= 1 && n <= 65535 && ((uintptr_t)regions_dev & 15) == 0, DANHIP_EINVAL,
             "jpeg_optimal_tables_device: bad arguments (1 <= n <= 65535 regions of danhip_jpeg_encode_optimize_layout's stride, 16-byte aligned)");
  hipLaunchKernelGGL(jpeg_enc_huff_tables_kernel, dim3((unsigned)n), dim3(DH_JHUF_GROUP), 0, (hipStream_t)stream, (const uint8_t*)nullptr,
                     (uint8_t*)regions_dev);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_jpeg_encode_huffman_batch(const void* staging_host, const void* staging_dev, size_t staging_bytes,
                                                const danhip_jpeg_enc_desc* descs_host, int32_t B, const int16_t* coef_dev, int64_t coef_count,
                                                uint8_t* files_dev, int64_t file_bytes, int64_t* sizes_dev, int32_t* status_dev, void* workspace,
                                                size_t workspace_bytes, int32_t* launches, void* stream) {
  if (launches) *launches = 0;
  DH_REQUIRE(staging_host && staging_dev && descs_host && B >= 1 && B <= 65535 && coef_count >= 0 && file_bytes >= 0, DANHIP_EINVAL,
             "jpeg_encode_huffman_batch: bad arguments (1 <= B <= 65535, staging in host and device memory, host descriptors)");
  DH_REQUIRE(coef_dev && files_dev && sizes_dev && status_dev, DANHIP_EINVAL, "jpeg_encode_huffman_batch: NULL buffer");
  DH_REQUIRE(((uintptr_t)staging_host & 15) == 0 && ((uintptr_t)staging_dev & 15) == 0 && ((uintptr_t)coef_dev & 15) == 0 &&
                 ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)sizes_dev & 7) == 0 && ((uintptr_t)status_dev & 3) == 0,
             DANHIP_EINVAL, "jpeg_encode_huffman_batch: staging, coef_dev and workspace must be 16-byte aligned, sizes_dev 8-byte, status_dev 4-byte");
  const char* why = danhip_jpeg_encode_scan_check(staging_host, staging_bytes, descs_host, B, coef_count, file_bytes);
  if (why) {
    danhip_set_error("jpeg_encode_huffman_batch: %s", why);
    return DANHIP_EINVAL;
  }
  const DhJencHeader* H = (const DhJencHeader*)staging_host;
  if (H->nprepared == 0) return DANHIP_OK;
  DH_REQUIRE(workspace && workspace_bytes >= (size_t)H->workspace_bytes, DANHIP_EINVAL,
             "jpeg_encode_huffman_batch: workspace of %zu bytes, danhip_jpeg_encode_scan_workspace_bytes asks for %lld", workspace_bytes,
             (long long)H->workspace_bytes);
  hipStream_t s = (hipStream_t)stream;
  const uint8_t* st = (const uint8_t*)staging_dev;
  uint8_t* ws = (uint8_t*)workspace;
  const dim3 lanes(DH_JHUF_GROUP), per_block((unsigned)H->max_len_groups, (unsigned)B), per_chunk((unsigned)H->max_stuff_groups, (unsigned)B);
  int n = 0;
  if (H->optimize) {
    const dim3 per_item((unsigned)(((int64_t)H->max_len_groups * DH_JHUF_GROUP + DH_JHUF_HIST_BLOCKS - 1) / DH_JHUF_HIST_BLOCKS), (unsigned)B);
    hipLaunchKernelGGL(jpeg_enc_huff_clear_kernel, dim3((unsigned)B), lanes, 0, s, ws);
    DH_LAUNCH_CHECK();
    if (launches) *launches = ++n;
    hipLaunchKernelGGL(jpeg_enc_huff_histogram_kernel, per_item, lanes, 0, s, st, coef_dev, coef_count, ws);
    DH_LAUNCH_CHECK();
    if (launches) *launches = ++n;
    hipLaunchKernelGGL(jpeg_enc_huff_tables_kernel, dim3((unsigned)B), lanes, 0, s, st, ws);
    DH_LAUNCH_CHECK();
    if (launches) *launches = ++n;
    static_assert(DANHIP_JPEG_ENCODE_OPTIMIZE_LAUNCHES == 3, "the launch count is part of the interface");
  }
  hipLaunchKernelGGL(jpeg_enc_huff_length_kernel, per_block, lanes, 0, s, st, coef_dev, coef_count, ws);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  hipLaunchKernelGGL(jpeg_enc_huff_offsets_kernel, dim3((unsigned)B), lanes, 0, s, st, ws, sizes_dev, status_dev);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  hipLaunchKernelGGL(jpeg_enc_huff_write_kernel, per_block, lanes, 0, s, st, coef_dev, coef_count, ws);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  hipLaunchKernelGGL(jpeg_enc_huff_count_kernel, per_chunk, lanes, 0, s, st, ws);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  hipLaunchKernelGGL(jpeg_enc_huff_finish_kernel, dim3((unsigned)B), lanes, 0, s, st, ws, files_dev, sizes_dev, status_dev);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  hipLaunchKernelGGL(jpeg_enc_huff_stuff_kernel, per_chunk, lanes, 0, s, st, ws, files_dev, status_dev);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  static_assert(DANHIP_JPEG_ENCODE_ENTROPY_LAUNCHES == 6, "the launch count is part of the interface");
  return DANHIP_OK;
}
