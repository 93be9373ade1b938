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
#include "common.h"
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
  const uint8_t* staging;
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
  __device__ __forceinline__ uint32_t header_byte(const DhJencImage& im, int i) { return i >= 0 && i < im.header_len ? staging[im.header_off + i] : 0; }
};

__device__ __forceinline__ const DhJencImage* image_of(const uint8_t* staging, int i) {
  const DhJencHeader* H = reinterpret_cast<const DhJencHeader*>(staging);
  return reinterpret_cast<const DhJencImage*>(staging + H->off_images) + i;
}

__device__ __forceinline__ void load_tabs(const uint8_t* staging, uint32_t* lds) {
  const DhJencHeader* H = reinterpret_cast<const DhJencHeader*>(staging);
  const uint32_t* t = reinterpret_cast<const uint32_t*>(staging + H->off_tabs);
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
  const DhJencImage im = *image_of(staging, blockIdx.y);
  if (!im.prepared || (int)blockIdx.x >= im.len_groups) return;       // uniform: an image smaller than the batch's largest
  __shared__ uint32_t tabs[4 * 256];
  __shared__ uint64_t sums[DH_JHUF_GROUP];
  __shared__ uint32_t flags;
  if (threadIdx.x == 0) flags = 0;
  load_tabs(staging, tabs);
  DevCtx c{coef, coef_count, tabs, ws, nullptr, staging};
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
  const DhJencImage im = *image_of(staging, blockIdx.y);
  if (!im.prepared || (int)blockIdx.x >= im.len_groups) return;
  __shared__ uint32_t tabs[4 * 256];
  __shared__ uint64_t sums[DH_JHUF_GROUP];
  load_tabs(staging, tabs);
  DevCtx c{coef, coef_count, tabs, ws, nullptr, staging};
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
  DevCtx c{nullptr, 0, nullptr, ws, nullptr, staging};
  const uint32_t n = dh_jhuf_lane_ffcount(c, im, scan_bytes, (int64_t)blockIdx.x * DH_JHUF_CHUNK_BYTES + (int64_t)threadIdx.x * DH_JHUF_LANE_BYTES);
  uint32_t total;
  group_scan<uint32_t>(n, sums, &total);
  if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(ws + im.ws_ff)[blockIdx.x] = total;
}

__global__ __launch_bounds__(DH_JHUF_GROUP) void jpeg_enc_huff_finish_kernel(const uint8_t* __restrict__ staging, uint8_t* __restrict__ ws,
                                                                             uint8_t* __restrict__ files, int64_t* __restrict__ sizes,
                                                                             int32_t* __restrict__ status) {
  const DhJencImage im = *image_of(staging, blockIdx.x);
  if (!im.prepared) return;
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
  DevCtx c{nullptr, 0, nullptr, ws, files, staging};
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
  const DhJencImage im = *image_of(staging, blockIdx.y);
  if (!im.prepared || (int)blockIdx.x >= im.stuff_groups) return;
  if (status[blockIdx.y] & DANHIP_JPEG_ENC_DEV_CAPACITY) return;
  const int64_t scan_bytes = dh_jhuf_scan_bytes(im, reinterpret_cast<const uint64_t*>(ws + im.ws_goff)[im.len_groups]);
  if ((int64_t)blockIdx.x * DH_JHUF_CHUNK_BYTES >= scan_bytes) return;
  __shared__ uint32_t sums[DH_JHUF_GROUP];
  DevCtx c{nullptr, 0, nullptr, ws, files, staging};
  const int64_t byte0 = (int64_t)blockIdx.x * DH_JHUF_CHUNK_BYTES + (int64_t)threadIdx.x * DH_JHUF_LANE_BYTES;
  const uint32_t n = dh_jhuf_lane_ffcount(c, im, scan_bytes, byte0);
  uint32_t total;
  const uint32_t before = group_scan<uint32_t>(n, sums, &total);
  dh_jhuf_lane_scatter(c, im, scan_bytes, byte0, reinterpret_cast<const uint32_t*>(ws + im.ws_ffoff)[blockIdx.x] + before);
}

}  // namespace

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
