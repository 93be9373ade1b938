// Device half of the JPEG decoder (include/danhip.h, "Baseline JPEG decode"): two launches per BATCH, each a (workgroup, image) grid through
// the descriptor table that jpeg_entropy.cpp filled.  All integer; every line restates libjpeg's JDCT_ISLOW / fancy-upsampling / YCbCr
// arithmetic (tests/jpeg_protocol.py is the same text in numpy, pinned against Pillow on the CPU).
//   1 jpeg_idct_kernel          coefficient x table entry -> islow IDCT (CONST_BITS 13, PASS1_BITS 2) -> clamp(x + 128) -> planar uint8
//                               component planes in the workspace, pitch = block-grid width * 8.  Eight lanes own a block: a lane loads its
//                               COLUMN as one 16-byte load (the host stores blocks column-major), runs pass 1 in registers, the 8x8 transpose
//                               goes through LDS, pass 2 runs on a row and leaves as one 8-byte store.  A wave's loads are 1 KiB contiguous.
//   2 jpeg_upsample_rgb_kernel  triangle-filter chroma upsampling (h2v1 / h2v2, edges = the down-sampled component's own first / last
//                               sample, not the block padding; a component at most 2 samples wide is replicated) + 16-bit fixed-point YCbCr -> RGB; a lane makes 8 pixels of one row =
//                               24 contiguous bytes, a wave's stores are contiguous.
// LDS of launch 1: int32 [32 blocks][8 rows][8] with a block stride of 68 dwords.  The column writes (ds_write_b32: lanes j = 0..7 of four
// blocks per 32-lane group) then fall on banks 4 * block + j - at most 2 addresses per bank, which a ds_write_b32 absorbs - where the
// unpadded stride 64 would put four blocks on the same 8 banks; the row reads are two 16-byte reads per lane, 16-byte aligned.
#include "common.h"
#include "jpeg_layout.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

#define JPEG_LDS_BLOCK_STRIDE 68

// One 8-point pass of jidctint.c's jpeg_idct_islow (the same text for columns and rows; only the descale differs).
__device__ __forceinline__ void idct_islow_1d(int x[8], const int shift) {
  int z1 = (x[2] + x[6]) * 4433;
  const int e2 = z1 + x[6] * (-15137);
  const int e3 = z1 + x[2] * 6270;
  const int e0 = (x[0] + x[4]) * 8192;          // << CONST_BITS
  const int e1 = (x[0] - x[4]) * 8192;
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int o0 = x[7], o1 = x[5], o2 = x[3], o3 = x[1];
  z1 = o0 + o3;
  int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const int z5 = (z3 + z4) * 9633;
  o0 *= 2446; o1 *= 16819; o2 *= 25172; o3 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
  z3 += z5; z4 += z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  const int r = 1 << (shift - 1);
  x[0] = (t10 + o3 + r) >> shift; x[7] = (t10 - o3 + r) >> shift;
  x[1] = (t11 + o2 + r) >> shift; x[6] = (t11 - o2 + r) >> shift;
  x[2] = (t12 + o1 + r) >> shift; x[5] = (t12 - o1 + r) >> shift;
  x[3] = (t13 + o0 + r) >> shift; x[4] = (t13 - o0 + r) >> shift;
}

__device__ __forceinline__ unsigned clamp255(int v) { return (unsigned)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const danhip_jpeg_desc* __restrict__ descs,
                                                        uint8_t* __restrict__ ws) {
  const danhip_jpeg_desc* d = descs + blockIdx.y;
  if ((int)blockIdx.x >= d->idct_groups) return;                 // uniform: an image smaller than the batch's largest, or a refused one
  __shared__ int lds[DH_JPEG_IDCT_BLOCKS_PER_GROUP * JPEG_LDS_BLOCK_STRIDE];
  const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
  const long nb0 = (long)d->blocks_w[0] * d->blocks_h[0], nb1 = (long)d->blocks_w[1] * d->blocks_h[1], nb2 = (long)d->blocks_w[2] * d->blocks_h[2];
  const long b = (long)blockIdx.x * DH_JPEG_IDCT_BLOCKS_PER_GROUP + slot;
  const bool valid = b < nb0 + nb1 + nb2;
  const int c = b < nb0 ? 0 : (b < nb0 + nb1 ? 1 : 2);
  const long local = b - (c == 0 ? 0 : (c == 1 ? nb0 : nb0 + nb1));
  int x[8];
  if (valid) {
    const s16x8 v = *reinterpret_cast<const s16x8*>(coef + d->coef_offset + b * 64 + j * 8);        // column j, rows 0..7
    const uint16_t* q = d->quant[d->quant_index[c]];
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = (int)v[r] * (int)q[r * 8 + j];
    idct_islow_1d(x, 11);                                        // CONST_BITS - PASS1_BITS
#pragma unroll
    for (int r = 0; r < 8; ++r) lds[slot * JPEG_LDS_BLOCK_STRIDE + r * 8 + j] = x[r];
  }
  __syncthreads();
  if (valid) {
    const i32x4 lo = *reinterpret_cast<const i32x4*>(&lds[slot * JPEG_LDS_BLOCK_STRIDE + j * 8]);
    const i32x4 hi = *reinterpret_cast<const i32x4*>(&lds[slot * JPEG_LDS_BLOCK_STRIDE + j * 8 + 4]);
    x[0] = lo[0]; x[1] = lo[1]; x[2] = lo[2]; x[3] = lo[3]; x[4] = hi[0]; x[5] = hi[1]; x[6] = hi[2]; x[7] = hi[3];
    idct_islow_1d(x, 18);                                        // CONST_BITS + PASS1_BITS + 3
    unsigned w0 = 0, w1 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      w0 |= clamp255(x[k] + 128) << (8 * k);
      w1 |= clamp255(x[k + 4] + 128) << (8 * k);
    }
    const int bw = d->blocks_w[c];
    const long by = local / bw, bx = local - by * bw;
    uint8_t* p = ws + d->plane_offset[c] + (by * 8 + j) * ((long)bw * 8) + bx * 8;
    *reinterpret_cast<uint2*>(p) = make_uint2(w0, w1);
  }
}

// six chroma samples cx0-1 .. cx0+4 of one row, every index clamped to the component's own [0, cw-1]
__device__ __forceinline__ void chroma_row6(const uint8_t* __restrict__ row, int cx0, int cw, int t[6]) {
  const unsigned w = *reinterpret_cast<const unsigned*>(row + cx0);
  t[0] = row[max(cx0 - 1, 0)];
  t[1] = w & 255; t[2] = (w >> 8) & 255; t[3] = (w >> 16) & 255; t[4] = w >> 24;
  t[5] = row[min(cx0 + 4, cw - 1)];
#pragma unroll
  for (int k = 2; k < 6; ++k) t[k] = (cx0 + k - 1 > cw - 1) ? t[k - 1] : t[k];
}

__device__ __forceinline__ void unpack8(uint2 w, int v[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[k] = (w.x >> (8 * k)) & 255; v[k + 4] = (w.y >> (8 * k)) & 255; }
}

// 8 output samples x0 .. x0+7 of output row y of one chroma plane
__device__ __forceinline__ void chroma8(const danhip_jpeg_desc* d, const uint8_t* __restrict__ ws, int c, int y, int x0, int v[8]) {
  const uint8_t* plane = ws + d->plane_offset[c];
  const long pitch = (long)d->blocks_w[c] * 8;
  if (d->mode == DANHIP_JPEG_444) {
    unpack8(*reinterpret_cast<const uint2*>(plane + y * pitch + x0), v);
    return;
  }
  const int cx0 = x0 >> 1, cw = d->comp_w[c];
  if (cw <= 2) {                                                 // jdsample.c filters only a component more than 2 samples wide: replicate
    const uint8_t* row = plane + (d->mode == DANHIP_JPEG_420 ? y >> 1 : y) * pitch;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = row[min(cx0 + (k >> 1), cw - 1)];
    return;
  }
  int s[6];
  if (d->mode == DANHIP_JPEG_422) {                              // h2v1: (3 near + neighbour + 1 | 2) >> 2
    chroma_row6(plane + y * pitch, cx0, cw, s);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = (3 * s[i + 1] + s[i] + 1) >> 2;
      v[2 * i + 1] = (3 * s[i + 1] + s[i + 2] + 2) >> 2;
    }
    return;
  }
  const int cy = y >> 1, ch = d->comp_h[c];                      // h2v2: column sums 3 near + far, then (3 s + neighbour + 8 | 7) >> 4
  const int fy = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
  int f[6];
  chroma_row6(plane + cy * pitch, cx0, cw, s);
  chroma_row6(plane + fy * pitch, cx0, cw, f);
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = 3 * s[k] + f[k];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = (3 * s[i + 1] + s[i] + 8) >> 4;
    v[2 * i + 1] = (3 * s[i + 1] + s[i + 2] + 7) >> 4;
  }
}

__global__ __launch_bounds__(256) void jpeg_upsample_rgb_kernel(const danhip_jpeg_desc* __restrict__ descs, const uint8_t* __restrict__ ws,
                                                                uint8_t* __restrict__ out) {
  const danhip_jpeg_desc* d = descs + blockIdx.y;
  if ((int)blockIdx.x >= d->rgb_groups) return;
  const int W = d->width, H = d->height, per_row = (W + 7) >> 3;
  const long item = (long)blockIdx.x * DH_JPEG_RGB_ITEMS_PER_GROUP + threadIdx.x;
  if (item >= (long)H * per_row) return;
  const int y = (int)(item / per_row), x0 = (int)(item - (long)y * per_row) * 8;
  int Y[8], Cb[8], Cr[8];
  unpack8(*reinterpret_cast<const uint2*>(ws + d->plane_offset[0] + (long)y * ((long)d->blocks_w[0] * 8) + x0), Y);
  unsigned char px[24];
  if (d->mode == DANHIP_JPEG_GREY) {
#pragma unroll
    for (int k = 0; k < 8; ++k) px[3 * k] = px[3 * k + 1] = px[3 * k + 2] = (unsigned char)Y[k];
  } else {
    chroma8(d, ws, 1, y, x0, Cb);
    chroma8(d, ws, 2, y, x0, Cr);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int cb = Cb[k] - 128, cr = Cr[k] - 128;
      px[3 * k] = (unsigned char)clamp255(Y[k] + ((91881 * cr + 32768) >> 16));
      px[3 * k + 1] = (unsigned char)clamp255(Y[k] + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      px[3 * k + 2] = (unsigned char)clamp255(Y[k] + ((116130 * cb + 32768) >> 16));
    }
  }
  uint8_t* p = out + d->out_offset + ((long)y * W + x0) * 3;
  const int n = min(8, W - x0) * 3;
  if (n == 24 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
    unsigned w[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((unsigned)px[4 * k + 3] << 24);
    uint2* q = reinterpret_cast<uint2*>(p);
    q[0] = make_uint2(w[0], w[1]); q[1] = make_uint2(w[2], w[3]); q[2] = make_uint2(w[4], w[5]);
  } else {
#pragma unroll
    for (int k = 0; k < 24; ++k)
      if (k < n) p[k] = px[k];
  }
}

}  // namespace

extern "C" int danhip_jpeg_reconstruct_batch(const int16_t* coef_dev, int64_t coef_count, const danhip_jpeg_desc* descs_host,
                                             const danhip_jpeg_desc* descs_dev, int32_t B, uint8_t* out, int64_t out_bytes, void* workspace,
                                             size_t workspace_bytes, int32_t* launches, void* stream) {
  if (launches) *launches = 0;
  DH_REQUIRE(descs_host && descs_dev && B >= 1 && B <= 65535 && coef_count >= 0 && out_bytes >= 0, DANHIP_EINVAL,
             "jpeg_reconstruct_batch: bad arguments (1 <= B <= 65535, descriptors in host and device memory)");
  DH_REQUIRE(workspace_bytes < ((size_t)1 << 46), DANHIP_EINVAL, "jpeg_reconstruct_batch: workspace size out of range");
  DH_REQUIRE(workspace_bytes >= danhip_jpeg_workspace_bytes(descs_host, B), DANHIP_EWORKSPACE, "jpeg_reconstruct_batch: workspace too small");
  int max_idct = 0, max_rgb = 0;
  for (int32_t i = 0; i < B; ++i) {
    const danhip_jpeg_desc* d = descs_host + i;
    if (d->status) {
      DH_REQUIRE(d->idct_groups == 0 && d->rgb_groups == 0, DANHIP_EINVAL, "jpeg_reconstruct_batch: descriptor %d is refused (%d) but asks for work",
                 i, d->status);
      continue;
    }
    const char* why = dh_jpeg_desc_check(d, coef_count, out_bytes, (int64_t)workspace_bytes);
    if (why) {
      danhip_set_error("jpeg_reconstruct_batch: descriptor %d: %s", i, why);
      return DANHIP_EINVAL;
    }
    max_idct = d->idct_groups > max_idct ? d->idct_groups : max_idct;
    max_rgb = d->rgb_groups > max_rgb ? d->rgb_groups : max_rgb;
  }
  if (max_idct == 0) return DANHIP_OK;                           // nothing decodable: nothing is launched
  DH_REQUIRE(coef_dev && out && workspace, DANHIP_EINVAL, "jpeg_reconstruct_batch: NULL buffer");
  DH_REQUIRE(((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)descs_dev & 7) == 0, DANHIP_EINVAL,
             "jpeg_reconstruct_batch: coef_dev / workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)max_idct, (unsigned)B), dim3(256), 0, s, coef_dev, descs_dev, (uint8_t*)workspace);
  DH_LAUNCH_CHECK();
  if (launches) *launches = 1;
  hipLaunchKernelGGL(jpeg_upsample_rgb_kernel, dim3((unsigned)max_rgb, (unsigned)B), dim3(256), 0, s, descs_dev, (const uint8_t*)workspace, out);
  DH_LAUNCH_CHECK();
  if (launches) *launches = 2;
  return DANHIP_OK;
}
