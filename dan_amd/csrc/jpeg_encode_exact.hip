// Device half of the JPEG encoder (include/danhip.h, "Baseline JPEG encode"): two launches per BATCH, each a (workgroup, image) grid
// through the descriptor table that danhip_jpeg_encode_prepare filled.  All integer, and every formula is a call into jpeg_encode.h, the
// text the host entry points run (jpeg_encode.cpp).
//   1 jpeg_enc_color_kernel  a lane takes 8 luma columns of one row (4:4:4) or of two rows (4:2:0): RGB -> YCbCr, the Y row(s) as 8-byte
//                            stores, chroma as 8 bytes per plane (4:4:4) or as the four h2v2 averages (4:2:0, one 4-byte store per plane).
//                            Source indices are clamped to the image, which replicates the right and bottom edges over the whole planes; the
//                            chroma rows below the component repeat ITS last row (two source rows of their own when the height is even).
//   2 jpeg_enc_fdct_kernel   eight lanes own a block, the lane shape of jpeg_idct_kernel: lane j loads ROW j of the block as one 8-byte
//                            load, level shift, the row pass in registers, the 8x8 transpose through LDS (block stride 68 dwords: the row
//                            writes are two 16-byte stores per lane, the column reads ds_read_b32 on banks 4 * block + j), the column pass, the
//                            reciprocal quantiser, and column j leaves as one 16-byte store in the decoder's column-major layout.  A dummy
//                            block (jpeg_encode.h) transforms the block it takes its DC from and stores zeros behind it.
#include "common.h"
#include "jpeg_encode.h"
#include "jpeg_layout.h"

// jpeg_encode.cpp: NULL = the descriptor is what (width, height, mode, quality) give and its offsets lie inside the buffers
extern "C" const char* danhip_jpeg_enc_desc_check(const danhip_jpeg_enc_desc* d, int64_t coef_count, int64_t workspace_bytes, int64_t file_bytes);

namespace {

typedef __attribute__((ext_vector_type(8))) short s16x8;
typedef __attribute__((ext_vector_type(4))) int i32x4;

#define JPEG_ENC_LDS_BLOCK_STRIDE 68

// 8 pixels of one row -> Y, Cb, Cr; row and columns clamped to the image
__device__ __forceinline__ void ycc_row8(const uint8_t* __restrict__ src, int W, int H, int y, int x0, int Y[8], int Cb[8], int Cr[8]) {
  const uint8_t* row = src + (long)min(y, H - 1) * W * 3;
  unsigned char px[24];
  const uint8_t* p = row + (long)x0 * 3;
  if (x0 + 8 <= W && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    const unsigned* q = reinterpret_cast<const unsigned*>(p);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const unsigned w = q[k];
      px[4 * k] = w & 255; px[4 * k + 1] = (w >> 8) & 255; px[4 * k + 2] = (w >> 16) & 255; px[4 * k + 3] = w >> 24;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint8_t* s = row + (long)min(x0 + k, W - 1) * 3;
      px[3 * k] = s[0]; px[3 * k + 1] = s[1]; px[3 * k + 2] = s[2];
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) dh_jenc_ycc(px[3 * k], px[3 * k + 1], px[3 * k + 2], &Y[k], &Cb[k], &Cr[k]);
}

__device__ __forceinline__ uint2 pack8(const int v[8]) {
  unsigned w0 = 0, w1 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { w0 |= (unsigned)v[k] << (8 * k); w1 |= (unsigned)v[k + 4] << (8 * k); }
  return make_uint2(w0, w1);
}

__global__ __launch_bounds__(256) void jpeg_enc_color_kernel(const danhip_jpeg_enc_desc* __restrict__ descs, uint8_t* __restrict__ ws) {
  const danhip_jpeg_enc_desc* d = descs + blockIdx.y;
  if ((int)blockIdx.x >= d->color_groups) return;                // uniform: an image smaller than the batch's largest
  const int W = d->width, H = d->height, bw0 = d->blocks_w[0];
  const bool sub = d->mode == DANHIP_JPEG_420;
  const int rows = d->blocks_h[0] * 8 / (sub ? 2 : 1);
  const long item = (long)blockIdx.x * 256 + threadIdx.x;
  if (item >= (long)rows * bw0) return;
  const int ry = (int)(item / bw0), x0 = (int)(item - (long)ry * bw0) * 8;
  const long pitch0 = (long)bw0 * 8;
  uint8_t* p0 = ws + d->plane_offset[0];
  uint8_t* p1 = ws + d->plane_offset[1];
  uint8_t* p2 = ws + d->plane_offset[2];
  int Y[8], Cb[2][8], Cr[2][8];
  if (!sub) {
    ycc_row8(d->src, W, H, ry, x0, Y, Cb[0], Cr[0]);
    *reinterpret_cast<uint2*>(p0 + ry * pitch0 + x0) = pack8(Y);
    *reinterpret_cast<uint2*>(p1 + ry * pitch0 + x0) = pack8(Cb[0]);       // 4:4:4: the three pitches are equal
    *reinterpret_cast<uint2*>(p2 + ry * pitch0 + x0) = pack8(Cr[0]);
    return;
  }
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    ycc_row8(d->src, W, H, 2 * ry + v, x0, Y, Cb[v], Cr[v]);
    *reinterpret_cast<uint2*>(p0 + (2 * ry + v) * pitch0 + x0) = pack8(Y);
  }
  const int cy = min(ry, d->comp_h[1] - 1);                      // below the component: its last row again
  if (cy != ry) {
#pragma unroll
    for (int v = 0; v < 2; ++v) ycc_row8(d->src, W, H, 2 * cy + v, x0, Y, Cb[v], Cr[v]);
  }
  unsigned wb = 0, wr = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int cx = (x0 >> 1) + i;
    wb |= (unsigned)dh_jenc_h2v2(Cb[0][2 * i], Cb[0][2 * i + 1], Cb[1][2 * i], Cb[1][2 * i + 1], cx) << (8 * i);
    wr |= (unsigned)dh_jenc_h2v2(Cr[0][2 * i], Cr[0][2 * i + 1], Cr[1][2 * i], Cr[1][2 * i + 1], cx) << (8 * i);
  }
  const long pitch1 = (long)d->blocks_w[1] * 8;
  *reinterpret_cast<unsigned*>(p1 + ry * pitch1 + (x0 >> 1)) = wb;
  *reinterpret_cast<unsigned*>(p2 + ry * pitch1 + (x0 >> 1)) = wr;
}

__global__ __launch_bounds__(256) void jpeg_enc_fdct_kernel(const danhip_jpeg_enc_desc* __restrict__ descs, const uint8_t* __restrict__ ws,
                                                            int16_t* __restrict__ coef) {
  const danhip_jpeg_enc_desc* d = descs + blockIdx.y;
  if ((int)blockIdx.x >= d->fdct_groups) return;
  __shared__ int lds[DH_JPEG_IDCT_BLOCKS_PER_GROUP * JPEG_ENC_LDS_BLOCK_STRIDE];
  const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
  const long nb0 = (long)d->blocks_w[0] * d->blocks_h[0], nb1 = (long)d->blocks_w[1] * d->blocks_h[1], nb2 = (long)d->blocks_w[2] * d->blocks_h[2];
  const long b = (long)blockIdx.x * DH_JPEG_IDCT_BLOCKS_PER_GROUP + slot;
  const bool valid = b < nb0 + nb1 + nb2;
  const int c = b < nb0 ? 0 : (b < nb0 + nb1 ? 1 : 2);
  const long local = b - (c == 0 ? 0 : (c == 1 ? nb0 : nb0 + nb1));
  int x[8];
  int dummy = 0;
  if (valid) {
    const int bw = d->blocks_w[c];
    const int by = (int)(local / bw), bx = (int)(local - (long)by * bw);
    int sy = by, sx = bx;
    if (c == 0) dummy = dh_jenc_block_source(by, bx, d->real_bw, d->real_bh, &sy, &sx);
    const uint2 w = *reinterpret_cast<const uint2*>(ws + d->plane_offset[c] + ((long)sy * 8 + j) * ((long)bw * 8) + (long)sx * 8);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = (int)((w.x >> (8 * k)) & 255) - 128;
      x[k + 4] = (int)((w.y >> (8 * k)) & 255) - 128;
    }
    dh_jenc_fdct_1d(x, 1);
    int* row = &lds[slot * JPEG_ENC_LDS_BLOCK_STRIDE + j * 8];
    *reinterpret_cast<i32x4*>(row) = i32x4{x[0], x[1], x[2], x[3]};
    *reinterpret_cast<i32x4*>(row + 4) = i32x4{x[4], x[5], x[6], x[7]};
  }
  __syncthreads();
  if (valid) {
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = lds[slot * JPEG_ENC_LDS_BLOCK_STRIDE + r * 8 + j];
    dh_jenc_fdct_1d(x, 0);
    const int t = c == 0 ? 0 : 1;
    s16x8 v;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int k = r * 8 + j;
      const int q = dh_jenc_quant(x[r], d->recip[t][k], d->corr[t][k], d->shift[t][k]);
      v[r] = (short)((dummy && k != 0) ? 0 : q);
    }
    *reinterpret_cast<s16x8*>(coef + d->coef_offset + b * 64 + j * 8) = v;       // column j, rows 0..7
  }
}

}  // namespace

extern "C" int danhip_jpeg_encode_pixels_batch(const danhip_jpeg_enc_desc* descs_host, const danhip_jpeg_enc_desc* descs_dev, int32_t B,
                                               int16_t* coef_dev, int64_t coef_count, void* workspace, size_t workspace_bytes, int32_t* launches,
                                               void* stream) {
  if (launches) *launches = 0;
  DH_REQUIRE(descs_host && descs_dev && B >= 1 && B <= 65535 && coef_count >= 0, DANHIP_EINVAL,
             "jpeg_encode_pixels_batch: bad arguments (1 <= B <= 65535, descriptors in host and device memory)");
  DH_REQUIRE(workspace_bytes < ((size_t)1 << 46), DANHIP_EINVAL, "jpeg_encode_pixels_batch: workspace size out of range");
  DH_REQUIRE(coef_dev && workspace, DANHIP_EINVAL, "jpeg_encode_pixels_batch: NULL buffer");
  DH_REQUIRE(((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)descs_dev & 7) == 0, DANHIP_EINVAL,
             "jpeg_encode_pixels_batch: coef_dev / workspace must be 16-byte aligned");
  int max_color = 0, max_fdct = 0;
  for (int32_t i = 0; i < B; ++i) {
    const danhip_jpeg_enc_desc* d = descs_host + i;
    const char* why = danhip_jpeg_enc_desc_check(d, coef_count, (int64_t)workspace_bytes, -1);
    if (!why && !d->src) why = "src is NULL";
    if (why) {
      danhip_set_error("jpeg_encode_pixels_batch: descriptor %d: %s", i, why);
      return DANHIP_EINVAL;
    }
    max_color = d->color_groups > max_color ? d->color_groups : max_color;
    max_fdct = d->fdct_groups > max_fdct ? d->fdct_groups : max_fdct;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(jpeg_enc_color_kernel, dim3((unsigned)max_color, (unsigned)B), dim3(256), 0, s, descs_dev, (uint8_t*)workspace);
  DH_LAUNCH_CHECK();
  if (launches) *launches = 1;
  hipLaunchKernelGGL(jpeg_enc_fdct_kernel, dim3((unsigned)max_fdct, (unsigned)B), dim3(256), 0, s, descs_dev, (const uint8_t*)workspace, coef_dev);
  DH_LAUNCH_CHECK();
  if (launches) *launches = 2;
  return DANHIP_OK;
}
