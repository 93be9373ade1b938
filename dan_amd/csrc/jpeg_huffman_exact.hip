// Huffman stage of the JPEG decoder on the device (include/danhip.h, "Huffman decoding on the device"): the self-synchronising parallel decoder
// over the staging buffer that danhip_jpeg_scan_prepare_batch packed.  All integer.  One workgroup per entry of the group table (256 lanes, one
// per subsequence of 128 stuffed bytes) or of the DC chunk table (one lane per MCU); the decoding itself is jpeg_huffman.h, shared with the
// host emulation.  5 + DANHIP_JPEG_SYNC_ROUNDS launches, whatever the data:
//   1     zero the coefficient buffer (danhip_zero_async)
//   2     jpeg_huff_sync_kernel, first = 1: every lane decodes its subsequence from state (0, 0) at its first bit and stores its exit; then
//         the group iterates "decode from the predecessor's exit if that differs from the entry I decoded from" around __syncthreads() until
//         no lane changed anything (at most one iteration per item).  A segment's first subsequence starts in the true state.
//   3..   the same kernel, first = 0, DANHIP_JPEG_SYNC_ROUNDS times: lane 0 of a group that starts inside a segment takes the previous group's
//         last exit as the launch before left it (two seam arrays, written and read in turn: no workgroup reads what another one writes in
//         the same launch, none waits for another).
//   n-2   jpeg_huff_write_kernel: segmented prefix sum of the completed-block counts (group-local scan + the tails of the groups before it in
//         the segment), one more decode of every subsequence from its final entry that stores the non-zero coefficients and the DC
//         differences and VERIFIES that it leaves where the stored exit says; the status bits of the image are set here.
//   n-1,n jpeg_dc_sum_kernel, jpeg_dc_apply_kernel: per-component DC prefix sum in scan order, reset at every segment (chunk totals, then
//         totals of the chunks before + a scan over the chunk's MCUs), int16 range and the block-energy bound.
// LDS of the Huffman kernels: the group's stream window (its items' bytes + 32 bytes of tail, 16-byte global loads) with 4 bytes of padding
// after every 128, so that the lanes' byte j - one subsequence apart - falls on banks 33 lanes apart instead of on one; the image's tables
// (at most 6 x 1424 bytes); the exits of the group.  48 KB in all.
#include "common.h"
#include "jpeg_huffman.h"
#include "jpeg_layout.h"

const char* dh_jpeg_scan_check(const void* staging, size_t staging_bytes, int32_t B, const danhip_jpeg_desc* descs, int64_t coef_count);

namespace {

#define HUFF_WIN_PHYS(o) ((o) + (((o) >> 7) << 2))
#define HUFF_WIN_WORDS ((DH_HUFF_WINDOW + (DH_HUFF_WINDOW / 128 + 1) * 4 + 3) / 4)

__device__ const uint8_t kZigColMajorDev[64] = {0,  8,  1,  2,  9,  16, 24, 17, 10, 3,  4,  11, 18, 25, 32, 40, 33, 26, 19, 12, 5,  6,
                                                13, 20, 27, 34, 41, 48, 56, 49, 42, 35, 28, 21, 14, 7,  15, 22, 29, 36, 43, 50, 57, 58,
                                                51, 44, 37, 30, 23, 31, 38, 45, 52, 59, 60, 53, 46, 39, 47, 54, 61, 62, 55, 63};

struct Tables {                    // the staging buffer's arrays on the device
  const DhScanHeader* h;
  const DhScanImage* images;
  const DhScanSeg* segs;
  const DhScanItem* items;
  const DhScanGroup* groups;
  const DhDcChunk* chunks;
  const DhHuffTab* tabs;
  const uint8_t* scan;
};

__device__ __forceinline__ Tables tables_of(const uint8_t* st) {
  const DhScanHeader* h = reinterpret_cast<const DhScanHeader*>(st);
  Tables t;
  t.h = h;
  t.images = reinterpret_cast<const DhScanImage*>(st + h->off_images);
  t.segs = reinterpret_cast<const DhScanSeg*>(st + h->off_segs);
  t.items = reinterpret_cast<const DhScanItem*>(st + h->off_items);
  t.groups = reinterpret_cast<const DhScanGroup*>(st + h->off_groups);
  t.chunks = reinterpret_cast<const DhDcChunk*>(st + h->off_chunks);
  t.tabs = reinterpret_cast<const DhHuffTab*>(st + h->off_tabs);
  t.scan = st + h->off_scan;
  return t;
}

struct DevCtx {                    // the context of jpeg_huffman.h over LDS (stream, tables) and the image's coefficient slot
  const uint8_t* win;
  const DhHuffTab* tabs;
  const uint8_t* zigt;
  int16_t* coef;
  int64_t coef_n;
  const danhip_jpeg_desc* desc;
  int32_t base, data_len;
  __device__ __forceinline__ uint32_t byte(int32_t i) const {
    if ((uint32_t)i >= (uint32_t)data_len) return 0;
    const uint32_t o = (uint32_t)(base + i);
    if (o >= (uint32_t)DH_HUFF_WINDOW) return 0;
    return win[HUFF_WIN_PHYS(o)];
  }
  __device__ __forceinline__ uint32_t look(int t, uint32_t i) const { return tabs[t].look[i & 511]; }
  __device__ __forceinline__ int32_t maxcode(int t, int l) const { return tabs[t].maxcode[l]; }
  __device__ __forceinline__ int32_t valoff(int t, int l) const { return tabs[t].valoff[l]; }
  __device__ __forceinline__ uint32_t sym(int t, int i) const { return tabs[t].sym[i & 255]; }
  __device__ __forceinline__ uint32_t zig(int k) const { return zigt[k & 63]; }
  __device__ __forceinline__ void store(int64_t blk, int el, int v) const {
    const int64_t i = blk * 64 + (el & 63);
    if ((uint64_t)i < (uint64_t)coef_n) coef[i] = (int16_t)v;
  }
  __device__ __forceinline__ int load(int64_t blk, int el) const {
    const int64_t i = blk * 64 + (el & 63);
    return (uint64_t)i < (uint64_t)coef_n ? (int)coef[i] : 0;
  }
  __device__ __forceinline__ uint32_t quant(int comp, int nat) const { return desc->quant[desc->quant_index[comp] & 3][nat & 63]; }
};

__device__ __forceinline__ DhBlockGeom geom_of(const DhScanImage* im) {
  DhBlockGeom g;
  g.bpm = im->bpm; g.nl = im->hs * im->vs; g.hs = im->hs; g.mcus_x = im->mcus_x;
  g.bw0 = im->blocks_w[0]; g.bw1 = im->blocks_w[1]; g.bw2 = im->blocks_w[2];
  g.plane0 = im->plane[0]; g.plane1 = im->plane[1]; g.plane2 = im->plane[2];
  g.total_blocks = im->total_blocks;
  return g;
}

// The group's stream window and its image's tables into LDS.  Only the part of the window the group's items (and the tail behind the last
// one) cover is loaded; a 16-byte load that would leave the scan area gives zeros.
__device__ __forceinline__ void stage_group(const Tables& T, const DhScanGroup& gr, const DhScanImage* im, uint32_t* win, uint32_t* tabs_lds) {
  const DhScanItem last = T.items[gr.first_item + gr.nitems - 1];
  const DhScanSeg* ls = T.segs + last.seg;
  int64_t end = im->scan_offset + ls->offset + (int64_t)last.sub * DH_HUFF_S + DH_HUFF_S + DH_HUFF_TAIL - gr.win_base;
  if (end > DH_HUFF_WINDOW) end = DH_HUFF_WINDOW;
  const int n16 = end < 0 ? 0 : (int)((end + 15) >> 4);
  const int64_t scan_bytes = T.h->scan_bytes;
  for (int i = threadIdx.x; i < n16; i += blockDim.x) {
    const int64_t at = gr.win_base + (int64_t)i * 16;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (at >= 0 && at + 16 <= scan_bytes) v = *reinterpret_cast<const uint4*>(T.scan + at);
    const uint32_t o = (uint32_t)i * 16;                          // 16 bytes never straddle a 128-byte row: one padding offset
    uint32_t* p = win + (HUFF_WIN_PHYS(o) >> 2);
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  }
  const uint32_t* src = reinterpret_cast<const uint32_t*>(T.tabs + im->tab_first);
  const int words = 2 * im->ncomp * (int)(sizeof(DhHuffTab) / 4);
  for (int i = threadIdx.x; i < words && i < 6 * (int)(sizeof(DhHuffTab) / 4); i += blockDim.x) tabs_lds[i] = src[i];
}

struct Lane {                      // what a lane knows about its item
  DhSub a;
  DevCtx c;
  int32_t sub, seg_items, first_mcu, mcu_count, final;
};

__device__ __forceinline__ Lane lane_of(const Tables& T, const DhScanGroup& gr, const DhScanImage* im, int item, const uint32_t* win, const uint32_t* tabs_lds,
                                        const uint8_t* zigt, int16_t* coef, const danhip_jpeg_desc* descs) {
  const DhScanItem x = T.items[item];
  const DhScanSeg* sg = T.segs + x.seg;
  Lane L;
  L.sub = x.sub; L.seg_items = sg->nitems; L.first_mcu = sg->first_mcu; L.mcu_count = sg->mcu_count; L.final = sg->final;
  L.a.start = x.sub * DH_HUFF_S;
  L.a.data_len = sg->data_len;
  L.a.end = min(L.a.start + DH_HUFF_S, sg->data_len);
  L.a.bpm = im->bpm; L.a.nl = im->hs * im->vs;
  L.c.win = reinterpret_cast<const uint8_t*>(win);
  L.c.tabs = reinterpret_cast<const DhHuffTab*>(tabs_lds);
  L.c.zigt = zigt;
  L.c.coef = coef ? coef + im->coef_offset : nullptr;
  L.c.coef_n = im->total_blocks * 64;
  L.c.desc = descs ? descs + gr.image : nullptr;
  L.c.base = (int32_t)(im->scan_offset + sg->offset - gr.win_base);
  L.c.data_len = sg->data_len;
  return L;
}

__global__ __launch_bounds__(256) void jpeg_huff_sync_kernel(const uint8_t* __restrict__ st, DhExit* __restrict__ ex, const int32_t* __restrict__ seam_in,
                                                             int32_t* __restrict__ seam_out, long long* __restrict__ tail, int32_t* __restrict__ status,
                                                             int first) {
  __shared__ uint32_t win[HUFF_WIN_WORDS];
  __shared__ uint32_t tabs_lds[6 * sizeof(DhHuffTab) / 4];
  __shared__ DhExit ex_l[DH_HUFF_G];
  __shared__ int s_head, s_sum;
  const Tables T = tables_of(st);
  const DhScanGroup gr = T.groups[blockIdx.x];
  const DhScanImage* im = T.images + gr.image;
  const int t = threadIdx.x;
  if (first && blockIdx.x == 0)
    for (int i = t; i < T.h->B; i += blockDim.x) status[i] = 0;
  if (t == 0) { s_head = 0; s_sum = 0; }
  stage_group(T, gr, im, win, tabs_lds);
  __syncthreads();
  const bool active = t < gr.nitems;
  Lane L = lane_of(T, gr, im, gr.first_item + (active ? t : 0), win, tabs_lds, nullptr, nullptr, nullptr);
  DhExit my = {0, 0, 0, 0};
  if (active) {
    if (first) my = dh_huff_decode_sub<DevCtx, false>(L.c, L.a, 0, nullptr, nullptr);
    else my = ex[gr.first_item + t];
    ex_l[t] = my;
  }
  __syncthreads();
  for (int iter = 0; iter < gr.nitems; ++iter) {                   // the bound: an iteration fixes at least one more item for good
    int changed = 0;
    if (active) {
      int32_t entry = 0;
      if (L.sub != 0) entry = t > 0 ? dh_huff_pack(ex_l[t - 1].off, ex_l[t - 1].state) : (first ? 0 : seam_in[blockIdx.x - 1]);
      if (entry != my.entry) {
        my = dh_huff_decode_sub<DevCtx, false>(L.c, L.a, entry, nullptr, nullptr);
        changed = 1;
      }
    }
    __syncthreads();                                               // every lane has read its predecessor's exit
    if (changed) ex_l[t] = my;
    if (!__syncthreads_or(changed)) break;
  }
  if (active) {
    ex[gr.first_item + t] = my;
    if (L.sub == 0) atomicMax(&s_head, t);
  }
  __syncthreads();
  if (active && t >= s_head) atomicAdd(&s_sum, my.n);              // blocks completed in the segment that runs on into the next group
  __syncthreads();
  if (t == 0) tail[blockIdx.x] = s_sum;
  if (t == gr.nitems - 1) seam_out[blockIdx.x] = dh_huff_pack(my.off, my.state);
}

__global__ __launch_bounds__(256) void jpeg_huff_write_kernel(const uint8_t* __restrict__ st, const DhExit* __restrict__ ex, const long long* __restrict__ tail,
                                                              int16_t* __restrict__ coef, int32_t* __restrict__ status) {
  __shared__ uint32_t win[HUFF_WIN_WORDS];
  __shared__ uint32_t tabs_lds[6 * sizeof(DhHuffTab) / 4];
  __shared__ int sv[DH_HUFF_G], sf[DH_HUFF_G];
  __shared__ int32_t s_entry[DH_HUFF_G];
  __shared__ uint8_t zigt[64];
  __shared__ unsigned long long s_carry;
  const Tables T = tables_of(st);
  const DhScanGroup gr = T.groups[blockIdx.x];
  const DhScanImage* im = T.images + gr.image;
  const int t = threadIdx.x;
  if (t < 64) zigt[t] = kZigColMajorDev[t];
  if (t == 0) s_carry = 0;
  stage_group(T, gr, im, win, tabs_lds);
  const bool active = t < gr.nitems;
  Lane L = lane_of(T, gr, im, gr.first_item + (active ? t : 0), win, tabs_lds, zigt, coef, nullptr);
  DhExit stored = {0, 0, 0, 0};
  if (active) stored = ex[gr.first_item + t];
  sv[t] = active ? stored.n : 0;
  sf[t] = active && L.sub == 0 ? 1 : 0;
  s_entry[t] = dh_huff_pack(stored.off, stored.state);
  __syncthreads();
  unsigned long long part = 0;                                     // tails of the groups before this one in the segment of its first item
  for (int k = gr.carry_from + t; k < (int)blockIdx.x; k += blockDim.x) part += (unsigned long long)tail[k];
  if (part) atomicAdd(&s_carry, part);
  for (int d = 1; d < DH_HUFF_G; d <<= 1) {                         // segmented inclusive scan of the block counts
    int v = sv[t], f = sf[t];
    if (t >= d && !f) { v += sv[t - d]; f = sf[t - d]; }
    __syncthreads();
    sv[t] = v; sf[t] = f;
    __syncthreads();
  }
  if (active) {
    int64_t before = 0;
    int32_t entry = 0;
    if (L.sub != 0) {
      before = t > 0 ? (int64_t)sv[t - 1] + (sf[t - 1] ? 0 : (int64_t)s_carry) : (int64_t)s_carry;
      if (t > 0) {
        entry = s_entry[t - 1];
      } else {
        const DhExit prev = ex[gr.first_item - 1];
        entry = dh_huff_pack(prev.off, prev.state);
      }
    }
    const DhBlockGeom g = geom_of(im);
    DhWrite w;
    w.cur = before; w.seg_blocks = (int64_t)L.mcu_count * im->bpm; w.first_block = (int64_t)L.first_mcu * im->bpm; w.final = L.final;
    const DhExit e = dh_huff_decode_sub<DevCtx, true>(L.c, L.a, entry, &g, &w);
    int bits = 0;
    if (!w.capped && (e.off != stored.off || e.state != stored.state || e.n != stored.n)) bits |= DANHIP_JPEG_DEV_NOTSYNC;
    if (w.error) bits |= DANHIP_JPEG_DEV_ERROR;
    if (L.sub == L.seg_items - 1 && before + stored.n < w.seg_blocks) bits |= DANHIP_JPEG_DEV_ERROR;      // the data end before the blocks do
    if (bits) atomicOr(status + gr.image, bits);
  }
}

__device__ __forceinline__ DevCtx dc_ctx(const DhScanImage* im, int image, int16_t* coef, const danhip_jpeg_desc* descs) {
  DevCtx c;
  c.win = nullptr; c.tabs = nullptr; c.zigt = nullptr;
  c.coef = coef + im->coef_offset;
  c.coef_n = im->total_blocks * 64;
  c.desc = descs + image;
  c.base = 0; c.data_len = 0;
  return c;
}

__global__ __launch_bounds__(DH_HUFF_DC_CHUNK) void jpeg_dc_sum_kernel(const uint8_t* __restrict__ st, int16_t* __restrict__ coef,
                                                                        const danhip_jpeg_desc* __restrict__ descs, long long* __restrict__ sums) {
  __shared__ unsigned long long s[3];
  const Tables T = tables_of(st);
  const DhDcChunk ck = T.chunks[blockIdx.x];
  const DhScanImage* im = T.images + ck.image;
  if (threadIdx.x < 3) s[threadIdx.x] = 0;
  __syncthreads();
  if ((int)threadIdx.x < ck.n) {
    DevCtx c = dc_ctx(im, ck.image, coef, descs);
    const DhBlockGeom g = geom_of(im);
    int64_t v[3];
    dh_dc_mcu_sum(c, g, (int64_t)T.segs[ck.seg].first_mcu + ck.mcu0 + threadIdx.x, v);
    for (int q = 0; q < 3; ++q)
      if (v[q]) atomicAdd(&s[q], (unsigned long long)v[q]);
  }
  __syncthreads();
  if (threadIdx.x < 3) sums[(long)blockIdx.x * 3 + threadIdx.x] = (long long)s[threadIdx.x];
}

__global__ __launch_bounds__(DH_HUFF_DC_CHUNK) void jpeg_dc_apply_kernel(const uint8_t* __restrict__ st, int16_t* __restrict__ coef,
                                                                          const danhip_jpeg_desc* __restrict__ descs, const long long* __restrict__ sums,
                                                                          int32_t* __restrict__ status) {
  __shared__ unsigned long long s_carry[3];
  __shared__ int sc[3][DH_HUFF_DC_CHUNK];
  const Tables T = tables_of(st);
  const DhDcChunk ck = T.chunks[blockIdx.x];
  const DhScanImage* im = T.images + ck.image;
  const int t = threadIdx.x;
  if (t < 3) s_carry[t] = 0;
  __syncthreads();
  unsigned long long part[3] = {0, 0, 0};                          // totals of the segment's chunks before this one
  for (int k = ck.chain_from + t; k < (int)blockIdx.x; k += blockDim.x)
    for (int q = 0; q < 3; ++q) part[q] += (unsigned long long)sums[(long)k * 3 + q];
  for (int q = 0; q < 3; ++q)
    if (part[q]) atomicAdd(&s_carry[q], part[q]);
  DevCtx c = dc_ctx(im, ck.image, coef, descs);
  const DhBlockGeom g = geom_of(im);
  const int64_t mcu = (int64_t)T.segs[ck.seg].first_mcu + ck.mcu0 + t;
  int64_t v[3] = {0, 0, 0};
  if (t < ck.n) dh_dc_mcu_sum(c, g, mcu, v);
  for (int q = 0; q < 3; ++q) sc[q][t] = (int)v[q];                 // at most 4 differences of 11 bits each: the chunk's sums stay far inside int32
  __syncthreads();
  for (int d = 1; d < DH_HUFF_DC_CHUNK; d <<= 1) {
    int a[3];
    for (int q = 0; q < 3; ++q) a[q] = sc[q][t] + (t >= d ? sc[q][t - d] : 0);
    __syncthreads();
    for (int q = 0; q < 3; ++q) sc[q][t] = a[q];
    __syncthreads();
  }
  if (t < ck.n) {
    int64_t pred[3];
    for (int q = 0; q < 3; ++q) pred[q] = (int64_t)s_carry[q] + sc[q][t] - v[q];
    if (dh_dc_mcu_apply(c, g, mcu, pred)) atomicOr(status + ck.image, DANHIP_JPEG_DEV_ERROR);
  }
}

}  // namespace

extern "C" int danhip_jpeg_huffman_decode_batch(const void* staging_host, const void* staging_dev, size_t staging_bytes, int32_t B, int16_t* coef_dev,
                                                int64_t coef_count, const danhip_jpeg_desc* descs_host, const danhip_jpeg_desc* descs_dev,
                                                void* workspace, size_t workspace_bytes, int32_t* status_dev, int32_t* launches, void* stream) {
  if (launches) *launches = 0;
  DH_REQUIRE(staging_host && descs_host && B >= 1 && B <= 65535 && coef_count >= 0, DANHIP_EINVAL,
             "jpeg_huffman_decode_batch: bad arguments (1 <= B <= 65535, staging buffer and descriptors in host and device memory)");
  const char* why = dh_jpeg_scan_check(staging_host, staging_bytes, B, descs_host, coef_count);
  if (why) {
    danhip_set_error("jpeg_huffman_decode_batch: %s", why);
    return DANHIP_EINVAL;
  }
  const DhScanHeader* h = (const DhScanHeader*)staging_host;
  if (h->ngroups == 0) return DANHIP_OK;                           // no image is prepared: nothing is launched
  DH_REQUIRE(workspace_bytes >= danhip_jpeg_scan_workspace_bytes(staging_host), DANHIP_EWORKSPACE, "jpeg_huffman_decode_batch: workspace too small");
  DH_REQUIRE(staging_dev && coef_dev && descs_dev && workspace && status_dev, DANHIP_EINVAL, "jpeg_huffman_decode_batch: NULL buffer");
  DH_REQUIRE(((uintptr_t)staging_dev & 15) == 0 && ((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)descs_dev & 7) == 0 &&
                 ((uintptr_t)status_dev & 3) == 0,
             DANHIP_EINVAL, "jpeg_huffman_decode_batch: staging_dev / coef_dev / workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  uint8_t* wsp = (uint8_t*)workspace;
  const size_t a = 15;
  DhExit* ex = (DhExit*)wsp;
  wsp += ((size_t)h->nitems * 16 + a) & ~a;
  int32_t* seam = (int32_t*)wsp;
  wsp += ((size_t)h->ngroups * 8 + a) & ~a;
  long long* tail = (long long*)wsp;
  wsp += ((size_t)h->ngroups * 8 + a) & ~a;
  long long* sums = (long long*)wsp;
  const uint8_t* st = (const uint8_t*)staging_dev;
  int n = 0;
  int rc = danhip_zero_async(coef_dev, (size_t)coef_count * 2, s);
  if (rc != DANHIP_OK) return rc;
  if (launches) *launches = ++n;
  for (int r = 0; r <= DANHIP_JPEG_SYNC_ROUNDS; ++r) {
    hipLaunchKernelGGL(jpeg_huff_sync_kernel, dim3((unsigned)h->ngroups), dim3(DH_HUFF_G), 0, s, st, ex, seam + ((r + 1) & 1) * h->ngroups,
                       seam + (r & 1) * h->ngroups, tail, status_dev, r == 0 ? 1 : 0);
    DH_LAUNCH_CHECK();
    if (launches) *launches = ++n;
  }
  hipLaunchKernelGGL(jpeg_huff_write_kernel, dim3((unsigned)h->ngroups), dim3(DH_HUFF_G), 0, s, st, ex, tail, coef_dev, status_dev);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  hipLaunchKernelGGL(jpeg_dc_sum_kernel, dim3((unsigned)h->nchunks), dim3(DH_HUFF_DC_CHUNK), 0, s, st, coef_dev, descs_dev, sums);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  hipLaunchKernelGGL(jpeg_dc_apply_kernel, dim3((unsigned)h->nchunks), dim3(DH_HUFF_DC_CHUNK), 0, s, st, coef_dev, descs_dev, sums, status_dev);
  DH_LAUNCH_CHECK();
  if (launches) *launches = ++n;
  return DANHIP_OK;
}
