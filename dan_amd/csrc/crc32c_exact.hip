// danhip_crc32c_batch: CRC-32C of n device byte ranges (any length, any byte alignment) in THREE launches whatever n and the sizes are.
//
// The remainder is linear over GF(2) (crc32c.h), so a range is cut into pieces whose raw remainders are shifted to the end of the range
// and XORed together in any order - integer XOR: the same bits whichever workgroup arrives first.
//   crc32c_plan_kernel   one workgroup: the exclusive prefix of the ranges' workgroup counts, accumulators zeroed.
//   crc32c_batch_kernel  the flat list of all ranges' windows, so ranges of very different sizes leave no workgroup idle.  A window is
//                        kGroup = 32 KiB of 16-byte ALIGNED memory lines (the first window of a range starts at its pointer rounded down),
//                        so every line inside the range is one whole-line 16-byte load, consecutive lanes on consecutive lines; only the
//                        two partial lines at the ends of a range are fetched byte by byte, and no byte outside the range is read.  The lines
//                        go to LDS; lane t then walks chunk t (kChunk = 128 bytes) out of LDS with 16-byte reads.  Chunks are 144 bytes apart
//                        there: 36 dwords, so the 16 lanes of a ds_read_b128 group fall on 16 different 4-bank slots (36 l mod 64 =
//                        4 (9 l mod 16)) - a 128-byte pitch would put all of them on one.  A lane's remainder is shifted to the end of the
//                        window's valid bytes (two table factors, x^(8*128*h) and x^(8*l)), the 256 values are XORed (wave shuffles, one
//                        LDS hop), wave 0 builds x^(8 * bytes behind the window) as a product over the set bits of that 64-bit count
//                        (lane i holds x^(8 * 2^i) or 1; six shuffle-multiply rounds) and one lane XORs the product into the range's
//                        word with an ordinary vector atomic.
//   crc32c_finish_kernel one lane per range: the init / final-xor term 0xFFFFFFFF * x^(8 len) ^ 0xFFFFFFFF, TensorFlow's mask on request.
// The walk has two forms, picked by option "crc_table": 1 (default) looks four bytes up in a 4 KiB slicing-by-4 table in LDS (data-dependent
// banks: lanes collide at random); 0 feeds every 32-bit word through 32 shift / conditional-xor steps (no memory access besides the data,
// ~32 VALU operations per byte).  Same bits either way.  Measured on the S3FD trainer's shard (131 ranges, 180 MB, one call): 0.16 ms =
// 1153 GB/s with the table, 0.24 ms = 764 GB/s without, beside 2.6 TB/s each way for a device copy of the same bytes: the walk is bound by
// LDS lookups / VALU work, not by HBM - and either is a twentieth of the 3.2 ms the image then takes over the host link
// (profiles/r16/checkpoint_crc.md).
#include "common.h"
#include "crc32c.h"

namespace {
using crc32c::kChunk;
using crc32c::kGroup;
constexpr int kThreads = 256;
constexpr int kPitch = kChunk + 16;                     // LDS bytes between two lanes' chunks
constexpr int kLinesPerLane = kGroup / 16 / kThreads;   // 8
constexpr int kPlanThreads = 256;
constexpr int kMaxSegments = 1 << 22;

__device__ const crc32c::Consts g_crc = crc32c::make_consts();

struct Layout {
  size_t table, prefix, acc, total;
};
Layout layout(int64_t n) {
  Layout l;
  l.table = 0;
  l.prefix = ((size_t)n * sizeof(danhip_crc_segment) + 15) & ~(size_t)15;
  l.acc = l.prefix + ((((size_t)n + 1) * 4 + 15) & ~(size_t)15);
  l.total = l.acc + (((size_t)n * 4 + 15) & ~(size_t)15);
  return l;
}

__host__ __device__ inline uint64_t seg_windows(const danhip_crc_segment& s) {
  if (s.bytes == 0) return 0;
  const uint64_t a = (uint64_t)(uintptr_t)s.ptr & 15u;
  return (a + s.bytes + kGroup - 1) / kGroup;
}

__global__ __launch_bounds__(kPlanThreads) void crc32c_plan_kernel(const danhip_crc_segment* __restrict__ tab, int n, uint32_t* __restrict__ prefix,
                                                                  uint32_t* __restrict__ acc) {
  __shared__ uint32_t part[kPlanThreads];
  const int t = threadIdx.x;
  const int per = (n + kPlanThreads - 1) / kPlanThreads;
  const int lo = min(n, t * per), hi = min(n, lo + per);
  uint32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += (uint32_t)seg_windows(tab[i]);
  part[t] = sum;
  __syncthreads();
  if (t == 0) {
    uint32_t run = 0;
    for (int i = 0; i < kPlanThreads; ++i) { const uint32_t v = part[i]; part[i] = run; run += v; }
    prefix[n] = run;
  }
  __syncthreads();
  uint32_t run = part[t];
  for (int i = lo; i < hi; ++i) {
    prefix[i] = run;
    acc[i] = 0;
    run += (uint32_t)seg_windows(tab[i]);
  }
}

__device__ __forceinline__ uint32_t word_shift(uint32_t c) {
#pragma unroll
  for (int i = 0; i < 32; ++i) c = (c >> 1) ^ (crc32c::kPoly & (0u - (c & 1u)));
  return c;
}

template <bool TABLE>
__global__ __launch_bounds__(kThreads) void crc32c_batch_kernel(const danhip_crc_segment* __restrict__ tab, int n, const uint32_t* __restrict__ prefix,
                                                               uint32_t* __restrict__ acc) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kThreads * kPitch];
  __shared__ uint32_t tbl[TABLE ? 4 * 256 : 1];
  __shared__ uint32_t wave_part[kThreads / 64];
  const int t = threadIdx.x;
  const uint32_t b = blockIdx.x;
  if (b >= prefix[n]) return;
  int s = 0;
  for (int hi = n; hi - s > 1;) {                        // the last range whose first window is <= b (ranges without windows are skipped)
    const int mid = (s + hi) >> 1;
    if (prefix[mid] <= b) s = mid; else hi = mid;
  }
  const uint8_t* ptr = (const uint8_t*)tab[s].ptr;
  const uint64_t bytes = tab[s].bytes;
  const uint32_t a = (uint32_t)((uintptr_t)ptr & 15u);
  const uint64_t w0 = (uint64_t)(b - prefix[s]) * kGroup;           // window start, counted from the aligned base ptr - a
  const uint8_t* win = ptr - a + w0;
  const int vs = w0 == 0 ? (int)a : 0;                               // valid bytes of the window: [vs, ve)
  const uint64_t left = a + bytes - w0;
  const int ve = left < (uint64_t)kGroup ? (int)left : kGroup;

  if (TABLE)
    for (int i = t; i < 4 * 256; i += kThreads) tbl[i] = g_crc.slice[i >> 8][i & 255];
  uint4 line[kLinesPerLane];
#pragma unroll
  for (int i = 0; i < kLinesPerLane; ++i) {
    const int p = (i * kThreads + t) * 16;
    line[i] = (p >= vs && p + 16 <= ve) ? *(const uint4*)(win + p) : make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < kLinesPerLane; ++i) {
    const int p = (i * kThreads + t) * 16;
    *(uint4*)(lds + (p / kChunk) * kPitch + (p % kChunk)) = line[i];
  }
  __syncthreads();
  if (t < 32) {                                          // the partial line at either end of the range, byte by byte
    const int p = (t < 16 ? (vs & ~15) : ((ve - 1) & ~15)) + (t & 15);
    const bool partial = t < 16 ? (vs & 15) != 0 || ve < (vs & ~15) + 16 : (ve & 15) != 0;
    if (partial && p >= vs && p < ve) lds[(p / kChunk) * kPitch + (p % kChunk)] = win[p];
  }
  __syncthreads();

  const int clo = max(vs, t * kChunk), chi = min(ve, (t + 1) * kChunk);
  uint32_t r = 0;
  const uint8_t* mine = lds + t * kPitch;
  if (clo == t * kChunk && chi == (t + 1) * kChunk) {
#pragma unroll
    for (int i = 0; i < kChunk / 16; ++i) {
      const uint4 v = *(const uint4*)(mine + 16 * i);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        r ^= w[k];
        if (TABLE) r = tbl[768 + (r & 255)] ^ tbl[512 + ((r >> 8) & 255)] ^ tbl[256 + ((r >> 16) & 255)] ^ tbl[r >> 24];
        else r = word_shift(r);
      }
    }
  } else {
    for (int p = clo; p < chi; ++p) r = crc32c::step_byte(r, mine[p - t * kChunk]);
  }
  if (clo < chi) {                                       // to the end of the window's valid bytes
    const int d = ve - chi;
    r = crc32c::mul(crc32c::mul(r, g_crc.chunk_pow[d / kChunk]), g_crc.byte_pow[d % kChunk]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r ^= __shfl_xor(r, o, 64);
  if ((t & 63) == 0) wave_part[t >> 6] = r;
  __syncthreads();
  if (t < 64) {
    const uint64_t behind = left - (uint64_t)ve;         // bytes of the range after this window
    uint32_t f = (behind >> t) & 1 ? g_crc.pow8[t] : crc32c::kOne;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f = crc32c::mul(f, __shfl_xor(f, o, 64));
    if (t == 0) {
      const uint32_t v = wave_part[0] ^ wave_part[1] ^ wave_part[2] ^ wave_part[3];
      atomicXor(&acc[s], crc32c::mul(v, f));
    }
  }
}

__global__ void crc32c_finish_kernel(const danhip_crc_segment* __restrict__ tab, int n, const uint32_t* __restrict__ acc, uint32_t* __restrict__ out,
                                     int masked) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t c = acc[i] ^ crc32c::mul(0xFFFFFFFFu, crc32c::pow_bytes(g_crc.pow8, tab[i].bytes)) ^ 0xFFFFFFFFu;
  out[i] = masked ? crc32c::mask(c) : c;
}

thread_local int g_last_launches = 0;
}  // namespace

extern "C" size_t danhip_crc_segment_bytes(void) { return sizeof(danhip_crc_segment); }
extern "C" int32_t danhip_crc32c_chunk_bytes(void) { return kChunk; }
extern "C" int32_t danhip_crc32c_group_bytes(void) { return kGroup; }
extern "C" int32_t danhip_crc32c_batch_last_launches(void) { return g_last_launches; }

extern "C" size_t danhip_crc32c_batch_workspace_bytes(int32_t n, uint64_t total_bytes) {
  (void)total_bytes;                                     // partial results are XORed into one word per range: nothing scales with the bytes
  if (n <= 0) return 0;
  return layout(n).total;
}

extern "C" int danhip_crc32c_batch(const danhip_crc_segment* table_host, int32_t n, uint32_t* crc_out_dev, int32_t masked, void* ws, size_t ws_bytes,
                                   void* stream) {
  g_last_launches = 0;
  DH_REQUIRE(n >= 0 && n <= kMaxSegments, DANHIP_EINVAL, "crc32c_batch: n=%d outside 0..%d", n, kMaxSegments);
  if (n == 0) return DANHIP_OK;
  DH_REQUIRE(table_host && crc_out_dev && ws, DANHIP_EINVAL, "crc32c_batch: null table, output or workspace");
  DH_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)crc_out_dev & 3) == 0, DANHIP_EINVAL, "crc32c_batch: workspace not 16-byte / output not 4-byte aligned");
  const Layout l = layout(n);
  DH_REQUIRE(ws_bytes >= l.total, DANHIP_EWORKSPACE, "crc32c_batch: workspace %zu bytes, %zu needed", ws_bytes, l.total);
  uint64_t windows = 0;
  for (int i = 0; i < n; ++i) {
    DH_REQUIRE(table_host[i].ptr || table_host[i].bytes == 0, DANHIP_EINVAL, "crc32c_batch: segment %d: null pointer with %llu bytes", i,
               (unsigned long long)table_host[i].bytes);
    DH_REQUIRE(table_host[i].bytes < (1ull << 60), DANHIP_EINVAL, "crc32c_batch: segment %d: %llu bytes", i, (unsigned long long)table_host[i].bytes);
    windows += seg_windows(table_host[i]);
    DH_REQUIRE(windows < (1ull << 31), DANHIP_EINVAL, "crc32c_batch: more than 2^31 windows of %d bytes", kGroup);
  }
  uint8_t* w = (uint8_t*)ws;
  const danhip_crc_segment* tab = (const danhip_crc_segment*)(w + l.table);
  uint32_t* prefix = (uint32_t*)(w + l.prefix);
  uint32_t* acc = (uint32_t*)(w + l.acc);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(crc32c_plan_kernel, dim3(1), dim3(kPlanThreads), 0, st, tab, (int)n, prefix, acc);
  DH_LAUNCH_CHECK();
  ++g_last_launches;
  // a grid of at least one workgroup keeps the launch count fixed; workgroups beyond the device table's own count leave at once
  const dim3 grid((unsigned)(windows ? windows : 1));
  if (danhip_option("crc_table"))
    hipLaunchKernelGGL(crc32c_batch_kernel<true>, grid, dim3(kThreads), 0, st, tab, (int)n, prefix, acc);
  else
    hipLaunchKernelGGL(crc32c_batch_kernel<false>, grid, dim3(kThreads), 0, st, tab, (int)n, prefix, acc);
  DH_LAUNCH_CHECK();
  ++g_last_launches;
  hipLaunchKernelGGL(crc32c_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, st, tab, (int)n, acc, crc_out_dev, (int)masked);
  DH_LAUNCH_CHECK();
  ++g_last_launches;
  return DANHIP_OK;
}
