// Test-time pipeline for images of DIFFERENT sizes (eval_dan.detect_image_list), compiled with -ffp-contract=off:
//   * resize_u8_linear_batch : every resized / mirrored copy of every image in ONE launch, through a device table of danhip_resize_item
//                              (filled and validated on the host by danhip_resize_item_init).  The pixel arithmetic is resize_u8.h's, the
//                              one danhip_resize_u8_linear uses.  A workgroup = one tile of 1024 consecutive output pixels of ONE item; the
//                              grid is the flat list of all items' tiles (per-item prefix first_tile), so no workgroup is empty however
//                              much the item sizes differ.
//   * detect_select          : the tail of one detection pass (detect_face's order + cut, the size filter, flip_test's mirror map) without
//                              sorting the A anchors: a three-digit (11 + 11 + 10 bit) radix select of the K-th largest score key, then the
//                              keys above it plus the highest-index ties of it, then a rank sort of those K <= 2048 in LDS.
//                              LAUNCHES PER CALL: 7, whatever A is (DANHIP_DETECT_SELECT_LAUNCHES): workspace zero-fill, three histogram
//                              passes, tie count per index chunk, collect, emit.
//                              Division: __fdiv_rn (IEEE round-to-nearest); the build passes no flag that relaxes fp32 division.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "common.h"
#include "resize_u8.h"

namespace {

// ------------------------------------------------------------------------------------------------- resize_u8_linear_batch
constexpr int kTilePix = 1024, kTileThreads = 256;

__global__ __launch_bounds__(kTileThreads) void resize_u8_linear_batch_kernel(const danhip_resize_item* __restrict__ tab, int n,
                                                                              const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
  int lo = 0, hi = n - 1;                                       // the last item with first_tile <= blockIdx.x (every item owns >= 1 tile)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].first_tile <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const danhip_resize_item it = tab[lo];
  const int lt = (int)blockIdx.x - it.first_tile;
  if (lt < 0 || lt >= it.tiles) return;                         // (uniform per workgroup: a table / grid mismatch does nothing)
  const long total = (long)it.Ho * it.Wo;
  const uint8_t* s = src + it.src_offset;
  uint8_t* d = dst + it.dst_offset;
#pragma unroll
  for (int k = 0; k < kTilePix / kTileThreads; ++k) {
    const long idx = (long)lt * kTilePix + k * kTileThreads + threadIdx.x;
    if (idx < total) {
      const int dx = (int)(idx % it.Wo), dy = (int)(idx / it.Wo);
      resize_u8_linear_pixel(s, it.pitch, it.H, it.W, 3, it.mirror != 0, it.scale_x, it.scale_y, dy, dx, d + idx * 3);
    }
  }
}

// ------------------------------------------------------------------------------------------------- detect_select
constexpr int SEL_THREADS = 256, SEL_MAX_GROUPS = 256, SEL_PER_GROUP = 2048, SEL_MAX_K = 2048, SEL_EMIT_THREADS = 1024;
constexpr int SEL_H1 = 0, SEL_H2 = 2048, SEL_H3 = 4096, SEL_STATE = 5120, SEL_ZERO_WORDS = 5136;      // workspace layout, 32-bit words
// state words: 0 number of collected candidates; 2, 3 first digit and the rank inside it; 4, 5 second digit, rank; 6, 7 the K-th key T and
// how many keys EQUAL to T belong to the K largest
constexpr int SEL_TIES = SEL_ZERO_WORDS;                        // tie_count[groups]
inline int sel_groups(long A) {
  long g = (A + SEL_PER_GROUP - 1) / SEL_PER_GROUP;
  return (int)(g < 1 ? 1 : (g > SEL_MAX_GROUPS ? SEL_MAX_GROUPS : g));
}
inline size_t sel_cand_offset(long A) { return ((size_t)(SEL_TIES + sel_groups(A)) * 4 + 15) / 16 * 16; }

// sort.hip's order-preserving image of a score (-0 = +0, every NaN one value above +inf): larger key = earlier in argsort_desc
__device__ __forceinline__ unsigned sel_key(float score) {
  unsigned b = __builtin_bit_cast(unsigned, score);
  if ((b << 1) == 0u) b = 0u;
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) b = 0x7FC00000u;
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

// The bin that holds the rank-th largest key (rank is 1-based) of a histogram of NB bins, and the rank inside that bin: bins are walked
// from the highest down.  All 256 threads call it; sh has 258 words.  rank <= the histogram's total (the callers' K <= A).
template <int NB>
__device__ __forceinline__ void sel_find(const unsigned* __restrict__ hist, unsigned rank, unsigned* sh, unsigned& digit, unsigned& newrank) {
  constexpr int PER = NB / SEL_THREADS;
  const int t = threadIdx.x;
  unsigned v[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) { v[i] = hist[NB - 1 - t * PER - i]; sum += v[i]; }
  sh[t] = sum;
  if (t == 0) { sh[256] = 0; sh[257] = 1; }
  __syncthreads();
  for (int off = 1; off < SEL_THREADS; off <<= 1) {
    const unsigned x = t >= off ? sh[t - off] : 0u;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const unsigned incl = sh[t], excl = incl - sum;
  if (excl < rank && rank <= incl) {                            // one thread
    unsigned c = excl;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (rank > c && rank <= c + v[i]) { sh[256] = (unsigned)(NB - 1 - t * PER - i); sh[257] = rank - c; }
      c += v[i];
    }
  }
  __syncthreads();
  digit = sh[256];
  newrank = sh[257];
  __syncthreads();
}

// PASS 0: histogram of key >> 21.  PASS 1: first digit from it, histogram of the next 11 bits among its keys.  PASS 2: second digit, histogram
// of the last 10 bits.  A workgroup counts in LDS and adds its non-empty bins to the workspace.
template <int PASS>
__global__ __launch_bounds__(SEL_THREADS) void sel_hist_kernel(const float* __restrict__ scores, int A, unsigned K, unsigned* __restrict__ ws) {
  __shared__ unsigned h[2048];
  __shared__ unsigned sh[258];
  unsigned prefix = 0;
  if (PASS == 1) {
    unsigned d, r;
    sel_find<2048>(ws + SEL_H1, K, sh, d, r);
    if (blockIdx.x == 0 && threadIdx.x == 0) { ws[SEL_STATE + 2] = d; ws[SEL_STATE + 3] = r; }
    prefix = d;
  } else if (PASS == 2) {
    unsigned d, r;
    sel_find<2048>(ws + SEL_H2, ws[SEL_STATE + 3], sh, d, r);
    if (blockIdx.x == 0 && threadIdx.x == 0) { ws[SEL_STATE + 4] = d; ws[SEL_STATE + 5] = r; }
    prefix = (ws[SEL_STATE + 2] << 11) | d;
  }
  for (int i = threadIdx.x; i < 2048; i += SEL_THREADS) h[i] = 0;
  __syncthreads();
  for (long i = (long)blockIdx.x * SEL_THREADS + threadIdx.x; i < A; i += (long)gridDim.x * SEL_THREADS) {
    const unsigned key = sel_key(scores[i]);
    if (PASS == 0) atomicAdd(&h[key >> 21], 1u);
    else if (PASS == 1) { if ((key >> 21) == prefix) atomicAdd(&h[(key >> 10) & 2047u], 1u); }
    else { if ((key >> 10) == prefix) atomicAdd(&h[key & 1023u], 1u); }
  }
  __syncthreads();
  unsigned* g = ws + (PASS == 0 ? SEL_H1 : (PASS == 1 ? SEL_H2 : SEL_H3));
  for (int i = threadIdx.x; i < (PASS == 2 ? 1024 : 2048); i += SEL_THREADS)
    if (h[i]) atomicAdd(&g[i], h[i]);
}

// The K-th key T and `need` (how many keys equal to T are among the K largest) from the third histogram; workgroup g counts the keys equal
// to T in ITS chunk of indices [g * chunk, (g + 1) * chunk).
__global__ __launch_bounds__(SEL_THREADS) void sel_ties_kernel(const float* __restrict__ scores, int A, int chunk, unsigned* __restrict__ ws) {
  __shared__ unsigned sh[258];
  unsigned d, need;
  sel_find<1024>(ws + SEL_H3, ws[SEL_STATE + 5], sh, d, need);
  const unsigned T = (ws[SEL_STATE + 2] << 21) | (ws[SEL_STATE + 4] << 10) | d;
  if (blockIdx.x == 0 && threadIdx.x == 0) { ws[SEL_STATE + 6] = T; ws[SEL_STATE + 7] = need; }
  const long lo = (long)blockIdx.x * chunk, hi = lo + chunk < A ? lo + chunk : A;
  unsigned c = 0;
  for (long i = lo + threadIdx.x; i < hi; i += SEL_THREADS) c += sel_key(scores[i]) == T ? 1u : 0u;
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int off = SEL_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[SEL_TIES + blockIdx.x] = sh[0];
}

// Every key above T, and of the keys equal to T the `need` with the highest indices: a chunk takes its ties from the top after the chunks
// behind it have taken theirs.  Candidates (key << 32 | index) are appended in any order: exactly K of them for finite scores.
__global__ __launch_bounds__(SEL_THREADS) void sel_collect_kernel(const float* __restrict__ scores, int A, int chunk, unsigned K,
                                                                  unsigned* __restrict__ ws, unsigned long long* __restrict__ cand) {
  __shared__ unsigned sh[SEL_THREADS];
  __shared__ unsigned wtot[SEL_THREADS / 64];
  const int t = threadIdx.x, g = blockIdx.x, G = gridDim.x;
  const unsigned T = ws[SEL_STATE + 6], need = ws[SEL_STATE + 7];
  sh[t] = (t > g && t < G) ? ws[SEL_TIES + t] : 0u;             // G <= SEL_MAX_GROUPS = SEL_THREADS
  __syncthreads();
  for (int off = SEL_THREADS / 2; off > 0; off >>= 1) {
    if (t < off) sh[t] += sh[t + off];
    __syncthreads();
  }
  const unsigned after = sh[0], mine = ws[SEL_TIES + g];
  const unsigned rest = after >= need ? 0u : need - after;
  const unsigned quota = rest < mine ? rest : mine;             // this chunk's ties to take: its `quota` highest indices
  const unsigned skip = mine - quota;                           // = all but its first `skip` ties in ascending index order
  const long lo = (long)g * chunk, hi = lo + chunk < A ? lo + chunk : A;
  unsigned running = 0;
  for (long base = lo; base < hi; base += SEL_THREADS) {
    const long i = base + t;
    const bool in = i < hi;
    const unsigned key = in ? sel_key(scores[i]) : 0u;
    const bool tie = in && key == T;
    bool take = in && key > T;
    if (quota > 0) {                                            // (uniform per workgroup)
      if (skip == 0) {
        take = take || tie;
      } else {
        const unsigned long long m = __ballot(tie);
        const int lane = t & 63, w = t >> 6;
        const unsigned before = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[w] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned wb = 0, tot = 0;
        for (int j = 0; j < SEL_THREADS / 64; ++j) { if (j < w) wb += wtot[j]; tot += wtot[j]; }
        if (tie && running + wb + before >= skip) take = true;
        running += tot;
        __syncthreads();
      }
    }
    if (take) {
      const unsigned pos = atomicAdd(&ws[SEL_STATE], 1u);
      if (pos < K) cand[pos] = ((unsigned long long)key << 32) | (unsigned)i;
    }
  }
}

// One workgroup: the candidates ordered by (key, index) descending through a rank sort in LDS (keys are unique), then row r of the output.
__global__ __launch_bounds__(SEL_EMIT_THREADS) void sel_emit_kernel(const unsigned long long* __restrict__ cand, const unsigned* __restrict__ ws,
                                                                    const float* __restrict__ boxes, const float* __restrict__ scores, int K,
                                                                    float shrink, int filter, float mirror_width, double* __restrict__ rows,
                                                                    uint8_t* __restrict__ valid) {
  __shared__ unsigned long long c[SEL_MAX_K];
  const unsigned got = ws[SEL_STATE];
  const int n = got < (unsigned)K ? (int)got : K;
  for (int i = threadIdx.x; i < n; i += SEL_EMIT_THREADS) c[i] = cand[i];
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += SEL_EMIT_THREADS) {
    const unsigned long long my = c[i];
    int r = 0;
    for (int j = 0; j < n; ++j) r += c[j] > my ? 1 : 0;
    const unsigned idx = (unsigned)(my & 0xFFFFFFFFull);
    const float* b = boxes + (size_t)idx * 4;                   // (ymin, xmin, ymax, xmax)
    float x0 = __fdiv_rn(b[1], shrink), y0 = __fdiv_rn(b[0], shrink), x2 = __fdiv_rn(b[3], shrink), y2 = __fdiv_rn(b[2], shrink);
    const float w = (x2 - x0) + 1.f, h = (y2 - y0) + 1.f;      // the filter sees the unmirrored row
    const bool ok = filter == 1 ? fmaxf(w, h) > 30.f : (filter == 2 ? fminf(w, h) < 100.f : true);
    if (mirror_width >= 0.f) {                                  // flip_test: x0' = (w - x2) - 1, x2' = (w - x0) - 1
      const float m0 = (mirror_width - x2) - 1.f, m2 = (mirror_width - x0) - 1.f;
      x0 = m0; x2 = m2;
    }
    double* o = rows + (size_t)r * 5;
    o[0] = (double)x0; o[1] = (double)y0; o[2] = (double)x2; o[3] = (double)y2; o[4] = (double)scores[idx];
    valid[r] = ok ? 1 : 0;
  }
  for (int r = n + threadIdx.x; r < K; r += SEL_EMIT_THREADS) {   // only when the precondition (finite scores) does not hold
    double* o = rows + (size_t)r * 5;
    o[0] = o[1] = o[2] = o[3] = o[4] = 0.;
    valid[r] = 0;
  }
}

int64_t item_tiles(const danhip_resize_item& it) { return ((int64_t)it.Ho * it.Wo + kTilePix - 1) / kTilePix; }

// what danhip_resize_item_init checks, on a finished item (the batch call repeats it on the host table)
const char* item_defect(const danhip_resize_item& it) {
  if (it.H <= 0 || it.W <= 0 || it.Ho <= 0 || it.Wo <= 0) return "non-positive size";
  if (!(it.fx > 0) || !(it.fy > 0) || !std::isfinite(it.fx) || !std::isfinite(it.fy)) return "fx / fy must be positive and finite";
  if ((double)it.Wo != std::rint((double)it.W * it.fx) || (double)it.Ho != std::rint((double)it.H * it.fy)) return "Ho / Wo are not rint(H * fy) / rint(W * fx)";
  if ((int64_t)it.pitch < 3 * (int64_t)it.W) return "pitch below 3 * W";
  if (it.mirror != 0 && it.mirror != 1) return "mirror is 0 or 1";
  if (it.src_offset < 0 || it.dst_offset < 0) return "negative offset";
  if (it.first_tile < 0 || it.tiles != item_tiles(it) || (int64_t)it.first_tile + it.tiles >= (1ll << 31)) return "tile prefix";
  return nullptr;
}

}  // namespace

static_assert(sizeof(danhip_resize_item) == 80, "danhip_resize_item layout");

extern "C" size_t danhip_resize_item_bytes(void) { return sizeof(danhip_resize_item); }

extern "C" int danhip_resize_item_init(danhip_resize_item* item, int64_t src_offset, int32_t H, int32_t W, int32_t pitch, int64_t dst_offset,
                                       int32_t Ho, int32_t Wo, double fx, double fy, int32_t mirror, int32_t first_tile, int32_t* tiles) {
  DH_REQUIRE(item && tiles, DANHIP_EINVAL, "resize_item_init: null pointer");
  danhip_resize_item it{};
  it.src_offset = src_offset; it.dst_offset = dst_offset;
  it.H = H; it.W = W; it.pitch = pitch; it.Ho = Ho; it.Wo = Wo; it.mirror = mirror;
  it.fx = fx; it.fy = fy;
  it.first_tile = first_tile;
  DH_REQUIRE(H > 0 && W > 0 && Ho > 0 && Wo > 0, DANHIP_EINVAL, "resize_item_init: non-positive size (%d x %d -> %d x %d)", H, W, Ho, Wo);
  const int64_t nt = item_tiles(it);
  DH_REQUIRE(nt < (1ll << 31), DANHIP_EINVAL, "resize_item_init: too many tiles");
  it.tiles = (int32_t)nt;
  const char* bad = item_defect(it);
  DH_REQUIRE(!bad, DANHIP_EINVAL, "resize_item_init: %s (H=%d W=%d pitch=%d Ho=%d Wo=%d fx=%g fy=%g)", bad, H, W, pitch, Ho, Wo, fx, fy);
  it.scale_x = 1. / fx;                                         // as danhip_resize_u8_linear passes them to its kernel
  it.scale_y = 1. / fy;
  *item = it;
  *tiles = it.tiles;
  return DANHIP_OK;
}

extern "C" int danhip_resize_u8_linear_batch(const danhip_resize_item* table_host, const danhip_resize_item* table_dev, int32_t n,
                                             const uint8_t* src, int64_t src_bytes, uint8_t* dst, int64_t dst_bytes, void* stream) {
  DH_REQUIRE(table_host && table_dev && src && dst && n > 0 && n <= 65535 && src_bytes > 0 && dst_bytes > 0, DANHIP_EINVAL,
             "resize_u8_linear_batch: bad arguments");
  int64_t total = 0;
  std::vector<std::pair<int64_t, int64_t>> ranges;              // destination [begin, end) of every item
  try {
    ranges.reserve(n);
  } catch (const std::bad_alloc&) {
    DH_REQUIRE(false, DANHIP_EINVAL, "resize_u8_linear_batch: out of host memory");
  }
  for (int i = 0; i < n; ++i) {
    const danhip_resize_item& it = table_host[i];
    const char* bad = item_defect(it);
    DH_REQUIRE(!bad, DANHIP_EINVAL, "resize_u8_linear_batch: item %d: %s", i, bad);
    DH_REQUIRE(it.scale_x == 1. / it.fx && it.scale_y == 1. / it.fy, DANHIP_EINVAL, "resize_u8_linear_batch: item %d was not filled by resize_item_init", i);
    DH_REQUIRE(it.first_tile == total, DANHIP_EINVAL, "resize_u8_linear_batch: item %d: first_tile %d, %lld expected", i, it.first_tile, (long long)total);
    total += it.tiles;
    DH_REQUIRE(total < (1ll << 31), DANHIP_EINVAL, "resize_u8_linear_batch: too many tiles");
    const int64_t src_end = it.src_offset + (int64_t)(it.H - 1) * it.pitch + 3 * (int64_t)it.W;
    const int64_t dst_end = it.dst_offset + 3 * (int64_t)it.Ho * it.Wo;
    DH_REQUIRE(src_end <= src_bytes, DANHIP_EINVAL, "resize_u8_linear_batch: item %d reads past the source buffer", i);
    DH_REQUIRE(dst_end <= dst_bytes, DANHIP_EINVAL, "resize_u8_linear_batch: item %d writes past the destination buffer", i);
    ranges.emplace_back(it.dst_offset, dst_end);
  }
  std::sort(ranges.begin(), ranges.end());
  for (int i = 1; i < n; ++i)
    DH_REQUIRE(ranges[i].first >= ranges[i - 1].second, DANHIP_EINVAL, "resize_u8_linear_batch: destination ranges of two items overlap at byte %lld",
               (long long)ranges[i].first);
  hipLaunchKernelGGL(resize_u8_linear_batch_kernel, dim3((unsigned)total), dim3(kTileThreads), 0, (hipStream_t)stream, table_dev, (int)n, src, dst);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" size_t danhip_detect_select_workspace_bytes(int64_t A) {
  if (A <= 0) return 0;
  return sel_cand_offset(A) + (size_t)SEL_MAX_K * sizeof(unsigned long long);
}

extern "C" int danhip_detect_select(const float* boxes, const float* scores, int32_t A, int32_t K, float shrink, int32_t filter, float mirror_width,
                                    double* rows, uint8_t* valid, void* workspace, size_t workspace_bytes, int32_t* launches, void* stream) {
  if (launches) *launches = 0;
  DH_REQUIRE(A > 0 && K >= 0 && K <= A && K <= SEL_MAX_K, DANHIP_EINVAL, "detect_select: A = %d, K = %d (0 <= K <= min(A, %d))", A, K, SEL_MAX_K);
  DH_REQUIRE(filter >= 0 && filter <= 2, DANHIP_EINVAL, "detect_select: filter is 0 (none), 1 (big) or 2 (small)");
  DH_REQUIRE(shrink > 0.f && std::isfinite(shrink) && !std::isnan(mirror_width), DANHIP_EINVAL, "detect_select: shrink must be positive and finite");
  if (K == 0) return DANHIP_OK;
  DH_REQUIRE(boxes && scores && rows && valid && workspace, DANHIP_EINVAL, "detect_select: null pointer");
  DH_REQUIRE(workspace_bytes >= danhip_detect_select_workspace_bytes(A), DANHIP_EWORKSPACE, "detect_select: workspace of %zu bytes, %zu needed",
             workspace_bytes, danhip_detect_select_workspace_bytes(A));
  hipStream_t s = (hipStream_t)stream;
  unsigned* ws = (unsigned*)workspace;
  unsigned long long* cand = (unsigned long long*)((char*)workspace + sel_cand_offset(A));
  const int G = sel_groups(A), chunk = cdiv(A, G);
  int count = 0;
  int rc = danhip_zero_async(workspace, (size_t)SEL_ZERO_WORDS * 4, s);
  if (rc) return rc;
  ++count;
  hipLaunchKernelGGL(sel_hist_kernel<0>, dim3(G), dim3(SEL_THREADS), 0, s, scores, A, (unsigned)K, ws);
  DH_LAUNCH_CHECK();
  ++count;
  hipLaunchKernelGGL(sel_hist_kernel<1>, dim3(G), dim3(SEL_THREADS), 0, s, scores, A, (unsigned)K, ws);
  DH_LAUNCH_CHECK();
  ++count;
  hipLaunchKernelGGL(sel_hist_kernel<2>, dim3(G), dim3(SEL_THREADS), 0, s, scores, A, (unsigned)K, ws);
  DH_LAUNCH_CHECK();
  ++count;
  hipLaunchKernelGGL(sel_ties_kernel, dim3(G), dim3(SEL_THREADS), 0, s, scores, A, chunk, ws);
  DH_LAUNCH_CHECK();
  ++count;
  hipLaunchKernelGGL(sel_collect_kernel, dim3(G), dim3(SEL_THREADS), 0, s, scores, A, chunk, (unsigned)K, ws, cand);
  DH_LAUNCH_CHECK();
  ++count;
  hipLaunchKernelGGL(sel_emit_kernel, dim3(1), dim3(SEL_EMIT_THREADS), 0, s, cand, ws, boxes, scores, K, shrink, filter, mirror_width, rows, valid);
  DH_LAUNCH_CHECK();
  ++count;
  static_assert(DANHIP_DETECT_SELECT_LAUNCHES == 7, "the documented launch count");
  if (launches) *launches = count;
  return DANHIP_OK;
}
