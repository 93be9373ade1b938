// WIDER FACE average precision on the device (include/danhip.h, "WIDER FACE evaluation"), compiled with -ffp-contract=off.  The protocol's
// decisions are all comparisons of IEEE doubles computed in a fixed order, so every kernel here is exact; the curve is summed in integers.
//   * wider_quantize    : what eval_dan.py:write_to_txt does to a row (size / score filters, floor / ceil, '{:.3f}' of the score) + compaction
//                         into the image's slot of the detection store; one workgroup per image, ballot prefix, order preserved.
//   * wider_score_range : step 1's (lo, hi) over every stored score; two launches (per-block partials, then one block), no atomics.
//   * wider_eval        : steps 2-4; a persistent grid, one workgroup per image at a time, every subset in the same pass:
//                           rank sort on (normalised score desc, index asc)  ->  first arg-max overlap per detection over LDS tiles of boxes
//                           ->  "first detection that selects box j" by an LDS atomicMin per box  ->  per subset a block prefix sum of
//                           (new recall, proposal == 1) packed in one int  ->  one binary search per threshold.
//                         A workgroup adds into its own uint32 partial curve (thread t owns threshold t: no atomics, no barrier).
//   * wider_ap          : partial curves -> int64 curve (one launch), then precision / recall / envelope / AP, one workgroup per subset.
// No floating-point atomics anywhere; the integer sums make the result the same bits whatever the order of the images.
#include <limits.h>

#include "common.h"

namespace {

constexpr int kQuantThreads = 256;
constexpr int kEvalThreads = 1024;
constexpr int kMaxDets = DANHIP_WIDER_MAX_DETS;                    // detections of one image the match kernel holds in LDS
constexpr int kPer = kMaxDets / kEvalThreads;                      // sorted detections per thread (consecutive: h = tid * kPer + u)
constexpr int kBoxTile = 512;                                      // ground-truth boxes per LDS tile (any number of boxes: tiles are looped)
constexpr int kMaxBlocks = 512;                                    // persistent workgroups of wider_eval = partial curves
constexpr int kRangeBlocks = 256;
constexpr int kMaxImages = 1 << 20;                                // I * kMaxDets < 2^31: a uint32 partial curve cannot overflow
constexpr int kApThreads = 256;
static_assert(kMaxDets % kEvalThreads == 0 && kBoxTile * 4 <= kMaxDets, "box tile aliases the unsorted score buffer");

inline int eval_blocks(int I) { return I < kMaxBlocks ? (I < 1 ? 1 : I) : kMaxBlocks; }

__device__ __forceinline__ double shfl_down_f64(double v, int off) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_down(lo, off);
  hi = __shfl_down(hi, off);
  return __hiloint2double(hi, lo);
}

// ------------------------------------------------------------------------------------------------- quantize + compact
// dets [B, Nmax, 5] (T = float: rows (xmin, ymin, xmax, ymax, score); quantize == 0: rows (x, y, w, h, score) of either type, kept as they
// are).  Image image_index[b] gets its surviving rows, in order, at store_rows[image_index[b] * cap ...] and their number in store_counts.
template <typename T>
__global__ void __launch_bounds__(kQuantThreads) wider_quantize_kernel(const T* __restrict__ dets, const int* __restrict__ num,
                                                                       const int* __restrict__ image_index, int Nmax, int quantize,
                                                                       double* __restrict__ store_rows, int* __restrict__ store_counts, int I, int cap,
                                                                       int* __restrict__ status) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int img = image_index[b];
  if (img < 0 || img >= I) {                                       // uniform per workgroup
    if (tid == 0) atomicOr(status, DANHIP_WIDER_EINDEX);
    return;
  }
  int n = num[b];
  n = n < 0 ? 0 : (n > Nmax ? Nmax : n);
  const T* src = dets + (long)b * Nmax * 5;
  double* dst = store_rows + (long)img * cap * 5;
  __shared__ int s_wave[kQuantThreads / 64];
  int base = 0;
  for (int k0 = 0; k0 < n; k0 += kQuantThreads) {
    const int k = k0 + tid;
    bool keep = false;
    double r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
    if (k < n) {
      if (quantize) {                                              // eval_dan.py:write_to_txt, fp32 as numpy evaluates it
        const float xmin = (float)src[k * 5], ymin = (float)src[k * 5 + 1], xmax = (float)src[k * 5 + 2], ymax = (float)src[k * 5 + 3];
        const float sc = (float)src[k * 5 + 4];
        const float bw = xmax - xmin + 1.f, bh = ymax - ymin + 1.f;
        keep = ceilf(bh) >= 10.f && bw > 1.f && sc > 0.01f;
        r0 = floorf(xmin); r1 = floorf(ymin); r2 = ceilf(bw); r3 = ceilf(bh);
        r4 = rint((double)sc * 1000.0) / 1000.0;                   // '{:.3f}' read back: sc * 1000 is exact in double, rint = half to even
      } else {
        keep = true;
        r0 = (double)src[k * 5]; r1 = (double)src[k * 5 + 1]; r2 = (double)src[k * 5 + 2]; r3 = (double)src[k * 5 + 3]; r4 = (double)src[k * 5 + 4];
      }
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[wid] = __popcll(m);
    __syncthreads();
    int off = base, total = 0;
    for (int w = 0; w < kQuantThreads / 64; ++w) {
      if (w < wid) off += s_wave[w];
      total += s_wave[w];
    }
    off += __popcll(m & ((1ull << lane) - 1ull));
    if (keep && off < cap) {
      double* o = dst + (long)off * 5;
      o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    const int old = atomicExch(&store_counts[img], base < cap ? base : cap);
    if (old != -1) atomicOr(status, DANHIP_WIDER_ETWICE);
    if (base > cap) atomicOr(status, DANHIP_WIDER_ECOUNT);
  }
}

// ------------------------------------------------------------------------------------------------- score range
__device__ __forceinline__ void range_block_reduce(double lo, double hi, double* s_lo, double* s_hi, double* out) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int off = 32; off > 0; off >>= 1) {
    lo = fmin(lo, shfl_down_f64(lo, off));
    hi = fmax(hi, shfl_down_f64(hi, off));
  }
  if (lane == 0) { s_lo[wid] = lo; s_hi[wid] = hi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < (int)blockDim.x / 64; ++w) { lo = fmin(lo, s_lo[w]); hi = fmax(hi, s_hi[w]); }
    out[0] = lo; out[1] = hi;
  }
}

__global__ void __launch_bounds__(256) wider_range_partial_kernel(const double* __restrict__ rows, long D, double* __restrict__ part) {
  __shared__ double s_lo[4], s_hi[4];
  double lo = INFINITY, hi = -INFINITY;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < D; i += (long)gridDim.x * 256) {
    const double s = rows[i * 5 + 4];
    lo = fmin(lo, s); hi = fmax(hi, s);
  }
  range_block_reduce(lo, hi, s_lo, s_hi, part + 2 * blockIdx.x);
}

__global__ void __launch_bounds__(256) wider_range_final_kernel(const double* __restrict__ part, int nparts, long D, double* __restrict__ range) {
  __shared__ double s_lo[4], s_hi[4];
  double lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nparts; i += 256) { lo = fmin(lo, part[2 * i]); hi = fmax(hi, part[2 * i + 1]); }
  if (D == 0) lo = hi = 0.0;                                       // no detection at all: nothing is normalised
  range_block_reduce(lo, hi, s_lo, s_hi, range);
}

// ------------------------------------------------------------------------------------------------- match + sweep
struct EvalArgs {
  const int* det_offsets; const double* det_rows; const int* gt_offsets; const double* gt_boxes; const uint8_t* gt_keep; const double* range;
  int I, S, T; long D, G; double iou_thr; uint32_t* partial; int* status;
};

__global__ void __launch_bounds__(kEvalThreads) wider_eval_kernel(EvalArgs a) {
  __shared__ double s_a[kMaxDets];          // normalised scores by original index; then the box tile [kBoxTile][4] as corners
  __shared__ double s_score[kMaxDets];      // normalised scores in evaluation order (descending)
  __shared__ int s_b[kMaxDets];             // evaluation order -> original index; then the packed prefix sums
  __shared__ int s_hit[kBoxTile];           // first detection (evaluation order) that selects a box of the tile with overlap >= threshold
  __shared__ int s_wsum[kEvalThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int S = a.S, T = a.T;
  uint32_t* part = a.partial + (long)blockIdx.x * S * T * 2;
  for (int s = 0; s < S; ++s)
    for (int t = tid; t < T; t += kEvalThreads) { part[((long)s * T + t) * 2] = 0; part[((long)s * T + t) * 2 + 1] = 0; }   // thread t owns threshold t for good
  const double lo = a.range[0], hi = a.range[1];
  const double span = hi - lo;
  for (int img = blockIdx.x; img < a.I; img += gridDim.x) {
    const long d0 = a.det_offsets[img], g0 = a.gt_offsets[img];
    const long nl = (long)a.det_offsets[img + 1] - d0, ml = (long)a.gt_offsets[img + 1] - g0;
    if (nl < 0 || ml < 0 || d0 < 0 || g0 < 0 || d0 + nl > a.D || g0 + ml > a.G) {                      // (all uniform per workgroup)
      if (tid == 0) atomicOr(a.status, DANHIP_WIDER_EOFFSETS);
      continue;
    }
    if (nl > kMaxDets) {
      if (tid == 0) atomicOr(a.status, DANHIP_WIDER_ECOUNT);
      continue;
    }
    const int n = (int)nl, m = (int)ml;
    if (n == 0 || m == 0) continue;                               // step 3: such an image adds to count_face only (wider_ap counts every box)
    const double* rows = a.det_rows + d0 * 5;
    __syncthreads();                                               // the previous image's sweep has read s_score / s_b
    for (int k = tid; k < n; k += kEvalThreads) s_a[k] = span == 0.0 ? 0.0 : (rows[(long)k * 5 + 4] - lo) / span;       // step 1
    __syncthreads();
    for (int k = tid; k < n; k += kEvalThreads) {                 // step 2: rank = detections that come before k (stable)
      const double sk = s_a[k];
      int rank = 0;
      for (int q = 0; q < n; ++q) {
        const double sq = s_a[q];
        rank += (sq > sk || (sq == sk && q < k)) ? 1 : 0;
      }
      s_b[rank] = k;
      s_score[rank] = sk;
    }
    __syncthreads();
    // step 3a: first arg-max of the overlap with every box, for detections h = tid * kPer + u
    double bx1[kPer], by1[kPer], bx2[kPer], by2[kPer], barea[kPer], best[kPer];
    int bj[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int h = tid * kPer + u;
      best[u] = -1.0; bj[u] = 0;
      bx1[u] = by1[u] = bx2[u] = by2[u] = barea[u] = 0.0;
      if (h < n) {
        const double* r = rows + (long)s_b[h] * 5;
        bx1[u] = r[0]; by1[u] = r[1]; bx2[u] = r[0] + r[2]; by2[u] = r[1] + r[3];
        barea[u] = (bx2[u] - bx1[u] + 1) * (by2[u] - by1[u] + 1);
      }
    }
    for (int j0 = 0; j0 < m; j0 += kBoxTile) {
      const int tm = m - j0 < kBoxTile ? m - j0 : kBoxTile;
      __syncthreads();                                             // s_a free (rank sort / previous tile done)
      for (int j = tid; j < tm; j += kEvalThreads) {
        const double* q = a.gt_boxes + (g0 + j0 + j) * 4;
        s_a[j * 4] = q[0]; s_a[j * 4 + 1] = q[1]; s_a[j * 4 + 2] = q[0] + q[2]; s_a[j * 4 + 3] = q[1] + q[3];
      }
      __syncthreads();
      for (int j = 0; j < tm; ++j) {
        const double qx1 = s_a[j * 4], qy1 = s_a[j * 4 + 1], qx2 = s_a[j * 4 + 2], qy2 = s_a[j * 4 + 3];
        const double qarea = (qx2 - qx1 + 1) * (qy2 - qy1 + 1);
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
          const double iw = fmin(bx2[u], qx2) - fmax(bx1[u], qx1) + 1, ih = fmin(by2[u], qy2) - fmax(by1[u], qy1) + 1;
          double o = 0.0;
          if (iw > 0 && ih > 0) {
            const double inter = iw * ih;
            o = inter / (barea[u] + qarea - inter);
          }
          if (o > best[u]) { best[u] = o; bj[u] = j0 + j; }        // strict: the first maximum wins, across tiles too
        }
      }
    }
    // step 3b: the walk's state.  recall[j] turns 1 at the FIRST detection that selects j (subset-independent; whether j is kept decides
    // what that means), so: an LDS atomicMin per box, tile by tile
    bool matched[kPer], first[kPer];
    int keepbits[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      matched[u] = tid * kPer + u < n && best[u] >= a.iou_thr;
      first[u] = false;
      keepbits[u] = matched[u] ? a.gt_keep[g0 + bj[u]] : 0;
    }
    for (int j0 = 0; j0 < m; j0 += kBoxTile) {
      __syncthreads();
      for (int j = tid; j < kBoxTile; j += kEvalThreads) s_hit[j] = INT_MAX;
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kPer; ++u)
        if (matched[u] && bj[u] >= j0 && bj[u] < j0 + kBoxTile) atomicMin(&s_hit[bj[u] - j0], tid * kPer + u);
      __syncthreads();
#pragma unroll
      for (int u = 0; u < kPer; ++u)
        if (matched[u] && bj[u] >= j0 && bj[u] < j0 + kBoxTile) first[u] = s_hit[bj[u] - j0] == tid * kPer + u;
    }
    // step 3c + 4 per subset: low half = pred_recall, high half = #{proposal == 1}, both inclusive prefix sums over the evaluation order
    for (int s = 0; s < S; ++s) {
      int c[kPer], run = 0;
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const bool kept = (keepbits[u] >> s) & 1;
        const int newrec = (first[u] && kept) ? 1 : 0;
        const int prop = (tid * kPer + u < n && !(matched[u] && !kept)) ? 1 : 0;
        run += newrec | (prop << 16);
        c[u] = run;
      }
      int incl = run;
      for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off);
        if (lane >= off) incl += v;
      }
      __syncthreads();                                             // previous subset's sweep has read s_b; s_wsum free
      if (lane == 63) s_wsum[wid] = incl;
      __syncthreads();
      int before = incl - run;
      for (int w = 0; w < wid; ++w) before += s_wsum[w];
#pragma unroll
      for (int u = 0; u < kPer; ++u)
        if (tid * kPer + u < n) s_b[tid * kPer + u] = before + c[u];
      __syncthreads();
      for (int t = tid; t < T; t += kEvalThreads) {
        const double thr = 1.0 - (double)(t + 1) / (double)T;
        int l = 0, r = n;                                          // number of scores >= thr (descending order)
        while (l < r) {
          const int mid = (l + r) >> 1;
          if (s_score[mid] >= thr) l = mid + 1; else r = mid;
        }
        if (l > 0) {
          const int v = s_b[l - 1];
          part[((long)s * T + t) * 2] += (uint32_t)(v >> 16);
          part[((long)s * T + t) * 2 + 1] += (uint32_t)(v & 0xffff);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------- curve + AP
__global__ void __launch_bounds__(256) wider_curve_reduce_kernel(const uint32_t* __restrict__ partial, int nparts, long entries, int64_t* __restrict__ curves) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= entries) return;
  int64_t sum = 0;
  for (int p = 0; p < nparts; ++p) sum += partial[(long)p * entries + e];
  curves[e] = sum;
}

// one workgroup per subset; mrec / mpre of step 5 in LDS (T + 2 doubles each)
__global__ void __launch_bounds__(kApThreads) wider_ap_kernel(const int64_t* __restrict__ curves, const uint8_t* __restrict__ gt_keep, long G, int T,
                                                             int64_t* __restrict__ count_face, double* __restrict__ precision, double* __restrict__ recall,
                                                             double* __restrict__ ap) {
  __shared__ double s_rec[DANHIP_WIDER_MAX_THRESHOLDS + 2], s_pre[DANHIP_WIDER_MAX_THRESHOLDS + 2];
  __shared__ unsigned long long s_count;
  const int s = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_count = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (long g = tid; g < G; g += kApThreads) mine += (gt_keep[g] >> s) & 1;
  atomicAdd(&s_count, mine);                                       // integer, LDS
  __syncthreads();
  const int64_t faces = (int64_t)s_count;
  const int64_t* cv = curves + (long)s * T * 2;
  for (int t = tid; t < T; t += kApThreads) {
    const int64_t c0 = cv[t * 2], c1 = cv[t * 2 + 1];
    const double p = c0 == 0 ? 0.0 : (double)c1 / (double)c0;      // curve[t][0] == 0 implies curve[t][1] == 0: 0 by definition
    const double r = faces == 0 ? 0.0 : (double)c1 / (double)faces;
    precision[(long)s * T + t] = p;
    recall[(long)s * T + t] = r;
    s_pre[t + 1] = p;
    s_rec[t + 1] = r;
  }
  if (tid == 0) { s_rec[0] = 0.0; s_pre[0] = 0.0; s_rec[T + 1] = 1.0; s_pre[T + 1] = 0.0; }
  __syncthreads();
  if (tid == 0) {
    for (int k = T + 1; k > 0; --k) s_pre[k - 1] = fmax(s_pre[k - 1], s_pre[k]);
    double sum = 0.0;
    for (int k = 0; k <= T; ++k)
      if (s_rec[k + 1] != s_rec[k]) sum += (s_rec[k + 1] - s_rec[k]) * s_pre[k + 1];
    count_face[s] = faces;
    ap[s] = faces == 0 ? 0.0 : sum;
  }
}

}  // namespace

extern "C" int danhip_wider_quantize(const void* dets, int in_dtype, const int32_t* num, const int32_t* image_index, int32_t B, int32_t Nmax,
                                     int32_t quantize, double* store_rows, int32_t* store_counts, int32_t I, int32_t cap, int32_t* status,
                                     void* stream) {
  DH_REQUIRE(dets && num && image_index && store_rows && store_counts && status, DANHIP_EINVAL, "wider_quantize: null pointer");
  DH_REQUIRE(B > 0 && Nmax > 0 && I > 0 && cap > 0, DANHIP_EINVAL, "wider_quantize: bad sizes");
  DH_REQUIRE(cap <= kMaxDets && Nmax <= cap, DANHIP_EINVAL, "wider_quantize: at most %d detections per image (Nmax %d, store rows per image %d)",
             kMaxDets, Nmax, cap);
  DH_REQUIRE(in_dtype == DANHIP_F32 || (in_dtype == DANHIP_WIDER_F64 && !quantize), DANHIP_EINVAL,
             "wider_quantize: rows are fp32, or float64 with quantize = 0 (the text route is defined on fp32 rows)");
  if (in_dtype == DANHIP_F32)
    hipLaunchKernelGGL(wider_quantize_kernel<float>, dim3(B), dim3(kQuantThreads), 0, (hipStream_t)stream, (const float*)dets, num, image_index, Nmax,
                       quantize, store_rows, store_counts, I, cap, status);
  else
    hipLaunchKernelGGL(wider_quantize_kernel<double>, dim3(B), dim3(kQuantThreads), 0, (hipStream_t)stream, (const double*)dets, num, image_index, Nmax,
                       quantize, store_rows, store_counts, I, cap, status);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" size_t danhip_wider_score_range_workspace_bytes(void) { return (size_t)kRangeBlocks * 2 * sizeof(double); }

extern "C" int danhip_wider_score_range(const double* det_rows, int64_t D, double* range, void* workspace, size_t workspace_bytes, void* stream) {
  DH_REQUIRE(range && workspace && D >= 0 && (det_rows || D == 0), DANHIP_EINVAL, "wider_score_range: bad arguments");
  DH_REQUIRE(workspace_bytes >= danhip_wider_score_range_workspace_bytes(), DANHIP_EWORKSPACE, "wider_score_range: workspace too small");
  const int nb = D <= 0 ? 1 : (int)((D + 255) / 256 < kRangeBlocks ? (D + 255) / 256 : kRangeBlocks);
  hipLaunchKernelGGL(wider_range_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, det_rows, (long)D, (double*)workspace);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(wider_range_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, nb, (long)D, range);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" size_t danhip_wider_eval_workspace_bytes(int32_t I, int32_t S, int32_t T) {
  if (I < 1 || S < 1 || T < 1) return 0;
  return (size_t)eval_blocks(I) * (size_t)S * (size_t)T * 2 * sizeof(uint32_t);
}

extern "C" int danhip_wider_eval(const int32_t* det_offsets, const double* det_rows, int64_t D, const int32_t* gt_offsets, const double* gt_boxes,
                                 const uint8_t* gt_keep, int64_t G, const double* range, int32_t I, int32_t S, int32_t T, int32_t max_dets,
                                 double iou_threshold, void* workspace, size_t workspace_bytes, int32_t* status, void* stream) {
  DH_REQUIRE(det_offsets && gt_offsets && range && workspace && status, DANHIP_EINVAL, "wider_eval: null pointer");
  DH_REQUIRE(D >= 0 && G >= 0 && (det_rows || D == 0) && ((gt_boxes && gt_keep) || G == 0), DANHIP_EINVAL, "wider_eval: null rows / boxes");
  DH_REQUIRE(I > 0 && I <= kMaxImages && S > 0 && S <= DANHIP_WIDER_MAX_SUBSETS && T > 0 && T <= DANHIP_WIDER_MAX_THRESHOLDS, DANHIP_EINVAL,
             "wider_eval: needs 1 <= I <= %d, 1 <= S <= %d, 1 <= T <= %d", kMaxImages, DANHIP_WIDER_MAX_SUBSETS, DANHIP_WIDER_MAX_THRESHOLDS);
  DH_REQUIRE(max_dets >= 0 && max_dets <= kMaxDets, DANHIP_EINVAL, "wider_eval: at most %d detections per image, the caller allows %d", kMaxDets,
             max_dets);
  DH_REQUIRE(workspace_bytes >= danhip_wider_eval_workspace_bytes(I, S, T), DANHIP_EWORKSPACE, "wider_eval: workspace too small");
  EvalArgs a = {det_offsets, det_rows, gt_offsets, gt_boxes, gt_keep, range, I, S, T, (long)D, (long)G, iou_threshold, (uint32_t*)workspace, status};
  hipLaunchKernelGGL(wider_eval_kernel, dim3(eval_blocks(I)), dim3(kEvalThreads), 0, (hipStream_t)stream, a);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_wider_ap(const void* workspace, size_t workspace_bytes, const uint8_t* gt_keep, int64_t G, int32_t I, int32_t S, int32_t T,
                               int64_t* curves, int64_t* count_face, double* precision, double* recall, double* ap, void* stream) {
  DH_REQUIRE(workspace && curves && count_face && precision && recall && ap && G >= 0 && (gt_keep || G == 0), DANHIP_EINVAL, "wider_ap: null pointer");
  DH_REQUIRE(I > 0 && I <= kMaxImages && S > 0 && S <= DANHIP_WIDER_MAX_SUBSETS && T > 0 && T <= DANHIP_WIDER_MAX_THRESHOLDS, DANHIP_EINVAL,
             "wider_ap: needs 1 <= I <= %d, 1 <= S <= %d, 1 <= T <= %d", kMaxImages, DANHIP_WIDER_MAX_SUBSETS, DANHIP_WIDER_MAX_THRESHOLDS);
  DH_REQUIRE(workspace_bytes >= danhip_wider_eval_workspace_bytes(I, S, T), DANHIP_EWORKSPACE, "wider_ap: workspace too small");
  const long entries = (long)S * T * 2;
  hipLaunchKernelGGL(wider_curve_reduce_kernel, dim3(cdiv(entries, 256)), dim3(256), 0, (hipStream_t)stream, (const uint32_t*)workspace, eval_blocks(I),
                     entries, curves);
  DH_LAUNCH_CHECK();
  hipLaunchKernelGGL(wider_ap_kernel, dim3(S), dim3(kApThreads), 0, (hipStream_t)stream, (const int64_t*)curves, gt_keep, (long)G, T, count_face, precision,
                     recall, ap);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}
