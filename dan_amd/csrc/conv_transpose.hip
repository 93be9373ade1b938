// Transposed convolution 4x4 / stride 2 / 'same' on NHWC (tf.layers.conv2d_transpose(x, Cout, (4, 4), strides=(2, 2), padding='same')),
// fused with the LFPN's lateral add - the rule is written out in include/danhip.h:
//   full[n, 2 iy + ky - 1, 2 ix + kx - 1, co] += x[n, iy, ix, ci] * W[ky, kx, co, ci];   out = lateral + bias + full, cropped to Ho x Wo.
//
// All three training kernels are the same implicit GEMM D[m][n] = sum_k A[m][k] B[n][k] on v_mfma_f32_16x16x32 with gathered A rows:
//   forward        one launch, four output-parity phases (grid z).  Phase (py, px) holds the outputs (2 qy + py, 2 qx + px); each of them has
//                  exactly the 2 x 2 taps ky in {1, 3} (py = 0) or {0, 2} (py = 1), reading input rows qy, qy - 1 or qy + 1, qy: a 2 x 2
//                  convolution over the input with K = 4 Cin.  Without the split a 4 x 4 gather over the zero-stuffed map would multiply
//                  three zeros for every product it keeps.  Rows = input-grid positions (n, qy, qx), columns = co, B = W as it lies
//                  (W[ky][kx][co][:] is a K-contiguous row), rounded to 16 bits.
//   data gradient  dX[n, iy, ix, ci] = sum over the 16 taps and co of dOut[n, 2 iy + ky - 1, 2 ix + kx - 1, co] W[ky, kx, co, ci]: a 4 x 4 /
//                  stride-2 convolution with K = 16 Cout; a tap outside the Ho x Wo map (the border, or the cropped last row / column)
//                  contributes nothing.  B = W with its two channel axes swapped ([ky][kx][ci][co]).
//   weight gradient dW[ky, kx, co, ci] = sum over pixels of dOut[.., co] x[.., ci]: K = pixels.  Both operands are staged through LDS
//                  TRANSPOSED ([channel][pixel]) so that a lane's eight K values lie together.  The pixels are cut into slabs
//                  (conv_transpose_plan.h); every workgroup stores its partial tile and ordered_reduce.hip adds the slabs in index order.
//                  The bias gradient is the column sum of dOut: partial rows, same reduction.
// Tiles: 128 pixels x 64 channels x K 64 per 256-thread workgroup (forward, data gradient: a wave owns 32 x 64 = 2 x 4 accumulators), 64 x
// 64 x 64 pixels for the weight gradient (a wave owns 32 x 32).  Global loads are staged through registers one K step ahead of the MFMAs.
// The epilogue goes through LDS so that a pixel's 64 channels leave as one 128-byte line (eight 16-byte lanes), with bias, lateral and the
// accumulate-into-slot read in the same lanes; one rounding, at the end.  No atomics anywhere: every result is a fixed function of the inputs,
// so deterministic mode needs no other form.
#include "conv_common.h"
#include "conv_transpose_plan.h"

namespace {

constexpr int LP = CT_BK + 8;        // LDS row pitch in 16-bit elements: 144 bytes (16-byte aligned rows, rows 36 banks apart)
constexpr int CP = CT_BN + 4;        // epilogue row pitch in floats

struct CtArgs {
  const bf16_t* a;        // forward: x [N,Hi,Wi,Ci]; data gradient: dOut [N,Ho,Wo,Co]
  const bf16_t* w;        // forward: [4][4][Co][Ci]; data gradient: [4][4][Ci][Co]
  const float* bias;
  const bf16_t* lateral;
  bf16_t* out;
  int N, Hi, Wi, Ho, Wo, Ci, Co, M, accumulate;
  FastDiv div_wi, div_hiwi;
};

// DGRAD = false: forward (grid z = phase); true: data gradient
template <bool DGRAD>
__global__ __launch_bounds__(256) void ct_gemm_kernel(const CtArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[CT_BM * CP * 4];      // K loop: As [128][LP] + Bs [64][LP] (27648 B); epilogue: fp32 [128][CP]
  bf16_t* As = reinterpret_cast<bf16_t*>(smem);
  bf16_t* Bs = As + CT_BM * LP;
  float* Cs = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * CT_BM, n0 = blockIdx.y * CT_BN;
  const int py = DGRAD ? 0 : (int)(blockIdx.z >> 1), px = DGRAD ? 0 : (int)(blockIdx.z & 1);
  const int KA = DGRAD ? a.Co : a.Ci;          // channels of the gathered operand = K per tap
  const int NB = DGRAD ? a.Ci : a.Co;          // rows of B per tap
  const int taps = DGRAD ? 16 : 4;
  const int kc_per_tap = KA / CT_BK;
  const int ktiles = taps * kc_per_tap;
  // staging roles: 16-byte chunk c8 = tid & 7 of rows (tid >> 3) + 32 i (A: i < 4, B: i < 2); the epilogue uses the same rows
  const int c8 = tid & 7, r0 = tid >> 3;
  int rn[4], ry[4], rx[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + r0 + 32 * i;
    rn[i] = 0; ry[i] = -(1 << 20); rx[i] = -(1 << 20);      // a row past M: every tap is out of range
    if (m < a.M) {
      const unsigned n = fdiv((unsigned)m, a.div_hiwi);
      const unsigned rem = (unsigned)m - n * (unsigned)(a.Hi * a.Wi);
      const unsigned y = fdiv(rem, a.div_wi);
      rn[i] = (int)n; ry[i] = (int)y; rx[i] = (int)(rem - y * (unsigned)a.Wi);
    }
  }
  uint4 ra[4], rb[2];
  auto load = [&](int kt) {
    const int tap = kt / kc_per_tap, c0 = (kt - tap * kc_per_tap) * CT_BK + c8 * 8;
    int wtap;
    if (DGRAD) {
      const int ky = tap >> 2, kx = tap & 3;
      wtap = tap;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int oy = 2 * ry[i] + ky - 1, ox = 2 * rx[i] + kx - 1;
        ra[i] = make_uint4(0, 0, 0, 0);
        if ((unsigned)oy < (unsigned)a.Ho && (unsigned)ox < (unsigned)a.Wo)
          ra[i] = *reinterpret_cast<const uint4*>(a.a + (((size_t)rn[i] * a.Ho + oy) * a.Wo + ox) * a.Co + c0);
      }
    } else {
      const int ty = tap >> 1, tx = tap & 1;
      // py = 0: ky = 1 reads row qy, ky = 3 row qy - 1;  py = 1: ky = 0 reads row qy + 1, ky = 2 row qy  (oy = 2 iy + ky - 1)
      const int ky = py ? 2 * ty : 1 + 2 * ty, kx = px ? 2 * tx : 1 + 2 * tx;
      const int dy = py ? 1 - ty : -ty, dx = px ? 1 - tx : -tx;
      wtap = ky * 4 + kx;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int iy = ry[i] + dy, ix = rx[i] + dx;
        ra[i] = make_uint4(0, 0, 0, 0);
        if ((unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi)
          ra[i] = *reinterpret_cast<const uint4*>(a.a + (((size_t)rn[i] * a.Hi + iy) * a.Wi + ix) * a.Ci + c0);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      rb[i] = *reinterpret_cast<const uint4*>(a.w + ((size_t)wtap * NB + n0 + r0 + 32 * i) * KA + c0);
  };
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  load(0);
  for (int kt = 0; kt < ktiles; ++kt) {
    __syncthreads();                                     // the previous step's fragments are in registers
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint4*>(As + (r0 + 32 * i) * LP + c8 * 8) = ra[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(Bs + (r0 + 32 * i) * LP + c8 * 8) = rb[i];
    __syncthreads();
    if (kt + 1 < ktiles) load(kt + 1);                   // in flight under this step's MFMAs
#pragma unroll
    for (int ks = 0; ks < CT_BK / 32; ++ks) {
      // operands of v_mfma_f32_16x16x32: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and B[k = 8 (l >> 4) + j][col l & 15]
      const int ko = ks * 32 + 8 * (lane >> 4);
      bf16x8 fa[2], fb[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(As + (wave * 32 + i * 16 + (lane & 15)) * LP + ko);
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(Bs + (j * 16 + (lane & 15)) * LP + ko);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = DH_MFMA_16x16x32(fa[i], fb[j], acc[i][j]);
    }
  }
  __syncthreads();                                       // every wave is done reading As / Bs: the buffer becomes the fp32 tile
  // C/D layout: col = lane & 15 (channel), row = (lane >> 4) * 4 + r (pixel)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) Cs[(wave * 32 + i * 16 + (lane >> 4) * 4 + r) * CP + j * 16 + (lane & 15)] = acc[i][j][r];
  __syncthreads();
  const int co = n0 + c8 * 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (ry[i] < 0) continue;                             // past M
    size_t o;
    if (DGRAD) {
      o = (size_t)(m0 + r0 + 32 * i) * a.Ci + co;
    } else {
      const int oy = 2 * ry[i] + py, ox = 2 * rx[i] + px;
      if (oy >= a.Ho || ox >= a.Wo) continue;            // the cropped last row / column
      o = (((size_t)rn[i] * a.Ho + oy) * a.Wo + ox) * a.Co + co;
    }
    float v[8];
    const float* cs = Cs + (r0 + 32 * i) * CP + c8 * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = cs[e];
    if (a.bias) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += a.bias[co + e];
    }
    if (a.lateral) {
      float t[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(a.lateral + o), t);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += t[e];
    }
    if (a.accumulate) {
      float t[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(a.out + o), t);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += t[e];
    }
    *reinterpret_cast<uint4*>(a.out + o) = dh_pack8(v);
  }
}

// ---------------------------------------------------------------- weight gradient
struct CtWgArgs {
  const bf16_t* x;        // [N,Hi,Wi,Ci]
  const bf16_t* dout;     // [N,Ho,Wo,Co]
  float* slab;            // [slabs][16][Co][Ci]
  int N, Hi, Wi, Ho, Wo, Ci, Co, M, steps, steps_per_slab, ci_tiles;
  long dw_elems;
  FastDiv div_wi, div_hiwi;
};

__global__ __launch_bounds__(256) void ct_wgrad_kernel(const CtWgArgs a) {
  __shared__ __attribute__((aligned(16))) bf16_t At[CT_BN * LP];      // dOut^T [co][pixel]
  __shared__ __attribute__((aligned(16))) bf16_t Bt[CT_BN * LP];      // x^T    [ci][pixel]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int cot = blockIdx.x / a.ci_tiles, cit = blockIdx.x - cot * a.ci_tiles;
  const int co0 = cot * CT_BN, ci0 = cit * CT_BN;
  const int tap = blockIdx.y, ky = tap >> 2, kx = tap & 3;
  const int s0 = blockIdx.z * a.steps_per_slab;
  const int s1 = min(a.steps, s0 + a.steps_per_slab);
  // staging roles: pixel tid & 63 of the step (a wave's 64 lanes store 64 consecutive 16-bit LDS columns: no bank conflict), channel chunks
  // (tid >> 6) and (tid >> 6) + 4
  const int pl = tid & 63, q0 = tid >> 6;
  uint4 rd[2], rx[2];
  auto load = [&](int st) {
    const int p = st * CT_BK + pl;
    rd[0] = rd[1] = rx[0] = rx[1] = make_uint4(0, 0, 0, 0);
    if (p < a.M) {
      const unsigned n = fdiv((unsigned)p, a.div_hiwi);
      const unsigned rem = (unsigned)p - n * (unsigned)(a.Hi * a.Wi);
      const unsigned iy = fdiv(rem, a.div_wi);
      const int ix = (int)(rem - iy * (unsigned)a.Wi);
      const int oy = 2 * (int)iy + ky - 1, ox = 2 * ix + kx - 1;
      if ((unsigned)oy < (unsigned)a.Ho && (unsigned)ox < (unsigned)a.Wo) {     // (a pixel without this tap adds nothing: x need not be read)
        const bf16_t* dp = a.dout + (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.Co + co0;
        const bf16_t* xp = a.x + (size_t)p * a.Ci + ci0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          rd[i] = *reinterpret_cast<const uint4*>(dp + (q0 + 4 * i) * 8);
          rx[i] = *reinterpret_cast<const uint4*>(xp + (q0 + 4 * i) * 8);
        }
      }
    }
  };
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  load(s0);
  for (int st = s0; st < s1; ++st) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bf16_t* d16 = reinterpret_cast<const bf16_t*>(&rd[i]);
      const bf16_t* x16 = reinterpret_cast<const bf16_t*>(&rx[i]);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        At[((q0 + 4 * i) * 8 + e) * LP + pl] = d16[e];
        Bt[((q0 + 4 * i) * 8 + e) * LP + pl] = x16[e];
      }
    }
    __syncthreads();
    if (st + 1 < s1) load(st + 1);
#pragma unroll
    for (int ks = 0; ks < CT_BK / 32; ++ks) {
      const int ko = ks * 32 + 8 * (lane >> 4);
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(At + (wm * 32 + i * 16 + (lane & 15)) * LP + ko);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(Bt + (wn * 32 + j * 16 + (lane & 15)) * LP + ko);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = DH_MFMA_16x16x32(fa[i], fb[j], acc[i][j]);
    }
  }
  // C/D layout: col = lane & 15 (ci), row = (lane >> 4) * 4 + r (co)
  float* dst = a.slab + (size_t)blockIdx.z * a.dw_elems + (size_t)tap * a.Co * a.Ci;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        dst[(size_t)(co0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r) * a.Ci + ci0 + wn * 32 + j * 16 + (lane & 15)] = acc[i][j][r];
}

// bias gradient: row b of `rows` = the column sum of dOut over output pixels [b per, min(Mo, (b + 1) per)).  Co / 8 lanes per pixel (16-byte
// loads), 256 / (Co / 8) pixels side by side; a lane adds its pixels in ascending order, the pixel groups meet in LDS in group order.
__global__ __launch_bounds__(256) void ct_bias_grad_kernel(const bf16_t* __restrict__ dout, float* __restrict__ rows, long Mo, long per, int Co) {
  __shared__ float red[2048];                            // [groups][Co], groups Co <= 256 * 8
  const int tpp = Co / 8, groups = 256 / tpp;
  const int g = threadIdx.x / tpp, c = threadIdx.x - g * tpp;
  const long p0 = (long)blockIdx.x * per, p1 = p0 + per < Mo ? p0 + per : Mo;
  if (g < groups) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long p = p0 + g; p < p1; p += groups) {
      float t[8];
      dh_unpack8(*reinterpret_cast<const uint4*>(dout + (size_t)p * Co + c * 8), t);
#pragma unroll
      for (int e = 0; e < 8; ++e) s[e] += t[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[g * Co + c * 8 + e] = s[e];
  }
  __syncthreads();
  for (int ch = threadIdx.x; ch < Co; ch += 256) {
    float s = red[ch];
    for (int k = 1; k < groups; ++k) s += red[k * Co + ch];
    rows[(size_t)blockIdx.x * Co + ch] = s;
  }
}

// fp32 W [4][4][Co][Ci] -> 16-bit wf (same layout) and, when asked for, wb [4][4][Ci][Co]
__global__ void ct_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ wf, bf16_t* __restrict__ wb, int Ci, int Co) {
  const long total = 16L * Co * Ci;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const bf16_t v = f2bf(w[idx]);
    wf[idx] = v;
    if (wb) {
      const int ci = (int)(idx % Ci);
      const long t = idx / Ci;
      const int co = (int)(t % Co);
      const long tap = t / Co;
      wb[(tap * Ci + ci) * Co + co] = v;
    }
  }
}

// ---------------------------------------------------------------- fp32 inference: plain FMA chains
// A workgroup owns eight same-phase outputs of one output row (qx0 .. qx0 + 7) and 256 output channels, one per lane; the inputs of the
// phase's four taps lie in LDS in chunks of 256 channels, so a weight is loaded once for eight products.  Sum order per output: channel
// chunk, then tap (ty, tx), then channel - fixed.
struct CtF32Args {
  const float* x; const float* w; const float* bias; const float* lateral; float* out;
  int N, Hi, Wi, Ho, Wo, Ci, Co, xtiles;
};
__global__ __launch_bounds__(256) void ct_fwd_f32_kernel(const CtF32Args a) {
  constexpr int PX = 8, KC = 256;
  __shared__ float xs[PX][4][KC];                        // 32 KiB
  const int phase = blockIdx.z & 3, n = blockIdx.z >> 2, py = phase >> 1, px = phase & 1;
  const int qy = blockIdx.x / a.xtiles, qx0 = (blockIdx.x - qy * a.xtiles) * PX;
  const int co = blockIdx.y * 256 + threadIdx.x;
  const int oy = 2 * qy + py;
  if (oy >= a.Ho) return;                                // (uniform for the workgroup)
  float acc[PX];
#pragma unroll
  for (int p = 0; p < PX; ++p) acc[p] = 0.f;
  for (int c0 = 0; c0 < a.Ci; c0 += KC) {
    const int kc = min(KC, a.Ci - c0);
    __syncthreads();
    for (int idx = threadIdx.x; idx < PX * 4 * kc; idx += 256) {
      const int c = idx % kc, t = (idx / kc) & 3, p = idx / (4 * kc);
      const int ty = t >> 1, tx = t & 1;
      const int iy = qy + (py ? 1 - ty : -ty), ix = qx0 + p + (px ? 1 - tx : -tx);
      float v = 0.f;
      if (qx0 + p < a.Wi && (unsigned)iy < (unsigned)a.Hi && (unsigned)ix < (unsigned)a.Wi)
        v = a.x[(((size_t)n * a.Hi + iy) * a.Wi + ix) * a.Ci + c0 + c];
      xs[p][t][c] = v;
    }
    __syncthreads();
    if (co < a.Co) {
      for (int t = 0; t < 4; ++t) {
        const int ty = t >> 1, tx = t & 1;
        const int ky = py ? 2 * ty : 1 + 2 * ty, kx = px ? 2 * tx : 1 + 2 * tx;
        const float* wp = a.w + ((size_t)(ky * 4 + kx) * a.Co + co) * a.Ci + c0;
        for (int c = 0; c < kc; c += 4) {
          const float4 w4 = *reinterpret_cast<const float4*>(wp + c);
#pragma unroll
          for (int p = 0; p < PX; ++p) {
            acc[p] = fmaf(xs[p][t][c], w4.x, acc[p]);
            acc[p] = fmaf(xs[p][t][c + 1], w4.y, acc[p]);
            acc[p] = fmaf(xs[p][t][c + 2], w4.z, acc[p]);
            acc[p] = fmaf(xs[p][t][c + 3], w4.w, acc[p]);
          }
        }
      }
    }
  }
  if (co >= a.Co) return;
  const float b = a.bias ? a.bias[co] : 0.f;
#pragma unroll
  for (int p = 0; p < PX; ++p) {
    const int ox = 2 * (qx0 + p) + px;
    if (qx0 + p >= a.Wi || ox >= a.Wo) continue;
    const size_t o = (((size_t)n * a.Ho + oy) * a.Wo + ox) * a.Co + co;
    float v = acc[p] + b;
    if (a.lateral) v += a.lateral[o];
    a.out[o] = v;
  }
}

int ct_check(const char* who, int N, int Hi, int Wi, int Ho, int Wo, int Ci, int Co) {
  const char* e = ct_shape_error(N, Hi, Wi, Ho, Wo, Ci, Co);
  DH_REQUIRE(!e, DANHIP_EINVAL, "%s: %s (N=%d, Hi=%d, Wi=%d, Ho=%d, Wo=%d, Cin=%d, Cout=%d)", who, e, N, Hi, Wi, Ho, Wo, Ci, Co);
  return DANHIP_OK;
}

}  // namespace

extern "C" int danhip_conv_transpose4x4s2_pack_weight(const float* w, void* wf, void* wb, int32_t Cin, int32_t Cout, void* stream) {
  if (int rc = ct_check("conv_transpose4x4s2_pack_weight", 1, 1, 1, 2, 2, Cin, Cout)) return rc;
  DH_REQUIRE(w && wf, DANHIP_EINVAL, "conv_transpose4x4s2_pack_weight: null pointer");
  const long total = 16L * Cin * Cout;
  hipLaunchKernelGGL(ct_pack_kernel, dim3(dh_grid_for(total, 256, 2048)), dim3(256), 0, (hipStream_t)stream, w, reinterpret_cast<bf16_t*>(wf),
                     reinterpret_cast<bf16_t*>(wb), Cin, Cout);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_conv_transpose4x4s2_add_fwd(const void* x, const void* wf, const float* bias, const void* lateral, void* out, int32_t N,
                                                  int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout, void* stream) {
  if (int rc = ct_check("conv_transpose4x4s2_add_fwd", N, Hi, Wi, Ho, Wo, Cin, Cout)) return rc;
  DH_REQUIRE(x && wf && out, DANHIP_EINVAL, "conv_transpose4x4s2_add_fwd: null pointer");
  CtArgs a{};
  a.a = reinterpret_cast<const bf16_t*>(x); a.w = reinterpret_cast<const bf16_t*>(wf); a.bias = bias;
  a.lateral = reinterpret_cast<const bf16_t*>(lateral); a.out = reinterpret_cast<bf16_t*>(out);
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.Ci = Cin; a.Co = Cout; a.M = N * Hi * Wi; a.accumulate = 0;
  a.div_wi = make_fastdiv(Wi); a.div_hiwi = make_fastdiv(Hi * Wi);
  hipLaunchKernelGGL(ct_gemm_kernel<false>, dim3(cdiv(a.M, CT_BM), Cout / CT_BN, 4), dim3(256), 0, (hipStream_t)stream, a);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" int danhip_conv_transpose4x4s2_dgrad(const void* dout, const void* wb, void* dx, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                                int32_t Cin, int32_t Cout, int accumulate, void* stream) {
  if (int rc = ct_check("conv_transpose4x4s2_dgrad", N, Hi, Wi, Ho, Wo, Cin, Cout)) return rc;
  DH_REQUIRE(dout && wb && dx, DANHIP_EINVAL, "conv_transpose4x4s2_dgrad: null pointer");
  CtArgs a{};
  a.a = reinterpret_cast<const bf16_t*>(dout); a.w = reinterpret_cast<const bf16_t*>(wb); a.out = reinterpret_cast<bf16_t*>(dx);
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.Ci = Cin; a.Co = Cout; a.M = N * Hi * Wi; a.accumulate = accumulate ? 1 : 0;
  a.div_wi = make_fastdiv(Wi); a.div_hiwi = make_fastdiv(Hi * Wi);
  hipLaunchKernelGGL(ct_gemm_kernel<true>, dim3(cdiv(a.M, CT_BM), Cin / CT_BN, 1), dim3(256), 0, (hipStream_t)stream, a);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}

extern "C" size_t danhip_conv_transpose4x4s2_wgrad_workspace_bytes(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout) {
  if (ct_shape_error(N, Hi, Wi, Ho, Wo, Cin, Cout)) return 0;
  return ct_wgrad_plan(N, Hi, Wi, Ho, Wo, Cin, Cout).bytes;
}

extern "C" int32_t danhip_conv_transpose4x4s2_wgrad_slabs(int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout) {
  if (ct_shape_error(N, Hi, Wi, Ho, Wo, Cin, Cout)) return 0;
  return ct_wgrad_plan(N, Hi, Wi, Ho, Wo, Cin, Cout).slabs;
}

extern "C" int danhip_conv_transpose4x4s2_wgrad(const void* x, const void* dout, float* dw, float* db, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho,
                                                int32_t Wo, int32_t Cin, int32_t Cout, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = ct_check("conv_transpose4x4s2_wgrad", N, Hi, Wi, Ho, Wo, Cin, Cout)) return rc;
  DH_REQUIRE(x && dout && (dw || db), DANHIP_EINVAL, "conv_transpose4x4s2_wgrad: null pointer");
  const CtWgradPlan p = ct_wgrad_plan(N, Hi, Wi, Ho, Wo, Cin, Cout);
  DH_REQUIRE(workspace && workspace_bytes >= p.bytes, DANHIP_EWORKSPACE,
             "conv_transpose4x4s2_wgrad: the workspace holds %zu bytes, danhip_conv_transpose4x4s2_wgrad_workspace_bytes says %zu", workspace_bytes, p.bytes);
  hipStream_t s = (hipStream_t)stream;
  if (dw) {
    CtWgArgs a{};
    a.x = reinterpret_cast<const bf16_t*>(x); a.dout = reinterpret_cast<const bf16_t*>(dout); a.slab = reinterpret_cast<float*>(workspace);
    a.N = N; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.Ci = Cin; a.Co = Cout; a.M = (int)p.pixels;
    a.steps = p.steps; a.steps_per_slab = p.steps_per_slab; a.ci_tiles = Cin / CT_BN; a.dw_elems = (long)p.dw_elems;
    a.div_wi = make_fastdiv(Wi); a.div_hiwi = make_fastdiv(Hi * Wi);
    hipLaunchKernelGGL(ct_wgrad_kernel, dim3((Cout / CT_BN) * (Cin / CT_BN), 16, p.slabs), dim3(256), 0, s, a);
    DH_LAUNCH_CHECK();
    if (int rc = dh_ordered_reduce(a.slab, (long)p.dw_elems, p.slabs, (long)p.dw_elems, dw, 1, s)) return rc;
  }
  if (db) {
    float* rows = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + p.db_off);
    hipLaunchKernelGGL(ct_bias_grad_kernel, dim3(p.db_rows), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(dout), rows, (long)N * Ho * Wo,
                       (long)p.db_pixels, Cout);
    DH_LAUNCH_CHECK();
    if (int rc = dh_ordered_reduce(rows, Cout, p.db_rows, Cout, db, 1, s)) return rc;
  }
  return DANHIP_OK;
}

extern "C" int danhip_conv_transpose4x4s2_add_fwd_f32(const float* x, const float* w, const float* bias, const float* lateral, float* out, int32_t N,
                                                      int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo, int32_t Cin, int32_t Cout, void* stream) {
  if (int rc = ct_check("conv_transpose4x4s2_add_fwd_f32", N, Hi, Wi, Ho, Wo, Cin, Cout)) return rc;
  DH_REQUIRE(x && w && out, DANHIP_EINVAL, "conv_transpose4x4s2_add_fwd_f32: null pointer");
  DH_REQUIRE((long)N * 4 <= 65535, DANHIP_EINVAL, "conv_transpose4x4s2_add_fwd_f32: N=%d exceeds the grid (16383 images per call)", N);
  CtF32Args a{};
  a.x = x; a.w = w; a.bias = bias; a.lateral = lateral; a.out = out;
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.Ci = Cin; a.Co = Cout; a.xtiles = cdiv(Wi, 8);
  hipLaunchKernelGGL(ct_fwd_f32_kernel, dim3(Hi * a.xtiles, cdiv(Cout, 256), N * 4), dim3(256), 0, (hipStream_t)stream, a);
  DH_LAUNCH_CHECK();
  return DANHIP_OK;
}
