// Sinkhorn divergence (models/sinkhorn.py) of real [na, D] and fake [nb, D]: the
// squared-distance matrices Cxy, Cxx, Cyy once per call, then T log-domain
// iterations that read each matrix once, on the pair (f, g) and on the two
// debiasing problems (p on Cxx, q on Cyy).
//
// Cost phase, three launches:
//   sk_norms_k   n[u] of real | fake, one wave per row.
//   sk_cost_k    one workgroup per 128 x 128 tile of one matrix: the exact-f32
//                Gram tile of pair_tile.h (inputs whose products and partial
//                sums are exact give exact costs); C = max(n_i + n_j - 2 G,
//                0). Of Cxx and Cyy only the tiles on or above the diagonal are
//                computed (the workgroups below it leave at once). Such a tile
//                is stored as it is, the diagonal as exact 0, and, off the
//                diagonal, a second time transposed: a wave turns its 64 x 32
//                part in LDS so that the mirrored rows leave as 16-byte stores
//                of 64 consecutive floats. Every Cxx workgroup also leaves the
//                sum of its tile, added in double.
//   sk_scale_k   one workgroup: the Cxx sums in tile order, an upper tile twice,
//                in double -> m, left in a device word that every later launch
//                reads (an iteration's eps is its host-computed factor times
//                that word); clears the first potentials buffer.
//
// Iteration, two launches:
//   sk_stream_k  memory-bound. A workgroup owns a band of 64 rows of one matrix
//                and its four waves walk the columns together, 256 per step: a
//                wave issues its 16 rows' 16-byte loads back to back, a lane
//                keeps the 16 rows' online (max, sum) of 2^((h_j - C_ij) s),
//                s = log2(e) / eps, in registers over the whole band and the
//                lanes are folded by shuffles at the end. On Cxy the same values
//                also give the columns' (max, sum) of 2^((f_i - C_ij) s)
//                over the wave's rows; the four waves' are merged in wave order
//                through LDS (double-buffered: one barrier per step) and one
//                partial per (band, column) is written. The Cxx and Cyy bands
//                have no barrier at all.
//   sk_update_k  a thread per potential: g's softmin from the band partials in
//                band order, the others from the row softmins; the new value is
//                the mean with the old one, or on the last iteration the softmin
//                itself, which also goes to pot together with the rows' marginal
//                violations. The potentials are double-buffered: every softmin of
//                an iteration has read the old ones.
//   sk_final_k   after the last iteration: marg_err, one workgroup, a fixed-order
//                sum in double; m beside it.
//
// No atomics, no workgroup waits for another, every sum has one order: calls
// repeat bitwise. Masked elements are selected away, never multiplied away, so
// the padding of a row or vector may hold anything.
#include "common.h"
#include "pair_tile.h"
#include "sinkhorn.h"

#include <cmath>

namespace mdt {

namespace {

constexpr float kSkInf = __builtin_huge_valf();
constexpr float kSkLow = -1.0e30f;  // the running maximum's start: finite, below every argument

__global__ __launch_bounds__(kSkThreads) void sk_norms_k(SinkhornArgs a) {
  const SkLayout L = sk_layout(a.na, a.nb);
  const int u = blockIdx.x * (kSkThreads / kWave) + wave_id();
  if (u >= a.na + a.nb) return;
  const float s = pair_row_norm(u < a.na ? a.real + (size_t)u * a.D : a.fake + (size_t)(u - a.na) * a.D, a.D);
  if (lane_id() == 0) a.ws[L.norms + (u < a.na ? u : L.lda + (u - a.na))] = s;
}

template <bool VEC>
__global__ __launch_bounds__(kPairThreads, 2) void sk_cost_k(SinkhornArgs a) {
  // A: the tile's rows, B: its columns, [row][kPairLd]; afterwards a wave's [32][kSkTLd] transposing buffer
  __shared__ __attribute__((aligned(16))) float lds[2 * kPairTile * kPairLd];
  __shared__ double red[kPairThreads / kWave];
  static_assert(4 * 32 * kSkTLd <= 2 * kPairTile * kPairLd, "the transposing buffers fit the operand tiles");
  float* As = lds;
  float* Bs = lds + kPairTile * kPairLd;

  const SkLayout L = sk_layout(a.na, a.nb);
  int b = blockIdx.x, prob, ti, tj;
  if (b < L.ta * L.tb) {
    prob = 0, ti = b / L.tb, tj = b % L.tb;
  } else if ((b -= L.ta * L.tb) < L.ta * L.ta) {
    prob = 1, ti = b / L.ta, tj = b % L.ta;
  } else {
    b -= L.ta * L.ta;
    prob = 2, ti = b / L.tb, tj = b % L.tb;
  }
  if (prob != 0 && tj < ti) return;  // the tile (tj, ti) stores this one
  const float* X = prob == 2 ? a.fake : a.real;
  const float* Y = prob == 1 ? a.real : a.fake;
  const int nX = prob == 2 ? a.nb : a.na, nY = prob == 1 ? a.na : a.nb;
  const float* qX = a.ws + L.norms + (prob == 2 ? L.lda : 0);
  const float* qY = a.ws + L.norms + (prob == 1 ? 0 : L.lda);
  float* Cm = a.ws + (prob == 0 ? L.cxy : prob == 1 ? L.cxx : L.cyy);
  const int ld = prob == 1 ? L.lda : L.ldb;

  const int D = a.D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
  const int i0 = ti * kPairTile, j0 = tj * kPairTile;

  const int srow = tid >> 3;  // staging: thread -> rows srow + 32 i (i < 4) of each operand tile
  const float* pa[4];
  const float* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = i0 + srow + 32 * i, v = j0 + srow + 32 * i;
    pa[i] = u < nX ? X + (size_t)u * D : nullptr;
    pb[i] = v < nY ? Y + (size_t)v * D : nullptr;
  }

  f32x16 acc[2][2];
  pair_gram128<VEC>(pa, pb, D, As, Bs, tid, acc);

  // accumulator register reg of lane (r, h): row 32 m + (reg & 3) + 8 (reg >> 2) + 4 h of the wave's 64, column
  // 32 n + r. The cost takes the register's place; a half wave stores 32 consecutive floats.
  double sum = 0.0;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int j = j0 + wc * 64 + n * 32 + r;
    const float qj = j < nY ? qY[j] : 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int i = i0 + wr * 64 + m * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        const float qi = i < nX ? qX[i] : 0.f;
        float c = pair_d2(acc[m][n][reg], qi, qj);
        if (prob != 0 && i == j) c = 0.f;
        acc[m][n][reg] = c;
        if (i < nX && j < nY) {
          Cm[(size_t)i * ld + j] = c;
          sum += (double)c;
        }
      }
  }

  if (prob != 0 && ti != tj) {  // the mirrored tile: rows j, columns i of the same matrix
    float* T = lds + wave * (32 * kSkTLd);
    __syncthreads();  // every wave is done with the operand tiles
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(T + r * kSkTLd + m * 32 + 8 * g + 4 * h) =
              make_float4(acc[m][n][4 * g], acc[m][n][4 * g + 1], acc[m][n][4 * g + 2], acc[m][n][4 * g + 3]);
      __syncthreads();
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const int jl = 4 * p + (lane >> 4), il = 4 * (lane & 15);
        const float4 v = *reinterpret_cast<const float4*>(T + jl * kSkTLd + il);
        const int gj = j0 + wc * 64 + n * 32 + jl, gi = i0 + wr * 64 + il;
        // gi is a multiple of 4 below nX, so gi + 3 is below the row stride: the padding takes what is past nX
        if (gj < nY && gi < nX) *reinterpret_cast<float4*>(Cm + (size_t)gj * ld + gi) = v;
      }
      __syncthreads();  // before the next half overwrites the buffer
    }
  }

  if (prob == 1) {  // block-uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (tid == 0) {
      double* part = reinterpret_cast<double*>(a.ws + L.part);
      part[ti * L.ta + tj] = ((red[0] + red[1]) + red[2]) + red[3];
    }
  }
}

__global__ __launch_bounds__(kSkThreads) void sk_scale_k(SinkhornArgs a) {
  __shared__ double red[kSkThreads];
  const SkLayout L = sk_layout(a.na, a.nb);
  const int tid = threadIdx.x;
  const double* part = reinterpret_cast<const double*>(a.ws + L.part);
  double s = 0.0;
  for (int t = tid; t < L.ta * L.ta; t += kSkThreads) {
    const int ti = t / L.ta, tj = t % L.ta;
    if (tj >= ti) s += tj > ti ? 2.0 * part[t] : part[t];
  }
  red[tid] = s;
  __syncthreads();
  for (int o = kSkThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    double* scale = reinterpret_cast<double*>(a.ws + L.scale);
    scale[0] = red[0] / ((double)a.na * (double)a.na);
    scale[1] = red[0];
  }
  float* pots = a.ws + L.pots;
  for (int i = tid; i < L.vec(); i += kSkThreads) pots[i] = 0.f;
}

// s = log2(e) / eps from the iteration's factor and the device's m, rounded once, and eps ln 2 in double.
// The rounding of s scales every argument alike, which moves a softmin by that relative error times the
// (h - C) of its dominant terms: half a rounding of the softmin's own size. (The inverse of the rounded s
// in place of eps ln 2 would move it by the relative error times up to eps log n, which at the start of the
// anneal is many times the softmin.)
struct SkEps {
  float s, eps;
  double inv;
};
__device__ __forceinline__ SkEps sk_eps(const SinkhornArgs& a, const SkLayout& L, double factor) {
  const double eps = factor * reinterpret_cast<const double*>(a.ws + L.scale)[0];
  return {(float)(1.4426950408889634 / eps), (float)eps, eps * 0.6931471805599453};
}

// -eps ln 2 (lw2 + m + log2 s) of a finished (max, sum), rounded once. The log weight lw2 = -log2 n is the
// same in every term of a softmin, so it is added here, in double: inside the exponent its float rounding
// would move every softmin the same way by up to eps ln 2 times 2^-24 log2 n.
__device__ __forceinline__ float sk_softmin(float m, float s, double lw2, const SkEps& e) {
  return (float)(-(((double)m + log2((double)s)) + lw2) * e.inv);
}

__device__ __forceinline__ float sk_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// (m, s) <- (m, s) + (m2, s2) of two partial log-sum-exps in base 2
__device__ __forceinline__ void sk_merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = fmaf(s, sk_exp2(m - mn), s2 * sk_exp2(m2 - mn));
  m = mn;
}

// One band: rows [row0, row0 + 16) of this wave over all columns. XY: also the columns' partials over the band.
template <bool XY>
__device__ __forceinline__ void sk_band(const float* __restrict__ C, int ld, int nrows, int ncols,
                                        const float* __restrict__ hcol, double lw2, float* __restrict__ soft,
                                        const float* __restrict__ hrow, float2* __restrict__ slab,
                                        SkEps e, int row0, float* colp) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* rp[kSkWaveRows];
  float fr[kSkWaveRows], M[kSkWaveRows], S[kSkWaveRows];
#pragma unroll
  for (int k = 0; k < kSkWaveRows; ++k) {
    const int row = min(row0 + k, nrows - 1);  // a row past the end reads the last one and is masked or not stored
    rp[k] = C + (size_t)row * ld;
    fr[k] = XY ? hrow[row] : 0.f;
    M[k] = kSkLow;
    S[k] = 0.f;
  }
  int step = 0;
  for (int c0 = 0; c0 < ncols; c0 += kSkChunk, ++step) {
    const int col = c0 + 4 * lane;
    const int cl = min(col, ld - 4);  // in bounds whatever the lane; what is past ncols is selected away
    const float4 hv4 = *reinterpret_cast<const float4*>(hcol + cl);
    float4 cv[kSkWaveRows];
#pragma unroll
    for (int k = 0; k < kSkWaveRows; ++k) cv[k] = *reinterpret_cast<const float4*>(rp[k] + cl);
    const float hv[4] = {hv4.x, hv4.y, hv4.z, hv4.w};
    const bool ok[4] = {col < ncols, col + 1 < ncols, col + 2 < ncols, col + 3 < ncols};
    float cm[4] = {kSkLow, kSkLow, kSkLow, kSkLow}, cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kSkWaveRows; ++k) {
      const float c[4] = {cv[k].x, cv[k].y, cv[k].z, cv[k].w};
      float x[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q] = ok[q] ? (hv[q] - c[q]) * e.s : -kSkInf;
      const float mn = fmaxf(M[k], fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
      const float t = (sk_exp2(x[0] - mn) + sk_exp2(x[1] - mn)) + (sk_exp2(x[2] - mn) + sk_exp2(x[3] - mn));
      S[k] = fmaf(S[k], sk_exp2(M[k] - mn), t);
      M[k] = mn;
      if (XY) {
        const bool rv = row0 + k < nrows;
#pragma unroll
        for (int q = 0; q < 4; ++q) cm[q] = fmaxf(cm[q], ok[q] && rv ? (fr[k] - c[q]) * e.s : -kSkInf);
      }
    }
    if (XY) {
#pragma unroll
      for (int k = 0; k < kSkWaveRows; ++k) {
        const float c[4] = {cv[k].x, cv[k].y, cv[k].z, cv[k].w};
        const bool rv = row0 + k < nrows;
#pragma unroll
        for (int q = 0; q < 4; ++q) cs[q] += sk_exp2((ok[q] && rv ? (fr[k] - c[q]) * e.s : -kSkInf) - cm[q]);
      }
      // the four waves' partials of this step's 256 columns, merged in wave order by the thread of the column
      float* buf = colp + (step & 1) * (4 * kSkChunk * 2);
      float4* w = reinterpret_cast<float4*>(buf + (wave * kSkChunk + 4 * lane) * 2);
      w[0] = make_float4(cm[0], cs[0], cm[1], cs[1]);
      w[1] = make_float4(cm[2], cs[2], cm[3], cs[3]);
      __syncthreads();  // the other buffer's readers passed the previous step's barrier
      const float2* rd = reinterpret_cast<const float2*>(buf) + tid;
      float2 acc = rd[0];
#pragma unroll
      for (int v = 1; v < 4; ++v) {
        const float2 o = rd[v * kSkChunk];
        sk_merge(acc.x, acc.y, o.x, o.y);
      }
      if (c0 + tid < ncols) slab[c0 + tid] = acc;
    }
  }
  // the lanes' partials of a row, folded by an xor butterfly; lane k stores row k
  float mine = 0.f;
#pragma unroll
  for (int k = 0; k < kSkWaveRows; ++k) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) sk_merge(M[k], S[k], __shfl_xor(M[k], o, 64), __shfl_xor(S[k], o, 64));
    const float v = sk_softmin(M[k], S[k], lw2, e);
    if (lane == k) mine = v;
  }
  if (lane < kSkWaveRows && row0 + lane < nrows) soft[row0 + lane] = mine;
}

__global__ __launch_bounds__(kSkThreads) void sk_stream_k(SinkhornArgs a, double factor, int cur) {
  __shared__ __attribute__((aligned(16))) float colp[2 * 4 * kSkChunk * 2];
  const SkLayout L = sk_layout(a.na, a.nb);
  const SkEps e = sk_eps(a, L, factor);
  const float* pots = a.ws + L.pots + (size_t)cur * L.vec();
  const float *f = pots, *g = pots + L.lda, *p = g + L.ldb, *q = p + L.lda;
  float* soft = a.ws + L.soft;
  const double la2 = -log2((double)a.na), lb2 = -log2((double)a.nb);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // the rows' addresses are the wave's, not a lane's
  int b = blockIdx.x;
  if (b < L.bands_a) {
    float2* slab = reinterpret_cast<float2*>(a.ws + L.slab) + (size_t)b * L.ldb;
    sk_band<true>(a.ws + L.cxy, L.ldb, a.na, a.nb, g, lb2, soft, f, slab, e, b * kSkBand + wave * kSkWaveRows, colp);
  } else if ((b -= L.bands_a) < L.bands_a) {
    sk_band<false>(a.ws + L.cxx, L.lda, a.na, a.na, p, la2, soft + L.lda + L.ldb, nullptr, nullptr, e,
                   b * kSkBand + wave * kSkWaveRows, colp);
  } else {
    b -= L.bands_a;
    sk_band<false>(a.ws + L.cyy, L.ldb, a.nb, a.nb, q, lb2, soft + 2 * L.lda + L.ldb, nullptr, nullptr, e,
                   b * kSkBand + wave * kSkWaveRows, colp);
  }
}

__global__ __launch_bounds__(kSkThreads) void sk_update_k(SinkhornArgs a, double factor, int cur, int last) {
  const SkLayout L = sk_layout(a.na, a.nb);
  const int idx = blockIdx.x * kSkThreads + threadIdx.x;
  if (idx >= L.vec()) return;
  // the buffer's four parts: f, g, p, q
  const int seg = idx < L.lda ? 0 : idx < L.lda + L.ldb ? 1 : idx < 2 * L.lda + L.ldb ? 2 : 3;
  const int k = idx - (seg == 0 ? 0 : seg == 1 ? L.lda : seg == 2 ? L.lda + L.ldb : 2 * L.lda + L.ldb);
  if (k >= ((seg & 1) ? a.nb : a.na)) return;
  const SkEps e = sk_eps(a, L, factor);
  float* pots = a.ws + L.pots;
  const float old = pots[(size_t)cur * L.vec() + idx];
  float t;
  if (seg == 1) {  // the columns of Cxy: the bands' partials in band order
    const float2* slab = reinterpret_cast<const float2*>(a.ws + L.slab) + k;
    float2 acc = slab[0];
    for (int b = 1; b < L.bands_a; ++b) {
      const float2 o = slab[(size_t)b * L.ldb];
      sk_merge(acc.x, acc.y, o.x, o.y);
    }
    t = sk_softmin(acc.x, acc.y, -log2((double)a.na), e);
  } else {
    t = a.ws[L.soft + idx];
  }
  pots[(size_t)(cur ^ 1) * L.vec() + idx] = last ? t : 0.5f * (old + t);
  if (last) {
    a.pot[(size_t)((seg & 1) ? a.na + k : k) * kSkCols + (seg >> 1)] = t;
    if (seg == 0) a.ws[L.marg + k] = fabsf(expm1f((old - t) / e.eps));
  }
}

__global__ __launch_bounds__(kSkThreads) void sk_final_k(SinkhornArgs a) {
  __shared__ double red[kSkThreads];
  const SkLayout L = sk_layout(a.na, a.nb);
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < a.na; i += kSkThreads) s += (double)a.ws[L.marg + i];
  red[tid] = s;
  __syncthreads();
  for (int o = kSkThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    a.out[0] = reinterpret_cast<const double*>(a.ws + L.scale)[0];
    a.out[1] = red[0] / (double)a.na;
  }
}

}  // namespace

}  // namespace mdt

namespace {
int sk_sizes(const mdt::SinkhornArgs* a, bool rows) {
  using namespace mdt;
  if (a->na < 2 || a->na > kSkMaxRows || a->nb < 2 || a->nb > kSkMaxRows) return 1;
  if (rows && (a->D < 1 || a->D > kSkMaxD)) return 2;
  if (!(std::isfinite(a->E) && a->E > 0.0 && a->E <= kSkMaxBlur)) return 3;
  if (a->T < 1 || a->T > kSkMaxIters) return 4;
  return 0;
}
bool sk_aligned(const void* p, uintptr_t to) { return p != nullptr && (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
}  // namespace

extern "C" int mdt_sinkhorn_check(const mdt::SinkhornArgs* a) {
  const int rc = sk_sizes(a, true);
  if (rc) return rc;
  return a->real && a->fake && sk_aligned(a->ws, 16) && sk_aligned(a->pot, 4) && sk_aligned(a->out, 8) ? 0 : 5;
}

extern "C" int mdt_sinkhorn_cost(const mdt::SinkhornArgs* a, hipStream_t s) {
  using namespace mdt;
  const int rc = sk_sizes(a, true);
  if (rc) return rc;
  if (!a->real || !a->fake || !sk_aligned(a->ws, 16)) return 5;
  const SkLayout L = sk_layout(a->na, a->nb);
  hipLaunchKernelGGL(sk_norms_k, dim3((unsigned)sk_cdiv(a->na + a->nb, kSkThreads / kWave)), dim3(kSkThreads), 0, s, *a);
  const bool vec = a->D % 4 == 0 && ((reinterpret_cast<uintptr_t>(a->real) | reinterpret_cast<uintptr_t>(a->fake)) & 15) == 0;
  const dim3 grid((unsigned)(L.ta * L.tb + L.ta * L.ta + L.tb * L.tb));
  if (vec) hipLaunchKernelGGL(sk_cost_k<true>, grid, dim3(kPairThreads), 0, s, *a);
  else hipLaunchKernelGGL(sk_cost_k<false>, grid, dim3(kPairThreads), 0, s, *a);
  hipLaunchKernelGGL(sk_scale_k, dim3(1), dim3(kSkThreads), 0, s, *a);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}

extern "C" int mdt_sinkhorn_step(const mdt::SinkhornArgs* a, int t, hipStream_t s) {
  using namespace mdt;
  const int rc = sk_sizes(a, false);
  if (rc) return rc;
  if (t < 0 || t >= a->T) return 4;
  const int last = t == a->T - 1;
  if (!sk_aligned(a->ws, 16) || (last && !(sk_aligned(a->pot, 4) && sk_aligned(a->out, 8)))) return 5;
  const SkLayout L = sk_layout(a->na, a->nb);
  const double factor = std::fmax(a->E, std::ldexp(4.0, -t));  // max(E, 4 * 0.5^t)
  hipLaunchKernelGGL(sk_stream_k, dim3((unsigned)(2 * L.bands_a + L.bands_b)), dim3(kSkThreads), 0, s, *a, factor, t & 1);
  hipLaunchKernelGGL(sk_update_k, dim3((unsigned)sk_cdiv(L.vec(), kSkThreads)), dim3(kSkThreads), 0, s, *a, factor, t & 1,
                     last);
  if (last) hipLaunchKernelGGL(sk_final_k, dim3(1), dim3(kSkThreads), 0, s, *a);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}

extern "C" int mdt_sinkhorn_rows(const mdt::SinkhornArgs* a, hipStream_t s) {
  int rc = mdt_sinkhorn_check(a);  // every refusal before the first launch
  if (rc == 0) rc = mdt_sinkhorn_cost(a, s);
  for (int t = 0; rc == 0 && t < a->T; ++t) rc = mdt_sinkhorn_step(a, t, s);
  return rc;
}
