// Sliced Wasserstein distance (models/swd.py): the projections of real [na, D]
// and fake [nb, D] on dirs [P, D], sorted per set and direction, and per
// direction (w1, w2sq) of the two one-dimensional empirical measures.
//
//   swd_project_k   proj[P, na + nb] = dirs (real | fake)^T on the exact-f32 MFMA
//                   32x32x2 (a k-ordered fma chain per element, so inputs whose
//                   products and partial sums are exact give exact projections).
//                   One workgroup per (tile of 64 rows, tile of 128 directions)
//                   over the whole of D: no split-K, no second pass, one
//                   summation order. The rows are the operand that is read from
//                   memory once per direction tile, so the direction tile is the
//                   tall one; 2 x 1 MFMA tiles per wave, K in LDS chunks of 32
//                   with the tail of D zero-filled, the next chunk's loads in
//                   flight under the current chunk's MFMAs. The row index is the
//                   MFMA's column, so a lane half stores 32 consecutive floats.
//                   The real/fake boundary is a per-row pointer choice.
//   swd_sort_k      one workgroup per direction. Both sets' projections sit in
//                   LDS, each padded with +inf to its own power of two, and are
//                   sorted by one bitonic network each; the networks share their
//                   barriers. Between two barriers a thread holds a run of 16
//                   elements in registers, the 2^4 indices that differ in four
//                   consecutive bit positions, and does the four strides of
//                   those bits there: stage k = 2^L takes ceil(L / 4) barriers,
//                   not L, 28 + 1 in all at 16384 elements. The chunks of a
//                   stage are cut from its top stride down, so only the last may
//                   be partial and it is the one on contiguous elements (16-byte
//                   LDS accesses). A compare-exchange is a compare and two
//                   selects: the multiset of values is kept whatever the values.
//                   The sorted values go back over proj; then thread i of the
//                   longer side walks the at most two partners whose cells
//                   overlap [i ns, (i + 1) ns) on the common grid of na nb
//                   cells, with integer overlap lengths (exact as floats), and a
//                   fixed-order wave and workgroup reduction ends in one
//                   division by na nb. No atomics: calls repeat bitwise.
#include "common.h"
#include "pair_tile.h"
#include "swd.h"

namespace mdt {

namespace {

constexpr float kSwdInf = __builtin_huge_valf();

template <bool VEC>
__global__ __launch_bounds__(kSwdThreads, 2) void swd_project_k(SwdArgs a) {
  // A: the direction tile, B: the row tile, [row][kSwdLd]
  __shared__ __attribute__((aligned(16))) float lds[(kSwdTileP + kSwdTileN) * kSwdLd];
  float* As = lds;
  float* Bs = lds + kSwdTileP * kSwdLd;

  const int D = a.D, N = a.na + a.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
  const int u0 = blockIdx.x * kSwdTileN, p0 = blockIdx.y * kSwdTileP;

  // this thread's rows of each operand (rows srow + 32 i, four k at sk of a chunk), null past the operand's end
  const int srow = tid >> 3, sk = (tid & 7) * 4;
  const float* pa[4];
  const float* pb[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = p0 + srow + 32 * i;
    pa[i] = p < a.P ? a.dirs + (size_t)p * D : nullptr;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int u = u0 + srow + 32 * i;
    pb[i] = u >= N ? nullptr : u < a.na ? a.real + (size_t)u * D : a.fake + (size_t)(u - a.na) * D;
  }

  f32x16 acc[2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
  float4 ra[4], rb[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) ra[i] = pair_load4<VEC>(pa[i], sk, D);
#pragma unroll
  for (int i = 0; i < 2; ++i) rb[i] = pair_load4<VEC>(pb[i], sk, D);

  for (int k0 = 0; k0 < D; k0 += kSwdBK) {
    __syncthreads();  // the previous chunk's fragments are read
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(As + (srow + 32 * i) * kSwdLd + sk) = ra[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(Bs + (srow + 32 * i) * kSwdLd + sk) = rb[i];
    __syncthreads();
    if (k0 + kSwdBK < D) {  // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
      for (int i = 0; i < 4; ++i) ra[i] = pair_load4<VEC>(pa[i], k0 + kSwdBK + sk, D);
#pragma unroll
      for (int i = 0; i < 2; ++i) rb[i] = pair_load4<VEC>(pb[i], k0 + kSwdBK + sk, D);
    }
    // lane half h takes k = 8 c + 4 h + j of the chunk in MFMA step (c, j), from both operands alike
#pragma unroll
    for (int c = 0; c < kSwdBK / 8; ++c) {
      float4 av[2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
        av[m] = *reinterpret_cast<const float4*>(As + (wr * 64 + m * 32 + r) * kSwdLd + 8 * c + 4 * h);
      const float4 bv = *reinterpret_cast<const float4*>(Bs + (wc * 32 + r) * kSwdLd + 8 * c + 4 * h);
      const float af[2][4] = {{av[0].x, av[0].y, av[0].z, av[0].w}, {av[1].x, av[1].y, av[1].z, av[1].w}};
      const float bf[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int m = 0; m < 2; ++m) acc[m] = mfma32x32x2(af[m][j], bf[j], acc[m]);
    }
  }

  // accumulator register reg of lane (r, h): direction 32 m + (reg & 3) + 8 (reg >> 2) + 4 h of the wave's 64, row r
  const int u = u0 + wc * 32 + r;
  if (u < N) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int p = p0 + wr * 64 + m * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (p < a.P) a.proj[(size_t)p * N + u] = acc[m][reg];
      }
  }
}

// (x, y) in ascending order when `up`, descending otherwise; equal values may trade places
__device__ __forceinline__ void swd_cx(float& x, float& y, bool up) {
  const bool sw = (x > y) == up;
  const float t = x;
  x = sw ? y : x;
  y = sw ? t : y;
}

// Stages k = 2 .. 16 of the network on the run [16 g, 16 g + 16): a sorted run, ascending where bit 4 of its
// first index is clear
__device__ __forceinline__ void swd_sort_run(float* s, int g) {
  const int base = g << kSwdRunBits;
  float v[kSwdRun];
#pragma unroll
  for (int q = 0; q < kSwdRun / 4; ++q) {
    const float4 t = *reinterpret_cast<const float4*>(s + base + 4 * q);
    v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
  }
#pragma unroll
  for (int k = 2; k <= kSwdRun; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
      for (int e = 0; e < kSwdRun; ++e)
        if ((e & j) == 0) swd_cx(v[e], v[e | j], ((base | e) & k) == 0);
#pragma unroll
  for (int q = 0; q < kSwdRun / 4; ++q)
    *reinterpret_cast<float4*>(s + base + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// Strides 2^(b + steps - 1) .. 2^b of stage k on the 16 elements whose indices differ in bits [b, b + 4) and
// agree with unit g elsewhere. b + steps <= log2 k, so the stage's direction is one for the unit.
template <bool LOW>  // b == 0: the elements are contiguous
__device__ __forceinline__ void swd_merge_unit(float* s, int g, int b, int steps, int k) {
  const int base = LOW ? g << kSwdRunBits : ((g >> b) << (b + kSwdRunBits)) | (g & ((1 << b) - 1));
  float v[kSwdRun];
  if (LOW) {
#pragma unroll
    for (int q = 0; q < kSwdRun / 4; ++q) {
      const float4 t = *reinterpret_cast<const float4*>(s + base + 4 * q);
      v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < kSwdRun; ++e) v[e] = s[base + (e << b)];
  }
  const bool up = (base & k) == 0;
#pragma unroll
  for (int t = kSwdRunBits - 1; t >= 0; --t) {
    if (t < steps) {
#pragma unroll
      for (int e = 0; e < kSwdRun; ++e)
        if ((e & (1 << t)) == 0) swd_cx(v[e], v[e | (1 << t)], up);
    }
  }
  if (LOW) {
#pragma unroll
    for (int q = 0; q < kSwdRun / 4; ++q)
      *reinterpret_cast<float4*>(s + base + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  } else {
#pragma unroll
    for (int e = 0; e < kSwdRun; ++e) s[base + (e << b)] = v[e];
  }
}

__device__ __forceinline__ int swd_log2(int pow2) { return 31 - __clz(pow2); }

__global__ __launch_bounds__(kSwdSortThreads) void swd_sort_k(SwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float swd_lds[];
  const int na = a.na, nb = a.nb, N = na + nb;
  const int PA = swd_pad(na), PB = swd_pad(nb);
  float* A = swd_lds;        // [PA] real projections, +inf past na
  float* B = swd_lds + PA;   // [PB] fake projections, +inf past nb
  float* red = B + PB;       // [2][16] wave partials
  const int tid = threadIdx.x;
  float* row = a.proj + (size_t)blockIdx.x * N;

  for (int i = tid; i < PA; i += kSwdSortThreads) A[i] = i < na ? row[i] : kSwdInf;
  for (int i = tid; i < PB; i += kSwdSortThreads) B[i] = i < nb ? row[na + i] : kSwdInf;
  __syncthreads();

  const int ma = swd_log2(PA), mb = swd_log2(PB), mmax = max(ma, mb);
  {  // units of 16 elements: array A's, then array B's
    const int ua = PA >> kSwdRunBits, ub = PB >> kSwdRunBits;
    for (int w = tid; w < ua + ub; w += kSwdSortThreads) swd_sort_run(w < ua ? A : B, w < ua ? w : w - ua);
  }
  for (int L = kSwdRunBits + 1; L <= mmax; ++L) {
    // an array whose length is below 2^L is sorted already
    const int ua = L <= ma ? PA >> kSwdRunBits : 0, ub = L <= mb ? PB >> kSwdRunBits : 0;
    for (int c = L; c > 0;) {
      const int b = max(c - kSwdRunBits, 0), steps = c - b;
      __syncthreads();  // the previous chunk's stores
      for (int w = tid; w < ua + ub; w += kSwdSortThreads) {
        float* s = w < ua ? A : B;
        const int g = w < ua ? w : w - ua;
        if (b == 0) swd_merge_unit<true>(s, g, 0, steps, 1 << L);
        else swd_merge_unit<false>(s, g, b, steps, 1 << L);
      }
      c = b;
    }
  }
  __syncthreads();

  for (int i = tid; i < na; i += kSwdSortThreads) row[i] = A[i];
  for (int i = tid; i < nb; i += kSwdSortThreads) row[na + i] = B[i];

  // the longer side's order statistic i covers cells [i ns, (i + 1) ns): at most two of the shorter side's
  const bool a_long = na >= nb;
  const float* Ls = a_long ? A : B;
  const float* Ss = a_long ? B : A;
  const int nl = a_long ? na : nb, ns = a_long ? nb : na;
  float s1 = 0.f, s2 = 0.f;
  for (int i = tid; i < nl; i += kSwdSortThreads) {
    const float x = Ls[i];
    const int c0 = i * ns, c1 = c0 + ns;
    const int jl = (c1 - 1) / nl;
    for (int j = c0 / nl; j <= jl; ++j) {
      const float len = (float)(min(c1, (j + 1) * nl) - max(c0, j * nl));  // at most 16384: exact
      const float d = x - Ss[j];
      s1 += len * fabsf(d);
      s2 += len * (d * d);
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane_id() == 0) {
    red[wave_id()] = s1;
    red[16 + wave_id()] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    float t1 = 0.f, t2 = 0.f;
    for (int w = 0; w < kSwdSortThreads / kWave; ++w) {
      t1 += red[w];
      t2 += red[16 + w];
    }
    const double cells = (double)na * (double)nb;  // up to 2^28: not always a float
    a.out[(size_t)blockIdx.x * kSwdCols] = (float)((double)t1 / cells);
    a.out[(size_t)blockIdx.x * kSwdCols + 1] = (float)((double)t2 / cells);
  }
}

}  // namespace

}  // namespace mdt

namespace {
int swd_sizes(const mdt::SwdArgs* a) {
  using namespace mdt;
  if (a->na < 2 || a->na > kSwdMaxRows || a->nb < 2 || a->nb > kSwdMaxRows) return 1;
  if (a->D < 1 || a->D > kSwdMaxD) return 2;
  if (a->P < 1 || a->P > kSwdMaxDirs) return 3;
  return 0;
}
}  // namespace

extern "C" int mdt_swd_check(const mdt::SwdArgs* a) {
  const int rc = swd_sizes(a);
  if (rc) return rc;
  return a->real && a->fake && a->dirs && a->proj && a->out ? 0 : 4;
}

extern "C" int mdt_swd_project(const mdt::SwdArgs* a, hipStream_t s) {
  using namespace mdt;
  const int rc = swd_sizes(a);
  if (rc) return rc;
  if (!a->real || !a->fake || !a->dirs || !a->proj) return 4;
  const int N = a->na + a->nb;
  const dim3 pgrid((unsigned)swd_cdiv(N, kSwdTileN), (unsigned)swd_cdiv(a->P, kSwdTileP));
  const bool vec = a->D % 4 == 0 && ((reinterpret_cast<uintptr_t>(a->real) | reinterpret_cast<uintptr_t>(a->fake) |
                                      reinterpret_cast<uintptr_t>(a->dirs)) & 15) == 0;
  if (vec) hipLaunchKernelGGL(swd_project_k<true>, pgrid, dim3(kSwdThreads), 0, s, *a);
  else hipLaunchKernelGGL(swd_project_k<false>, pgrid, dim3(kSwdThreads), 0, s, *a);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}

extern "C" int mdt_swd_sort(const mdt::SwdArgs* a, hipStream_t s) {
  using namespace mdt;
  SwdArgs b = *a;
  b.D = 1;
  const int rc = swd_sizes(&b);
  if (rc) return rc;
  if (!a->proj || !a->out) return 4;
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&swd_sort_k),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSwdSortLdsMax);
  if (attr != hipSuccess) return 9;
  hipLaunchKernelGGL(swd_sort_k, dim3((unsigned)a->P), dim3(kSwdSortThreads), swd_sort_lds(a->na, a->nb), s, *a);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}

extern "C" int mdt_swd_rows(const mdt::SwdArgs* a, hipStream_t s) {
  int rc = mdt_swd_check(a);  // every refusal before the first launch
  if (rc == 0) rc = mdt_swd_project(a, s);
  if (rc == 0) rc = mdt_swd_sort(a, s);
  return rc;
}
