// Reconstruction report: per image pair (x, r) of S x S pixels the squared error
// and the SSIM (Wang et al. 2004: 11x11 Gaussian window, sigma 1.5, valid
// positions, C1 = 0.01^2, C2 = 0.03^2) with its luminance and contrast-structure
// means. models/recon_report.py is the definition; docs/KERNELS.md, "Reconstruction
// report", has the design, the resource table and the measurements.
//
// One tile routine, recon_tile<GROUP>, serves both kernels. A tile is `rows_in`
// consecutive input rows of one image pair and the rows_in - 10 output rows they
// cover. Its three steps, each followed by a synchronisation of the GROUP lanes:
//   stage: both images' rows go to LDS once, shifted by -0.5 (variances and the
//          covariance are shift-invariant, and the terms that cancel in
//          sum w x^2 - mx^2 shrink from x^2 <= 1 to (x - 0.5)^2 <= 0.25); the
//          squared error comes out of the same loads, from the unshifted values;
//   horizontal: a lane owns kReconRun output columns of one input row: it walks
//          the run's 16 input positions once, forms the five products on the fly
//          and feeds each into the (up to 6) windows that hold it; lanes of a
//          wave walk down a column (odd row strides: distinct banks);
//   vertical: a lane owns an output position, reads 11 rows of the five filtered
//          maps, forms l, cs and l * cs and adds them to its three sums.
// recon_wave_k: sides up to 32, a wavefront per image and its own LDS slice, no
// workgroup barrier (a wave's LDS operations run in order). recon_band_k: a
// workgroup per (image, band of output rows); recon_fold_k adds the band sums in
// band order. Every sum has a fixed order (a lane's positions in index order, a
// shuffle tree over the lanes, waves and bands in order): no atomics, results
// repeat bitwise and do not depend on n or on where an image is scheduled.
// No matrix instructions: the separable filter is 2 x 11 multiply-adds per
// position and map; as two banded GEMMs it would be S + S of them.
#include "recon.h"

// every sum below is written out: no contraction beyond the fmaf calls
#pragma clang fp contract(off)

namespace mdt {
namespace {

constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f, kShift = 0.5f;

// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, rounded once to float
__device__ constexpr float kTap[kReconWin] = {
    (float)0.00102838008447911,  (float)0.007598758135239185, (float)0.03600077212843083, (float)0.10936068950970002,
    (float)0.2130055377112537,   (float)0.26601172486179436,  (float)0.2130055377112537,  (float)0.10936068950970002,
    (float)0.03600077212843083,  (float)0.007598758135239185, (float)0.00102838008447911};

template <int GROUP>
__device__ inline void group_sync() {
  if constexpr (GROUP == 64) {
    // one wave's LDS operations run in order; keep the compiler's too
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

__device__ inline float wave_sum(float v) {  // a fixed tree: lane 0 holds the sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// x, r: the first of the tile's rows_in input rows. se_rows: the leading rows whose
// squared error this tile counts. Lane t == 0 of the group returns out[4] = the
// sums of (x - r)^2 over those rows and of l * cs, l, cs over the tile's positions.
template <int GROUP>
__device__ inline void recon_tile(const float* __restrict__ x, const float* __restrict__ r, int S, int rows_in,
                                  int se_rows, bool vec, float* lds, int t, float out[kReconCols]) {
  const int W = S - (kReconWin - 1), ldi = recon_in_ld(S), ldm = recon_map_ld(S);
  float* lx = lds;
  float* lr = lx + rows_in * ldi;
  float* maps = lr + rows_in * ldi;
  const int map_sz = rows_in * ldm;

  float se = 0.0f;
  const int total = rows_in * S;
  if (vec) {  // S % 4 == 0 and 16-byte aligned bases: a quad never leaves its row
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const float4* r4 = reinterpret_cast<const float4*>(r);
    for (int q = t; q < total / 4; q += GROUP) {
      const float4 a = x4[q], b = r4[q];
      const int row = (4 * q) / S, at = row * ldi + (4 * q - row * S);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        lx[at + i] = av[i] - kShift;
        lr[at + i] = bv[i] - kShift;
        const float d = av[i] - bv[i];
        if (row < se_rows) se += d * d;
      }
    }
  } else {
    for (int e = t; e < total; e += GROUP) {
      const float a = x[e], b = r[e];
      const int row = e / S, at = row * ldi + (e - row * S);
      lx[at] = a - kShift;
      lr[at] = b - kShift;
      const float d = a - b;
      if (row < se_rows) se += d * d;
    }
  }
  group_sync<GROUP>();

  const int runs = (W + kReconRun - 1) / kReconRun;
  for (int it = t; it < runs * rows_in; it += GROUP) {
    const int run = it / rows_in, row = it - run * rows_in, c0 = run * kReconRun;
    float acc[kReconRun][kReconMaps];
#pragma unroll
    for (int j = 0; j < kReconRun; ++j)
#pragma unroll
      for (int m = 0; m < kReconMaps; ++m) acc[j][m] = 0.0f;
#pragma unroll
    for (int p = 0; p < kReconRun + kReconWin - 1; ++p) {
      const int col = min(c0 + p, S - 1);  // past the row's end only for windows that are not stored
      const float a = lx[row * ldi + col], b = lr[row * ldi + col];
      const float prod[kReconMaps] = {a, b, a * a, b * b, a * b};
#pragma unroll
      for (int j = 0; j < kReconRun; ++j) {
        if (p - j >= 0 && p - j < kReconWin) {  // window j holds position p at tap p - j: taps arrive in order
#pragma unroll
          for (int m = 0; m < kReconMaps; ++m) acc[j][m] = fmaf(kTap[p - j], prod[m], acc[j][m]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kReconRun; ++j)
      if (c0 + j < W) {
#pragma unroll
        for (int m = 0; m < kReconMaps; ++m) maps[m * map_sz + row * ldm + c0 + j] = acc[j][m];
      }
  }
  group_sync<GROUP>();

  float s_ssim = 0.0f, s_l = 0.0f, s_cs = 0.0f;
  const int npos = (rows_in - (kReconWin - 1)) * W;
  for (int p = t; p < npos; p += GROUP) {
    const int y = p / W, xx = p - y * W;
    float v[kReconMaps];
#pragma unroll
    for (int m = 0; m < kReconMaps; ++m) {
      const float* col = maps + m * map_sz + y * ldm + xx;
      float s = 0.0f;
#pragma unroll
      for (int k = 0; k < kReconWin; ++k) s = fmaf(kTap[k], col[k * ldm], s);
      v[m] = s;
    }
    const float vx = v[2] - v[0] * v[0], vy = v[3] - v[1] * v[1], vxy = v[4] - v[0] * v[1];
    const float mx = v[0] + kShift, my = v[1] + kShift;
    const float l = (2.0f * mx * my + kC1) / (mx * mx + my * my + kC1);
    const float cs = (2.0f * vxy + kC2) / (vx + vy + kC2);
    s_ssim += l * cs;
    s_l += l;
    s_cs += cs;
  }

  float part[kReconCols] = {wave_sum(se), wave_sum(s_ssim), wave_sum(s_l), wave_sum(s_cs)};
  if constexpr (GROUP > 64) {
    __syncthreads();  // the staged inputs are long read: the head of their LDS takes the waves' sums
    if ((t & 63) == 0) {
#pragma unroll
      for (int c = 0; c < kReconCols; ++c) lds[(t >> 6) * kReconCols + c] = part[c];
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
      for (int c = 0; c < kReconCols; ++c) {
        float s = lds[c];
        for (int w = 1; w < GROUP / 64; ++w) s += lds[w * kReconCols + c];
        part[c] = s;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kReconCols; ++c) out[c] = part[c];
}

__global__ __launch_bounds__(64 * kReconWaves) void recon_wave_k(ReconArgs a, int vec) {
  extern __shared__ float smem[];
  const int S = a.side, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long img = (long long)blockIdx.x * kReconWaves + wave;
  if (img >= a.n) return;  // no workgroup barrier below
  const size_t base = (size_t)img * S * S;
  float out[kReconCols];
  recon_tile<64>(a.real + base, a.recon + base, S, S, S, vec != 0, smem + wave * recon_lds_floats(S, S), lane, out);
  if (lane == 0) {
    const float npos = (float)((S - (kReconWin - 1)) * (S - (kReconWin - 1)));
    float* row = a.table + (size_t)img * kReconCols;
    row[0] = out[0];
#pragma unroll
    for (int c = 1; c < kReconCols; ++c) row[c] = out[c] / npos;
  }
}

__global__ __launch_bounds__(kReconThreads) void recon_band_k(ReconArgs a, int vec) {
  extern __shared__ float smem[];
  const int S = a.side, H = S - (kReconWin - 1), R = recon_band_rows(S);
  const unsigned img = blockIdx.x / a.bands, band = blockIdx.x - img * a.bands;
  const int o0 = band * R, o1 = min(H, o0 + R), rows_in = o1 - o0 + kReconWin - 1;
  // a band counts the squared error of the input rows it starts at; the last one also of its halo
  const int se_rows = (int)band == a.bands - 1 ? rows_in : o1 - o0;
  const size_t base = (size_t)img * S * S + (size_t)o0 * S;
  float out[kReconCols];
  recon_tile<kReconThreads>(a.real + base, a.recon + base, S, rows_in, se_rows, vec != 0, smem, threadIdx.x, out);
  if (threadIdx.x == 0) {
    float* row = a.partial + (size_t)blockIdx.x * kReconCols;
#pragma unroll
    for (int c = 0; c < kReconCols; ++c) row[c] = out[c];
  }
}

__global__ __launch_bounds__(kReconThreads) void recon_fold_k(ReconArgs a) {
  const int img = blockIdx.x * kReconThreads + threadIdx.x;
  if (img >= a.n) return;
  const float* p = a.partial + (size_t)img * a.bands * kReconCols;
  float s[kReconCols] = {p[0], p[1], p[2], p[3]};
  for (int b = 1; b < a.bands; ++b)
#pragma unroll
    for (int c = 0; c < kReconCols; ++c) s[c] += p[b * kReconCols + c];
  const float npos = (float)((a.side - (kReconWin - 1)) * (a.side - (kReconWin - 1)));
  float* row = a.table + (size_t)img * kReconCols;
  row[0] = s[0];
#pragma unroll
  for (int c = 1; c < kReconCols; ++c) row[c] = s[c] / npos;
}

}  // namespace
}  // namespace mdt

using namespace mdt;

extern "C" int mdt_recon_check(const ReconArgs* a) {
  if (a->n < 1 || a->n > kReconMaxRows) return 1;
  if (a->side < kReconMinSide || a->side > kReconMaxSide) return 2;
  if (a->bands != recon_bands(a->side)) return 3;
  if (!a->real || !a->recon || !a->table || (a->side > kReconWaveSide && !a->partial)) return 4;
  return 0;
}

extern "C" int mdt_recon_rows(const ReconArgs* a, hipStream_t s) {
  const int rc = mdt_recon_check(a);
  if (rc) return rc;
  static const hipError_t attr_w = hipFuncSetAttribute(reinterpret_cast<const void*>(&recon_wave_k),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kReconLds1);
  static const hipError_t attr_b = hipFuncSetAttribute(reinterpret_cast<const void*>(&recon_band_k),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, kReconLds1);
  if (attr_w != hipSuccess || attr_b != hipSuccess) return 9;
  const int S = a->side;
  const int vec = S % 4 == 0 && (reinterpret_cast<uintptr_t>(a->real) | reinterpret_cast<uintptr_t>(a->recon)) % 16 == 0;
  if (S <= kReconWaveSide) {
    const int lds = kReconWaves * recon_lds_floats(S, S) * (int)sizeof(float);
    hipLaunchKernelGGL(recon_wave_k, dim3((a->n + kReconWaves - 1) / kReconWaves), dim3(64 * kReconWaves), lds, s, *a, vec);
  } else {
    const int lds = recon_lds_floats(S, recon_band_rows(S) + kReconWin - 1) * (int)sizeof(float);
    hipLaunchKernelGGL(recon_band_k, dim3((unsigned)a->n * a->bands), dim3(kReconThreads), lds, s, *a, vec);
    hipLaunchKernelGGL(recon_fold_k, dim3((a->n + kReconThreads - 1) / kReconThreads), dim3(kReconThreads), 0, s, *a);
  }
  return hipGetLastError() == hipSuccess ? 0 : 9;
}
