// Lloyd's k-means on image rows for the NDB / JSD mode-coverage score (see
// kmeans.hip): K centroids started from given real rows, T fixed iterations of
// assign / update / fold over the real rows, then one assignment of real | fake
// to the final centroids. models/ndb.py is the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdt {

constexpr int kKmMaxK = 256;
constexpr int kKmMaxRows = 65536;   // per set
constexpr int kKmMaxD = 65536;
constexpr int kKmMaxIters = 1000;
constexpr int kKmThreads = 256;
// assign: a band of 64 or 32 rows against every centroid, 32 x 32 MFMA tiles, D in LDS chunks of kKmBK
constexpr int kKmBK = 32;
constexpr int kKmLd = kKmBK + 4;    // LDS row stride (floats): 16-lane groups of a 16-byte read hit 16 slots
constexpr int kKmCus = 256;
// update: a workgroup sums kKmSplitRows rows of a 64-column slab of X per cell
constexpr int kKmSlab = 64;
constexpr int kKmSplitRows = 1024;
// fold: a workgroup finishes kKmFoldCols columns of one centroid and leaves that segment's part of |c|^2
constexpr int kKmFoldCols = 2048;
constexpr int kKmMaxSegs = kKmMaxD / kKmFoldCols;

__host__ __device__ inline int km_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
__host__ __device__ inline int km_kpad(int K) { return (K + 31) & ~31; }
// the band height: 64 rows, or 32 while 64 would leave compute units without a band
__host__ __device__ inline int km_band(int n) { return km_cdiv(n, 64) >= kKmCus ? 64 : 32; }
__host__ __device__ inline int km_bands(int n) { return km_cdiv(n, km_band(n)); }
__host__ __device__ inline int km_splits(int n) { return km_cdiv(n, kKmSplitRows); }
__host__ __device__ inline int km_segs(int D) { return km_cdiv(D, kKmFoldCols); }
// dynamic LDS of the assign kernel: two buffers of (band + kpad) staged rows
__host__ __device__ inline size_t km_assign_lds(int band, int kpad) {
  return 2 * (size_t)(band + kpad) * kKmLd * sizeof(float);
}

// The workspace, in 4-byte words from its 16-byte aligned base.
struct KmLayout {
  size_t c2;      // float [K][segs]: |c_k|^2 by column segment
  size_t band;    // int [bands(na + nb)]: labels changed per band of the last assign
  size_t cnt;     // int [splits][kKmMaxK]: rows per cell and row split
  size_t part;    // float [splits][K][D]: the column sums per cell and row split
  size_t total;
};

__host__ __device__ inline KmLayout km_layout(int na, int nb, int D, int K) {
  KmLayout L;
  const int R = km_splits(na);
  size_t o = 0;
  L.c2 = o; o += (size_t)kKmMaxK * kKmMaxSegs;
  L.band = o; o += ((size_t)km_cdiv(na + nb, 32) + 3) & ~(size_t)3;
  L.cnt = o; o += (size_t)R * kKmMaxK;
  L.part = o; o += (((size_t)R * K * D) + 3) & ~(size_t)3;
  L.total = o;
  return L;
}

struct KmeansArgs {
  int na, nb, D, K, T;
  const float* real;        // [na, D]
  const float* fake;        // [nb, D] (nb may be 0: then unused)
  const long long* init;    // [K] distinct real-row indices (kmeans_rows only)
  float* ws;                // [km_layout(na, nb, D, K).total], 16-byte aligned
  float* cent;              // [K, D] in/out
  int* labels;              // [na + nb] out (assign: also the previous labels when prev is set)
  float* mind;              // [na + nb] out
  int* moved;               // [T] out (kmeans_rows), [1] (assign)
  int* counts;              // [K] out (update)
  double* inertia;          // [1] out: sum of mind over the real rows
};

}  // namespace mdt

extern "C" {
// 0, or why not: 1 rows outside [2, 65536] (nb: 0 or that), 2 D outside [1, 65536], 3 K outside [2, 256] (a fit: or above
// na), 4 T outside [1, 1000], 5 missing or misaligned buffer
int mdt_kmeans_check(const mdt::KmeansArgs* a);
// centroids from init, T iterations on the real rows, the final assignment of real | fake
int mdt_kmeans_rows(const mdt::KmeansArgs* a, hipStream_t s);
// The steps alone. assign: labels, mind and moved[0] of real | fake against cent; `prev` != 0 counts the rows whose
// label differs from what labels held, else every row. update: counts and the new cent from labels of the real rows.
int mdt_kmeans_assign(const mdt::KmeansArgs* a, int prev, hipStream_t s);
int mdt_kmeans_update(const mdt::KmeansArgs* a, hipStream_t s);
}
