// Sliced Wasserstein distance of generated against held-out images (see
// swd.hip): the projections of real | fake on P directions, sorted per set and
// direction, and per direction the first and squared second Wasserstein
// distance of the two one-dimensional empirical measures. models/swd.py is the
// definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdt {

constexpr int kSwdCols = 2;          // a table row: w1, w2sq
constexpr int kSwdMaxRows = 16384;   // per set: both sorted sets of a projection in one workgroup's LDS
constexpr int kSwdMaxD = 65536;
constexpr int kSwdMaxDirs = 4096;
// projection kernel: a tile of kSwdTileP directions by kSwdTileN rows per workgroup, 2 x 1 MFMA tiles per wave.
// The rows are the operand that is read once per direction tile, so the direction tile is the tall one.
constexpr int kSwdTileP = 128;
constexpr int kSwdTileN = 64;
constexpr int kSwdBK = 32;           // k per LDS chunk
constexpr int kSwdLd = kSwdBK + 4;   // LDS row stride (floats): 16-lane groups of a 16-byte read hit 16 slots
constexpr int kSwdThreads = 256;
// sort kernel: one workgroup per direction; a thread's register run is kSwdRun elements (four strides of the
// bitonic network between two barriers)
constexpr int kSwdSortThreads = 1024;
constexpr int kSwdRunBits = 4;
constexpr int kSwdRun = 1 << kSwdRunBits;

__host__ __device__ inline int swd_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// An array's length in LDS: the next power of two, at least one register run; the tail holds +inf
__host__ __device__ inline int swd_pad(int n) {
  int p = kSwdRun;
  while (p < n) p <<= 1;
  return p;
}
// Dynamic LDS of the sort kernel: both padded arrays and the reduction's 2 x 16 wave partials
inline size_t swd_sort_lds(int na, int nb) { return sizeof(float) * ((size_t)swd_pad(na) + swd_pad(nb) + 32); }
constexpr size_t kSwdSortLdsMax = sizeof(float) * (2 * kSwdMaxRows + 32);

struct SwdArgs {
  int na, nb, D, P;
  const float* real;  // [na, D]
  const float* fake;  // [nb, D]
  const float* dirs;  // [P, D]
  float* proj;        // [P, na + nb] out: per direction the sorted real | the sorted fake projections
  float* out;         // [P, kSwdCols]
};

}  // namespace mdt

extern "C" {
// 0, or why not: 1 na/nb outside [2, 16384], 2 D outside [1, 65536], 3 P outside [1, 4096], 4 missing buffer
int mdt_swd_check(const mdt::SwdArgs* a);
// projections over (row tile, direction tile), then sort + integrate per direction
int mdt_swd_rows(const mdt::SwdArgs* a, hipStream_t s);
// The two launches alone (bench/swd.py times them): the first needs real, fake, dirs and proj, the second
// proj and out (and ignores D). Same refusals.
int mdt_swd_project(const mdt::SwdArgs* a, hipStream_t s);
int mdt_swd_sort(const mdt::SwdArgs* a, hipStream_t s);
}
