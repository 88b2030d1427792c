// Precision, recall, density and coverage of generated against held-out images on
// k-nearest-neighbour radii (see prdc.hip): per row of real | fake the k-th
// smallest squared distance to another row of its own set, the number of rows
// of the other set whose radius ball holds it, and the nearest squared distance
// to the other set. models/prdc.py is the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pair_tile.h"  // kPairTile: rows per operand tile

namespace mdt {

constexpr int kPrdcMaxK = 8;       // slots of a row's k-list
constexpr int kPrdcCols = 3;       // a table row: rad, cnt, dminx
constexpr int kPrdcMaxRows = 32768;  // per set
constexpr int kPrdcMaxD = 65536;
constexpr int kPrdcRowThreads = 256;  // the per-row kernels
constexpr int kPrdcMaxStrips = 64;
// workgroups the radius kernel's strip count aims at: 4 resident rounds of 2 per CU on 256 CUs
constexpr int kPrdcBlocks = 2048;

__host__ __device__ inline long long prdc_cdiv(long long a, long long b) { return (a + b - 1) / b; }
__host__ __device__ inline int prdc_tiles(long long rows) { return (int)prdc_cdiv(rows, kPairTile); }
// Strips of a row tile's column tiles: a function of (na, nb) alone, never of the
// device's load. Strip s of a set of T tiles takes the column tiles
// [s * per, min(T, (s + 1) * per)) with per = ceil(T / strips); the set with
// fewer tiles leaves its last strips empty (their k-lists stay at +inf).
inline int prdc_strips(long long na, long long nb) {
  const long long ta = prdc_tiles(na), tb = prdc_tiles(nb), tmax = ta > tb ? ta : tb;
  long long s = kPrdcBlocks / (ta + tb);
  if (s > kPrdcMaxStrips) s = kPrdcMaxStrips;
  if (s > tmax) s = tmax;
  if (s < 1) s = 1;
  return (int)prdc_cdiv(tmax, prdc_cdiv(tmax, s));
}

struct PrdcArgs {
  int na, nb, D, k, strips;
  const float* real;  // [na, D]
  const float* fake;  // [nb, D]
  float* q;           // [na + nb] squared norms
  float* rad;         // [na + nb] k-th smallest same-set d2
  int* cnt;           // [na + nb] membership counts
  unsigned* dminx;    // [na + nb] nearest d2 to the other set, as float bits (d2 >= 0: unsigned order is float order)
  float* lists;       // [strips][na + nb][kPrdcMaxK] one k-list per (strip, row)
  float* out;         // [na + nb][kPrdcCols]
};

}  // namespace mdt

extern "C" {
// 0, or why not: 1 na/nb outside [k + 1, 32768], 2 D outside [1, 65536], 3 strips != prdc_strips(na, nb),
// 4 k outside [1, 8], 5 missing buffer
int mdt_prdc_check(const mdt::PrdcArgs* a);
// norms, radius kernel over (row tile of either set, strip), radius fold, membership kernel over
// (real tile, strip of fake tiles), final fold -> out
int mdt_prdc_rows(const mdt::PrdcArgs* a, hipStream_t s);
}
