// Two-sample statistics of generated against held-out images (see two_sample.hip):
// per row of the union U = real rows | fake rows, the nearest squared distance
// to a real and to a fake row and the Gaussian-kernel row sums at three
// bandwidths, over all other rows. models/sample_report.py is the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdt {

constexpr int kTsBandwidths = 3;
constexpr int kTsCols = 2 + 2 * kTsBandwidths;  // dmin_r, dmin_f, ksum_r[3], ksum_f[3]
constexpr int kTsMaxRows = 32768;               // per set
constexpr int kTsMaxD = 65536;
constexpr int kTsTile = 128;                    // union rows per operand tile of the pair kernel
constexpr int kTsBK = 32;                       // k per LDS chunk
constexpr int kTsLd = kTsBK + 4;                // LDS row stride (floats): 16-lane groups of a 16-byte read hit 16 slots
constexpr int kTsThreads = 256;
constexpr int kTsNormThreads = 256;             // one wave per row
constexpr int kTsFoldThreads = 256;
constexpr int kTsMaxStrips = 64;
// workgroups the strip count aims at: 4 resident rounds of 2 per CU on 256 CUs
constexpr int kTsBlocks = 2048;

__host__ __device__ inline long long ts_cdiv(long long a, long long b) { return (a + b - 1) / b; }
// G is symmetric, so a pair of tiles is multiplied once: the workgroup of row
// tile I takes the column tiles J = (I + d) mod T at offsets d = 0 .. T/2 and
// gives tile (I, J) to the rows of I and, where 1 <= d and 2 d < T, also to the
// rows of J (at 2 d = T both workgroups meet the pair and each keeps its own
// rows). ts_offsets: the offsets of a row tile; ts_toffsets: those it also
// reduces the other way, one partial per (offset, row).
__host__ __device__ inline int ts_tiles(long long rows) { return (int)ts_cdiv(rows, kTsTile); }
__host__ __device__ inline int ts_offsets(long long rows) { return ts_tiles(rows) / 2 + 1; }
__host__ __device__ inline int ts_toffsets(long long rows) { return (ts_tiles(rows) - 1) / 2; }
// Strips of a row tile's offsets: a function of the union's rows alone (never
// of the device's load), so a pass repeats bitwise. No strip is empty.
inline int ts_strips(long long rows) {
  const long long tiles = ts_tiles(rows), offs = ts_offsets(rows);
  long long s = kTsBlocks / tiles;
  if (s > kTsMaxStrips) s = kTsMaxStrips;
  if (s > offs) s = offs;
  if (s < 1) s = 1;
  return (int)ts_cdiv(offs, ts_cdiv(offs, s));
}

struct TwoSampleArgs {
  int na, nb, D, strips;
  const float* real;  // [na, D]
  const float* fake;  // [nb, D]
  // -1/h_s as a float pair (hi + lo): the exponent's argument is formed to
  // beyond float32, so a kernel sum carries the expf and summation error only
  float c_hi[kTsBandwidths], c_lo[kTsBandwidths];
  float* q;           // [na + nb] squared norms of the union's rows
  float* part;        // [strips][na + nb][kTsCols] one partial per (strip, row)
  float* tpart;       // [ts_toffsets][na + nb][kTsCols] one partial per (offset, row) from the tiles taken the other way
  float* out;         // [na + nb][kTsCols]
};

}  // namespace mdt

extern "C" {
// 0, or why not: 1 na/nb outside [2, 32768], 2 D outside [1, 65536], 3 strips != ts_strips(na + nb), 5 missing buffer
int mdt_two_sample_check(const mdt::TwoSampleArgs* a);
// norms, pair kernel over (row tile, strip of offsets), fold in strip, then offset order -> out
int mdt_two_sample_rows(const mdt::TwoSampleArgs* a, hipStream_t s);
}
