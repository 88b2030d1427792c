// Debiased entropic optimal-transport distance of generated against held-out
// images (see sinkhorn.hip): the three squared-distance matrices of real | fake,
// their scale m, T annealed log-domain Sinkhorn iterations on the pair and on
// the two debiasing problems, and the potentials' table. models/sinkhorn.py is
// the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pair_tile.h"

namespace mdt {

constexpr int kSkCols = 2;          // a table row: the pair's potential, the debiasing potential
constexpr int kSkMaxRows = 16384;   // per set: the cost matrices are stored (3.2 GB at the cap)
constexpr int kSkMaxD = 65536;
constexpr int kSkMaxIters = 10000;
constexpr double kSkMaxBlur = 4.0;
// cost kernel: one kPairTile x kPairTile tile of pair_tile.h per workgroup
constexpr int kSkTLd = 64 + 4;      // the transposing store's row stride: a wave's 32 columns of 64 rows
constexpr int kSkThreads = 256;     // every other kernel
// iteration kernel: a wave keeps kSkWaveRows rows' running (max, sum) in registers, a workgroup's four waves
// own a band of kSkBand rows and walk its columns together, 256 per step (a 16-byte load per lane and row)
constexpr int kSkWaveRows = 16;
constexpr int kSkBand = 4 * kSkWaveRows;
constexpr int kSkChunk = 4 * 64;

__host__ __device__ inline int sk_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
__host__ __device__ inline int sk_pad4(int n) { return (n + 3) & ~3; }

// The workspace, in floats from its 16-byte aligned base. Every offset is a multiple of 4, so every matrix
// row and vector starts on 16 bytes and the double words on 8. An element index inside one matrix is below
// 2^28 and fits 32 bits; the offsets of the matrices do not (3 * 2^28 floats at the cap) and are 64-bit.
struct SkLayout {
  int lda, ldb;      // row strides of a matrix with na / nb columns, and the padded lengths of a vector over them
  int ta, tb;        // cost tiles per side
  int bands_a, bands_b;
  size_t cxy, cxx, cyy;  // [na, ldb], [na, lda], [nb, ldb]
  size_t norms;      // [lda + ldb] squared norms of real | fake
  size_t pots;       // [2][vec]: the double-buffered potentials, a buffer is f [lda] | g [ldb] | p [lda] | q [ldb]
  size_t soft;       // [vec]: an iteration's row softmins, laid out like a buffer (the g part is not used)
  size_t slab;       // [bands_a][ldb][2]: per band of Cxy the columns' (max, sum) partials
  size_t marg;       // [lda] marginal violations of the last iteration
  size_t part;       // double [ta * ta]: per cost workgroup of Cxx the sum of its tile
  size_t scale;      // double [2]: m, and the sum it came from
  size_t total;
  __host__ __device__ int vec() const { return 2 * (lda + ldb); }
};

__host__ __device__ inline SkLayout sk_layout(int na, int nb) {
  SkLayout L;
  L.lda = sk_pad4(na); L.ldb = sk_pad4(nb);
  L.ta = sk_cdiv(na, kPairTile); L.tb = sk_cdiv(nb, kPairTile);
  L.bands_a = sk_cdiv(na, kSkBand); L.bands_b = sk_cdiv(nb, kSkBand);
  size_t o = 0;
  L.cxy = o; o += (size_t)na * L.ldb;
  L.cxx = o; o += (size_t)na * L.lda;
  L.cyy = o; o += (size_t)nb * L.ldb;
  L.norms = o; o += (size_t)L.lda + L.ldb;
  L.pots = o; o += 2 * (size_t)L.vec();
  L.soft = o; o += (size_t)L.vec();
  L.slab = o; o += 2 * (size_t)L.bands_a * L.ldb;
  L.marg = o; o += (size_t)L.lda;
  L.part = o; o += 2 * (size_t)L.ta * L.ta;
  L.scale = o; o += 4;
  L.total = o;
  return L;
}

struct SinkhornArgs {
  int na, nb, D, T;
  double E;           // the blur as a fraction of m
  const float* real;  // [na, D]
  const float* fake;  // [nb, D]
  float* ws;          // [sk_layout(na, nb).total], 16-byte aligned
  float* pot;         // [na + nb, kSkCols] out
  double* out;        // [2] out: m, marg_err
};

}  // namespace mdt

extern "C" {
// 0, or why not: 1 na/nb outside [2, 16384], 2 D outside [1, 65536], 3 E outside (0, 4] or not finite,
// 4 T outside [1, 10000], 5 missing or misaligned buffer
int mdt_sinkhorn_check(const mdt::SinkhornArgs* a);
// the cost phase (norms, the three matrices, m, cleared potentials), then T iterations
int mdt_sinkhorn_rows(const mdt::SinkhornArgs* a, hipStream_t s);
// The two phases alone (the tests and bench/sinkhorn.py use them): the first needs real, fake and ws; the
// second runs iteration t of T on a workspace the first has filled and iterations 0 .. t-1 have advanced (it
// ignores D and the rows; pot and out are written when t == T - 1). Same refusals, and 4 for t outside [0, T).
int mdt_sinkhorn_cost(const mdt::SinkhornArgs* a, hipStream_t s);
int mdt_sinkhorn_step(const mdt::SinkhornArgs* a, int t, hipStream_t s);
}
