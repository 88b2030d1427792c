// Ex-post Gaussian-mixture prior, fitted by EM (see gmm.hip): K full-covariance
// components on rows z [n, Z]. models/gmm.py is the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdt {

constexpr int kGmmMaxK = 32;
constexpr int kGmmMaxZ = 64;
constexpr int kGmmMaxRows = 1 << 20;
constexpr int kGmmMaxIters = 1000;
constexpr float kGmmRegCovar = 1e-4f;
constexpr float kGmmDeadWeight = 1e-6f;
constexpr int kGmmThreads = 256;
constexpr int kGmmTile = 128;   // rows per E-step workgroup, 32 per wave
constexpr int kGmmBlocks = 512; // the M-step's target number of workgroups

__host__ __device__ inline int gmm_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
__host__ __device__ inline int gmm_zpad(int Z) { return 16 * gmm_cdiv(Z, 16); }
// LDS row stride of a [.., zpad] operand: 16-lane groups of an MFMA fragment read hit distinct banks
__host__ __device__ inline int gmm_ld(int Z) { return gmm_zpad(Z) + 4; }
// One component's M-step record: N_k, sum r d [Z], sum r d d^T [Z, Z] (blocks on and below the diagonal only)
__host__ __device__ inline int gmm_rec(int Z) { return 1 + Z + Z * Z; }
__host__ __device__ inline int gmm_tiles(int n) { return gmm_cdiv(n, kGmmTile); }
// Row tiles per M-step strip and the number of strips: a function of (n, K) alone, so that the fold order,
// and with it every bit of the fit, does not depend on the device.
__host__ __device__ inline int gmm_strip_tiles(int n, int K) {
  const int want = gmm_cdiv(kGmmBlocks, K);
  return gmm_cdiv(gmm_tiles(n), want < 1 ? 1 : want);
}
__host__ __device__ inline int gmm_strips(int n, int K) { return gmm_cdiv(gmm_tiles(n), gmm_strip_tiles(n, K)); }

// Dynamic LDS (floats) of the E-step: the row tile, two W_k buffers, two mu_k, the tile's lp and ll
inline size_t gmm_estep_lds(int Z, int K) {
  return sizeof(float) * ((size_t)kGmmTile * gmm_ld(Z) + 2 * (size_t)gmm_zpad(Z) * gmm_ld(Z) + 2 * kGmmMaxZ +
                          (size_t)kGmmTile * (K + 1) + kGmmTile + 8);
}

// The workspace, in floats: offsets of its parts
struct GmmWs {
  size_t W, c, status, llpart, mpart, r, ll, total;
};
inline GmmWs gmm_ws_layout(int n, int Z, int K) {
  GmmWs w;
  size_t o = 0;
  auto take = [&o](size_t m) { const size_t at = o; o += (m + 3) & ~(size_t)3; return at; };
  w.W = take((size_t)K * Z * Z);
  w.c = take(K);
  w.status = take(K);
  w.llpart = take(gmm_tiles(n));
  const size_t recs = (size_t)gmm_strips(n, K) * K, recs1 = gmm_strips(n, 1);  // the start's moments run with K = 1
  w.mpart = take((recs > recs1 ? recs : recs1) * gmm_rec(Z));
  w.r = take((size_t)n * K);
  w.ll = take(n);
  w.total = o;
  return w;
}

struct GmmArgs {
  int n, Z, K;
  float reg;
  const float* z;   // [n, Z]
  float* pi;        // [K]       the parameters: read, and by a fit replaced
  float* mu;        // [K, Z]
  float* cov;       // [K, Z, Z]
  float* pi_out;    // em_step: where the next parameters go (a fit: pi, mu, cov themselves)
  float* mu_out;
  float* cov_out;
  float* W;         // [K, Z, Z] out: L_k^-1, zero above the diagonal
  float* c;         // [K] out
  float* status;    // [K] out: 1.0 where a pivot was not positive
  float* r;         // [n, K] out (null: not written)
  float* ll;        // [n] out
  float* llpart;    // [tiles] per-tile sums of ll
  float* mpart;     // [strips, K, rec] M-step partials
  float* ll_hist;   // fit: [iters + 1] out
};

}  // namespace mdt

extern "C" {
// 0, or why not: 1 n outside (K, 2^20], 2 Z outside [1, 64], 3 K outside [1, 32], 4 missing buffer,
// 5 iters outside [0, 1000]
int mdt_gmm_check(const mdt::GmmArgs* a);
// the start, `iters` times (E, M, fold + prepare), one last E; 3 launches per iteration
int mdt_gmm_fit(const mdt::GmmArgs* a, int iters, hipStream_t s);
// prepare, E, M and the fold of one iteration from (pi, mu, cov) into the *_out parameters; W and c stay
// those of the input parameters
int mdt_gmm_em_step(const mdt::GmmArgs* a, hipStream_t s);
// prepare and E only: ll [n]
int mdt_gmm_score(const mdt::GmmArgs* a, hipStream_t s);
}
