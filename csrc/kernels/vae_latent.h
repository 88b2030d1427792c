// Latent report pass of both VAE trainers (see vae_latent.hip).
#pragma once
#include "vae_mlp.h"

namespace mdt {

constexpr uint32_t kLatentStream = 3u << 28;  // Philox stream word of the pass (no rng_stream: replicas agree)
constexpr int kLatMaxZ = 64;                  // one row per lane: Z accumulator pairs live in VGPRs
constexpr int kLatRowTile = 64;               // i rows per pair workgroup (one wave, one row per lane)
constexpr int kLatJTile = 16;                 // j rows per LDS tile: 16 * ceil4(Z) float4 <= 16 KiB
constexpr int kLatPrepRows = 16;              // rows per prep workgroup (= rows per statistics partial)
constexpr int kLatFinRows = 64;               // rows per finish workgroup (= rows per row-mean partial)
constexpr int kLatMaxSplits = 64;
// j-split target: one resident round of single-wave workgroups on 256 CUs x 4 SIMDs x 2 waves
constexpr int kLatWaveSlots = 2048;

// Device state of a pass: a TrainState of its own (the encoder's first kernel
// advances the step there, latent_collect_k the cursor; sched_off = 1)
// followed by the results. The train, eval and iw states are never touched.
struct LatentState {
  TrainState st;
  double kl;          // sum_d kl_per_dim
  double mi, tc, dwkl, sampled_kl;   // per-row means, nats
};

__host__ __device__ inline int lat_zt(int Z) { return (Z + 3) / 4 * 4; }  // latent width the pair kernel is built for
inline long long lat_cdiv(long long a, long long b) { return (a + b - 1) / b; }
// j-splits of the pair kernel: a function of n alone (never of the device's
// load), so a pass is reproducible.
inline int lat_splits(long long n) {
  const long long it = lat_cdiv(n, kLatRowTile), jt = lat_cdiv(n, kLatJTile);
  long long s = kLatWaveSlots / it;
  if (s > kLatMaxSplits) s = kLatMaxSplits;
  if (s > jt) s = jt;
  return s < 1 ? 1 : (int)s;
}

struct LatentArgs {
  long long n;           // rows of the pass
  int Z, splits;
  const float* mulv;     // [n, 2Z] rows mu | lv
  float *eps, *z;        // [n, Z]
  float4* pk;            // [n, zt] (mu, -exp(-lv)/2, -(lv + log 2pi)/2, 0); zero past Z
  float *lq_cond, *lp, *lq_joint, *lq_marg;   // [n]
  float *acc_m, *acc_s;  // [splits][zt + 1][n] running max / scaled sum (accumulator zt = the joint)
  double* stat;          // [nblk_prep][4][Z]: sum mu, sum mu^2, sum kl_d, sum exp(lv) of kLatPrepRows rows
  double* part;          // [nblk_fin][4]: sum of cond-joint, joint-marg, marg-lp, cond-lp of kLatFinRows rows
  float *kl_per_dim, *mu_var, *post_var;      // [Z]
  LatentState* lst;
  const HParams* hp;
};

}  // namespace mdt

extern "C" {
// 0, or the reason the arguments are outside the domain 1 <= Z <= 64, 1 <= n, n*Z <= 2^32, 1 <= splits <= tiles
int mdt_latent_check(const mdt::LatentArgs* a);
int mdt_latent_report(const mdt::LatentArgs* a, hipStream_t s);   // prep, pair, finish, fold
int mdt_latent_pair(const mdt::LatentArgs* a, hipStream_t s);     // the pair kernel alone (timing)
// batch rows mulv[:M] -> pass rows cursor*B + i, then the cursor advances
int mdt_latent_collect(const float* mulv, int M, int B, int Z, float* rows, long long rows_cap, void* lst,
                       hipStream_t s);
// MLP-VAE: F1's split-K slabs -> mulv[M, 2Z], in iw_sample_k's order
int mdt_latent_mulv(const mdt::VaeArgs* a, hipStream_t s);
}
