// Total-correlation penalty of a training batch, both VAE trainers (see vae_tc.hip).
#pragma once
#include "vae_latent.h"

namespace mdt {

constexpr int kTcPackThreads = 256;
constexpr int kTcFoldThreads = 256;

// d-chunk of the column pass (g_mu, g_lv): its accumulators are 2 * chunk VGPRs
// on top of the lane's packed row (3 ZT)
__host__ __device__ inline int tc_chunk(int zt) { return zt % 8 == 0 ? 8 : 4; }
// Splits of the streamed side (j in the pair kernel and the row pass, i in the
// column pass): a function of the batch rows alone, so a step repeats bitwise.
inline int tc_splits(int M, int /*Z*/) { return lat_splits(M); }

struct TcArgs {
  int M, Z, splits;
  const float* mulv;     // [M, 2Z] rows mu | lv of the step
  const float* eps;      // [M, Z] the step's noise
  float* z;              // [M, Z]  f32 z = mu + eps exp(lv/2)
  float4* pk;            // [M, zt] (mu, -exp(-lv)/2, -(lv + log 2pi)/2, 0); zero past Z
  float *acc_m, *acc_s;  // [splits][zt + 1][M]: the pair kernel's running max / scaled sum
  float* lse_d;          // [M, zt] m[i,d] = logsumexp_j t[i,j,d]
  float* lse_j;          // [M]     J[i]   = logsumexp_j sum_d t[i,j,d]
  float *gz, *gmu, *glv; // [splits][M][zt] partial sums of the two backward passes
  float* csum;           // [splits][M][zt + 1] the row pass's sums of exp(t - m) per (i, d) and of exp(sum_d t - J)
  const float* tcw;      // the step's weight: TrainState.tc_t (or a plain device float)
  TrainState* st;        // optional: epoch_tc += tc_batch
  double* value;         // [1] tc_batch of the step (unweighted)
  float* add_out;        // optional [M, 2Z]: tc_t * d tc_batch / d[mu|lv]
  float* dmulv;          // optional [M, 2Z]: the same added in place ...
  void* dmulv16;         // ... and its bf16 copy written again (optional)
};

}  // namespace mdt

extern "C" {
// 0, or why the arguments are outside 1 <= M <= 4096, 1 <= Z <= 64, 1 <= splits <= min(64, ceil(M/16))
int mdt_tc_check(const mdt::TcArgs* a);
// pack, pair, merge: lse_d, lse_j
int mdt_tc_forward(const mdt::TcArgs* a, hipStream_t s);
// row pass + column pass (one launch) into gz / gmu / glv
int mdt_tc_backward(const mdt::TcArgs* a, hipStream_t s);
// partials in split order -> value, epoch_tc, add_out and / or dmulv (+ dmulv16)
int mdt_tc_fold(const mdt::TcArgs* a, hipStream_t s);
// latent_pair_k over operands the caller packed (vae_latent.hip): reads n, Z, splits, z, pk, acc_m, acc_s only
int mdt_latent_pair_operands(const mdt::LatentArgs* a, hipStream_t s);
}
