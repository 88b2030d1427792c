// Importance-weighted test log-likelihood pass of the MLP-VAE (see vae_iw.hip).
#pragma once
#include "vae_mlp.h"

namespace mdt {

constexpr uint32_t kIwStream = 1u << 29;  // Philox stream word of the pass (no rng_stream: replicas agree)
constexpr int kIwRowTile = 32;            // virtual rows per decoder workgroup
constexpr int kIwMaxLds = 64 * 1024;      // decoder A tile: kIwRowTile * (ceil16(H) + 4) floats

// Device state of a pass: a TrainState of its own (F1 reads the cursor and
// advances the step there; sched_off = 1) followed by the pass totals. The
// train and eval states are never touched.
struct IwState {
  TrainState st;
  double nll;        // sum of row_nll over the rows reduced so far (fixed order)
  double neg_elbo;   // sum of row_neg_elbo
};

// One chunk of S samples k0 .. k0+S-1 of a batch of M rows. Virtual row
// v = s*M + i (sample s of the chunk, batch row i).
struct IwArgs {
  int M, B, D, H, Z;
  int K, k0, S;
  int first, last;       // first / last chunk of the batch
  int cap_rows;          // capacity (virtual rows) of h3 / bce / prior / eps / z
  long long rows_cap;    // capacity of row_nll / row_neg_elbo
  const float *b2, *W3, *b3, *W4, *b4;
  const float* slab_mv;  // F1's [mu|lv] split-K slabs
  const float* xb;       // F1's copy of the batch rows [M, D]
  float* mulv;           // [M, 2Z]
  float *eps, *z;        // [S, M, Z] of this chunk
  float* h3;             // [S*M, H]
  float *prior, *bce;    // [S*M]
  float *lse_m, *lse_s, *lw_sum;  // running max / scaled sum / sum of logw per batch row [B]
  float *row_nll, *row_neg_elbo;  // [nbatches * B], written at cursor*B + i after the last chunk
  IwState* ist;
  const HParams* hp;
};

}  // namespace mdt

extern "C" {
int mdt_iw_check(const mdt::IwArgs* a);
int mdt_iw_chunk(const mdt::IwArgs* a, hipStream_t s);  // sample, decoder + BCE, reduce
int mdt_iw_reduce(const mdt::IwArgs* a, hipStream_t s); // reduce only (uses M, B, K, S, first, last, prior .. ist)
// conv-VAE pass (conv_iw.hip)
int mdt_iw_reparam(const float* mulv, int M, int B, int Z, int k0, int S, const void* ist, const void* hp, void* z16,
                   float* z32, float* eps, float* prior, hipStream_t s);
int mdt_iw_row_bce(const float* logits, const float* xb, int V, int M, int P, float* bce, hipStream_t s);
}
