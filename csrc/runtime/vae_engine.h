// Native owner of one MLP-VAE trial's device memory and kernel sequence.
//
// Memory is laid out for HBM residency and contiguous collectives:
//   params / grads / exp_avg / exp_avg_sq : one flat fp32 arena each, same
//     layout, every tensor 256-byte aligned. fc4 (the first gradients to
//     become final in backward) is placed LAST so gradient bucket 0 is the
//     arena tail and bucket 1 the head: both are contiguous views, the
//     all-reduce needs no pack/unpack copies.
//   acts : one arena for every saved activation / gradient-of-activation.
//   state : the trial's train / eval TrainState and HParams (trial_state.h),
//     device structs read by the kernels.
#pragma once
#include <torch/extension.h>

#include <string>
#include <tuple>
#include <vector>

#include "../kernels/vae_mlp.h"
#include "trial_state.h"

namespace mdt {

struct LayoutEntry {
  std::string name;
  int64_t offset;
  std::vector<int64_t> shape;
};

// Device state of an importance-weighted pass (kernels/vae_iw.h: IwState),
// shared by both trainers: allocate, zero for a pass of `nbatches`, read back
// {nll, neg_elbo, step (batches begun), cursor}.
at::Tensor iw_state_new(int64_t device_index);
void iw_state_begin(at::Tensor state, int64_t nbatches);
std::vector<double> iw_state_read(const at::Tensor& state);

// Device state of a latent report pass (kernels/vae_latent.h: LatentState),
// shared by both trainers like the iw state (csrc/runtime/latent_ops.cpp):
// read back {kl, mi, tc, dwkl, sampled_kl, step (batches begun), cursor}.
at::Tensor latent_state_new(int64_t device_index);
void latent_state_begin(at::Tensor state, int64_t nbatches);
std::vector<double> latent_state_read(const at::Tensor& state);
// Batch rows mulv[:M] -> pass rows cursor*B + i of `rows` [*, 2Z]; advances the pass cursor.
void latent_collect(const at::Tensor& mulv, int64_t M, int64_t B, int64_t Z, at::Tensor rows, at::Tensor state);

class MlpVaeEngine {
 public:
  MlpVaeEngine(int64_t batch, int64_t D, int64_t H, int64_t Z, int64_t device_index);

  std::vector<std::tuple<std::string, int64_t, std::vector<int64_t>>> layout() const;
  int64_t numel() const { return total_; }
  int64_t bucket_split() const { return split_; }  // arena offset where fc4 starts

  void forward(const at::Tensor& X, const at::Tensor& idx, int64_t M, bool train, bool eval,
               int64_t rng_stream, bool want_recon);
  void backward(const at::Tensor& X, const at::Tensor& idx, int64_t M, int64_t part, bool fuse_adam);
  void adam();
  void loss_finalize(bool eval);
  at::Tensor decode(const at::Tensor& z);  // sigmoid(fc4(relu(fc3 z))) -> [M, D]
  at::Tensor act(const std::string& name, int64_t M);
  void set_stamps(at::Tensor t) { stamps_ = t; }  // int64 [6*512*8*8] or undefined
  // float32 [B, 2Z] that the backward's B2 adds to d[mu|lv] (the total-correlation penalty's share,
  // csrc/kernels/vae_tc.hip), or None: B2 as without it
  void set_dmulv_add(c10::optional<at::Tensor> t);

  // Importance-weighted log-likelihood pass (csrc/kernels/vae_iw.hip). It runs
  // on a device state of its own (iw_state); train_state / eval_state, their
  // loss rings and the optimizer arenas are not touched.
  void iw_begin(int64_t nbatches);  // zero the pass state: cursor 0, step 0, totals 0
  // One batch of M rows at the pass cursor: encoder once, then the K samples
  // in chunks of `chunk`; per-row results into row_nll / row_neg_elbo at
  // cursor*B + i, totals into iw_state. Launches only (graph-capturable once
  // the workspaces exist: run it once eagerly first).
  void iw_batch(const at::Tensor& X, const at::Tensor& idx, int64_t M, int64_t K, int64_t chunk,
                at::Tensor row_nll, at::Tensor row_neg_elbo);
  std::vector<double> iw_read();    // nll, neg_elbo, step (batches begun), cursor
  at::Tensor iw_act(const std::string& name, int64_t S, int64_t M);  // of the last chunk: "eps" | "z" [S, M, Z], "prior" | "bce" [S, M], "h3" [S*M, H]
  // virtual rows the chunk workspace holds; it grows (reallocates) when a pass
  // asks for more, which invalidates graphs captured over the old one
  int64_t iw_capacity() const { return iw_cap_; }
  at::Tensor iw_state;

  // Latent report pass (csrc/kernels/vae_latent.hip), on a third state of its
  // own (latent_state): train_state / eval_state / iw_state are not touched.
  void latent_begin(int64_t nbatches);  // zero the pass state
  // One batch of M rows at the pass cursor: the encoder (F1), the slab sum to
  // mulv in the importance-weighted pass's order, then the rows into
  // `rows` [nbatches*B, 2Z] at cursor*B + i. Launches only (graph-capturable).
  void latent_batch(const at::Tensor& X, const at::Tensor& idx, int64_t M, at::Tensor rows);
  std::vector<double> latent_read();    // kl, mi, tc, dwkl, sampled_kl, step (batches begun), cursor
  at::Tensor latent_state;

  at::Tensor params, grads, exp_avg, exp_avg_sq, acts, partials;
  TrialStateBuf state;  // train / eval TrainState and the HParams image (trial_state.h)

 private:
  void fill_args(void* args, const at::Tensor& X, const at::Tensor& idx, int64_t M, bool train,
                 bool eval, int64_t rng_stream, bool want_recon);
  int64_t B_, D_, H_, Z_, total_, split_;
  int last_f2_blocks_ = 0, last_f3_blocks_ = 0;
  std::vector<LayoutEntry> layout_;
  at::Tensor stamps_, dmulv_add_;
  at::Tensor iw_ws_, iw_rowbuf_;  // chunk workspace (h3 | eps | z | prior | bce) and [3][B] running row state
  int64_t iw_cap_ = 0, iw_nbatches_ = 0, latent_nbatches_ = 0;
  std::vector<std::pair<std::string, int64_t>> act_off_;
};

}  // namespace mdt
