// Host side of the device-resident lr / KL-weight schedule (kernels/vae_mlp.h):
// the schedule fields of HParams and the effective values stored in a
// TrainState, shared by TrialStateBuf (conv) and MlpVaeEngine (MLP).
#pragma once
#include <torch/extension.h>

#include <cstddef>
#include <cstring>
#include <memory>

#include "../kernels/vae_mlp.h"

namespace mdt {

// Validates and stores the schedule (all zero = off).
inline void sched_fill(HParams& h, double kl_beta, int64_t lr_warmup, int64_t lr_decay, int64_t lr_decay_steps,
                       double lr_min_ratio, int64_t kl_anneal) {
  constexpr int64_t kMax = 2147483647;
  TORCH_CHECK_VALUE(lr_warmup >= 0 && lr_warmup <= kMax, "lr_warmup_steps must be >= 0, got ", lr_warmup);
  TORCH_CHECK_VALUE(kl_anneal >= 0 && kl_anneal <= kMax, "kl_anneal_steps must be >= 0, got ", kl_anneal);
  TORCH_CHECK_VALUE(lr_decay == kLrDecayNone || lr_decay == kLrDecayCosine, "lr_decay must be 0 (none) or 1 (cosine)");
  TORCH_CHECK_VALUE(lr_decay_steps >= 0 && lr_decay_steps <= kMax, "lr_decay_steps must be >= 0, got ", lr_decay_steps);
  TORCH_CHECK_VALUE(lr_min_ratio >= 0.0 && lr_min_ratio <= 1.0, "lr_min_ratio must be in [0, 1], got ", lr_min_ratio);
  TORCH_CHECK_VALUE(lr_decay != kLrDecayCosine || lr_decay_steps > lr_warmup,
                    "cosine decay needs lr_decay_steps > lr_warmup_steps");
  h.kl_beta_d = kl_beta;
  h.lr_min_ratio = lr_min_ratio;
  h.lr_warmup = (int32_t)lr_warmup;
  h.lr_decay = (int32_t)lr_decay;
  h.lr_decay_steps = (int32_t)lr_decay_steps;
  h.kl_anneal = (int32_t)kl_anneal;
}

// Re-seeds the effective values of `state` for step `step` (what the kernel
// that advances to `step` would have written), and marks eval states as
// schedule-free. Like the beta^t products: a re-stepped or resumed trial is
// right on its very next step, and one that never ran a step reads sane values.
inline void sched_seed(at::Tensor& state, const HParams& h, int64_t step, bool eval) {
  constexpr size_t lo = offsetof(TrainState, lr_t), hi = offsetof(TrainState, loss_hist);
  auto img = std::make_unique<TrainState>();  // zero-initialised host image
  img->sched_off = eval ? 1 : 0;
  sched_store(img.get(), h, step);
  auto cpu = torch::empty({(int64_t)(hi - lo)}, torch::kUInt8);
  std::memcpy(cpu.data_ptr(), reinterpret_cast<const char*>(img.get()) + lo, hi - lo);
  state.narrow(0, lo, hi - lo).copy_(cpu);
}

}  // namespace mdt
