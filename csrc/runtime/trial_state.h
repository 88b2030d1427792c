// The state buffers of one trial, shared by both trainers: the train / eval
// TrainState and the HParams image the kernels read (kernels/vae_mlp.h), so a
// captured hipGraph replays across batches and hparam changes. The host side
// of the device-resident lr / KL-weight schedule lives here too: the schedule
// fields of HParams and the effective values stored in a TrainState.
#pragma once
#include <torch/extension.h>

#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <vector>

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
  // ... and the total-correlation weight, which lives after the loss ring
  auto tc = torch::empty({(int64_t)sizeof(float)}, torch::kUInt8);
  std::memcpy(tc.data_ptr(), &img->tc_t, sizeof(float));  // 0 without a weight (the image is zero-initialised)
  state.narrow(0, offsetof(TrainState, tc_t), sizeof(float)).copy_(tc);
}

class TrialStateBuf {
 public:
  // device_index < 0: the buffers live on the host (every method only narrows and copies)
  TrialStateBuf(int64_t device_index) {
    auto bopt = torch::TensorOptions().dtype(torch::kUInt8);
    bopt = device_index < 0 ? bopt.device(torch::kCPU) : bopt.device(torch::kCUDA, device_index);
    train_state = torch::zeros({(int64_t)((sizeof(TrainState) + 63) / 64 * 64)}, bopt);
    eval_state = torch::zeros_like(train_state);
    hparams = torch::zeros({(int64_t)((sizeof(HParams) + 63) / 64 * 64)}, bopt);
    set_hparams(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, 0, false);
  }
  void set_hparams(double lr, double b1, double b2, double eps, double wd, double kl_beta, double gs, int64_t seed,
                   bool decoupled, int64_t lr_warmup = 0, int64_t lr_decay = 0, int64_t lr_decay_steps = 0,
                   double lr_min_ratio = 0.0, int64_t kl_anneal = 0, double free_bits = 0.0,
                   double tc_weight = 0.0, double ema_decay = 0.0) {
    TORCH_CHECK_VALUE(std::isfinite(ema_decay) && ema_decay >= 0.0 && ema_decay < 1.0,
                      "ema_decay must be in [0, 1), got ", ema_decay);
    TORCH_CHECK_VALUE(std::isfinite(free_bits) && free_bits >= 0.0, "free_bits must be finite and >= 0, got ", free_bits);
    TORCH_CHECK_VALUE(std::isfinite(tc_weight) && tc_weight >= 0.0, "tc_weight must be finite and >= 0, got ", tc_weight);
    HParams h;
    std::memset(&h, 0, sizeof(h));
    h.lr = (float)lr; h.beta1 = (float)b1; h.beta2 = (float)b2; h.eps = (float)eps; h.weight_decay = (float)wd;
    h.kl_beta = (float)kl_beta; h.grad_scale = (float)gs; h.decoupled_wd = decoupled ? 1 : 0;
    h.seed_lo = (uint32_t)((uint64_t)seed & 0xffffffffu); h.seed_hi = (uint32_t)((uint64_t)seed >> 32);
    h.lr_d = lr; h.beta1_d = b1; h.beta2_d = b2;
    sched_fill(h, kl_beta, lr_warmup, lr_decay, lr_decay_steps, lr_min_ratio, kl_anneal);
    h.free_bits = (float)free_bits;
    h.tc_weight = (float)tc_weight;
    h.ema_decay = ema_decay;
    hp_ = h;
    const bool changed = b1 != b1_ || b2 != b2_;
    b1_ = b1; b2_ = b2;
    auto cpu = torch::empty({(int64_t)sizeof(HParams)}, torch::kUInt8);
    std::memcpy(cpu.data_ptr(), &h, sizeof(h));
    hparams.narrow(0, 0, sizeof(HParams)).copy_(cpu);
    const int64_t tstep = (int64_t)read_state(false)[0], estep = (int64_t)read_state(true)[0];
    if (changed) {  // keep the stored beta^t products consistent with the new betas
      pows(train_state, tstep);
      pows(eval_state, estep);
    }
    // the effective lr / KL weight stored in the states follow the new values
    sched_seed(train_state, hp_, tstep, false);
    sched_seed(eval_state, hp_, estep, true);
  }
  void set_cursor(bool eval, int64_t cursor, int64_t nbatches) {
    int32_t v[2] = {(int32_t)cursor, (int32_t)nbatches};
    auto cpu = torch::empty({8}, torch::kUInt8);
    std::memcpy(cpu.data_ptr(), v, 8);
    (eval ? eval_state : train_state).narrow(0, offsetof(TrainState, cursor), 8).copy_(cpu);
  }
  void set_step(bool eval, int64_t step) {
    auto cpu = torch::empty({8}, torch::kUInt8);
    std::memcpy(cpu.data_ptr(), &step, 8);
    at::Tensor& s = eval ? eval_state : train_state;
    s.narrow(0, offsetof(TrainState, step), 8).copy_(cpu);
    pows(s, step);
    sched_seed(s, hp_, step, eval);
  }
  void reset_loss(bool eval) {
    at::Tensor& s = eval ? eval_state : train_state;
    s.narrow(0, offsetof(TrainState, epoch_loss), 16).zero_();
    s.narrow(0, offsetof(TrainState, epoch_tc), 8).zero_();
  }
  // step, cursor, nbatches, epoch_loss, epoch_count, lr, kl_beta, free_bits
  std::vector<double> read_state(bool eval) {
    auto cpu = (eval ? eval_state : train_state).narrow(0, 0, offsetof(TrainState, loss_hist)).to(torch::kCPU);
    TrainState h;
    std::memcpy(&h, cpu.data_ptr(), offsetof(TrainState, loss_hist));
    // + the effective lr, KL weight and free-bits floor of the last completed step (what its kernels used)
    return {(double)h.step, (double)h.cursor, (double)h.nbatches, h.epoch_loss, h.epoch_count, h.lr_t, (double)h.kl_t,
            (double)h.fb_t};
  }
  // total-correlation penalty: the effective weight of the last completed step and the running sum of tc_batch
  std::vector<double> read_tc(bool eval) {
    constexpr size_t lo = offsetof(TrainState, tc_t), n = sizeof(TrainState) - lo;
    auto cpu = (eval ? eval_state : train_state).narrow(0, lo, n).to(torch::kCPU);
    auto h = std::make_unique<TrainState>();
    std::memcpy(reinterpret_cast<char*>(h.get()) + lo, cpu.data_ptr(), n);
    return {(double)h->tc_t, h->epoch_tc};
  }
  at::Tensor loss_history(bool eval) {  // CPU float tensor [kLossHist]
    return (eval ? eval_state : train_state)
        .narrow(0, offsetof(TrainState, loss_hist), sizeof(float) * kLossHist)
        .to(torch::kCPU)
        .view(torch::kFloat32);
  }
  at::Tensor train_state, eval_state, hparams;

 private:
  void pows(at::Tensor& s, int64_t step) {
    double v[2] = {std::pow(b1_, (double)step), std::pow(b2_, (double)step)};
    auto cpu = torch::empty({16}, torch::kUInt8);
    std::memcpy(cpu.data_ptr(), v, 16);
    s.narrow(0, offsetof(TrainState, b1pow), 16).copy_(cpu);
  }
  double b1_ = -1, b2_ = -1;
  HParams hp_{};  // host copy: set_step re-seeds the schedule's effective values from it
};

}  // namespace mdt
