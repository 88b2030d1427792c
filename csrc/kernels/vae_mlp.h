// Host/device-shared structures of the fused MLP-VAE step (see vae_mlp.hip).
#pragma once
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace mdt {

constexpr int kMaxBatch = 4096;
constexpr int kKldPartial = 0;      // F2 waves write [0, 2048)  (8 per block)
constexpr int kBcePartial = 2048;   // F3 waves write [2048, kPartials) (8 per block)
constexpr int kPartials = 2048 + 65536;
constexpr int kLossHist = 4096;     // per-step loss ring (host reads at log points)

// Device-resident training state of one trial (memset to 0 at creation).
//
// Advance protocol (no atomics, no extra launch): within one step
//   F1 block 0 increments `step`   (F1 never reads step),
//   F2 block 0 advances `cursor`   (F2 never reads cursor; F1 already copied
//                                    the batch rows into the xb buffer that
//                                    F3/B3 read).
// So `step` counts steps started: the RNG counter of the running step is
// step-1 and Adam's 1-based t is step.
//
// The thread that advances `step` (step_advance below) also evaluates the
// trial's lr / KL-weight schedule for the new t and records the effective
// values here, so every consumer of the step reads plain numbers and the host
// reads back what the kernels used.
struct TrainState {
  int64_t step;
  int32_t cursor;      // batch index within the epoch's index list
  int32_t nbatches;    // cursor wraps at this value
  double b1pow, b2pow; // beta1^step, beta2^step (Adam bias corrections; F1 advances them)
  double epoch_loss;   // running sum of per-batch losses since the host reset it
  double epoch_count;  // batches accumulated in epoch_loss
  double lr_t;         // effective lr of step `step`: lr_d * f_lr(step) (Adam reads this, not HParams.lr)
  float kl_t;          // effective KL weight of step `step`: (float)(kl_beta_d * f_kl(step))
  float kl_next;       // ... of step `step + 1`: for the fused 28x28 forward/backward, which run
                       // BEFORE their step is advanced (no block of that launch writes it)
  int32_t sched_off;   // 1: factors are 1 whatever the step (eval states: eval uses the full beta)
  float fb_t;          // effective free-bits floor (nats per latent element) of the step: HParams.free_bits,
                       // 0 in eval states (eval reports the true KL, as it uses the full beta)
  float loss_hist[kLossHist];
  // total-correlation penalty (vae_tc.hip), after the ring: every earlier field keeps its offset
  float tc_t;          // effective weight of the step: tc_weight * f_kl(step), 0 in eval states
  int32_t pad_;
  double epoch_tc;     // running sum of tc_batch (unweighted) since the host reset it; epoch_loss and the
                       // loss ring stay BCE + kl_t * KL
};

// Per-trial hyper-parameters, device-resident so a captured graph picks up
// lr/beta changes (schedules, HPO perturbation) without re-capture.
struct HParams {
  float lr, beta1, beta2, eps, weight_decay, kl_beta, grad_scale;
  int32_t decoupled_wd;
  uint32_t seed_lo, seed_hi;
  double lr_d, beta1_d, beta2_d;  // double copies: torch computes lr/bc1 in double
  double kl_beta_d;
  // schedule (all 0 = off: both factors are exactly 1.0 and lr_d * 1.0,
  // (float)kl_beta_d are the unscheduled values bit for bit)
  double lr_min_ratio;            // r: cosine floor as a fraction of lr
  int32_t lr_warmup;              // W: linear warm-up steps
  int32_t lr_decay;               // 0 none, 1 cosine
  int32_t lr_decay_steps;         // T: total steps including warm-up (cosine: T > W)
  int32_t kl_anneal;              // A: KL weight ramps linearly over the first A steps
  // free bits: per-sample, per-dimension KL floor in nats (0 = off, see fb_fwd / fb_bwd in common.h)
  float free_bits;
  // total-correlation penalty: weight of tc_batch in the objective (0 = off), ramped like the KL weight
  float tc_weight;
  // weight averaging (ema.hip): the decay of the parameter average, 0 = off; last, so every earlier
  // field keeps its offset
  double ema_decay;
};

constexpr int kLrDecayNone = 0, kLrDecayCosine = 1;

// Schedule factors of the 1-based optimizer step t, in double; the same
// arithmetic as hpo/schedule.py (the device's cos(pi p) is cospi(p)).
__host__ __device__ inline double sched_lr_factor(const HParams& hp, long long t) {
  if (hp.lr_warmup > 0 && t <= hp.lr_warmup) return (double)t / (double)hp.lr_warmup;
  if (hp.lr_decay == kLrDecayCosine) {
    const double q = (double)(t - hp.lr_warmup) / (double)(hp.lr_decay_steps - hp.lr_warmup);
    const double p = q < 1.0 ? q : 1.0;
#ifdef __HIP_DEVICE_COMPILE__
    const double c = cospi(p);
#else
    const double c = cos(3.14159265358979323846 * p);
#endif
    return hp.lr_min_ratio + (1.0 - hp.lr_min_ratio) * 0.5 * (1.0 + c);
  }
  return 1.0;
}
__host__ __device__ inline double sched_kl_factor(const HParams& hp, long long t) {
  if (hp.kl_anneal <= 0) return 1.0;
  const double q = (double)t / (double)hp.kl_anneal;
  return q < 1.0 ? q : 1.0;
}
// Effective values of step t into a state image (device: the advancing
// thread; host: set_step / set_hparams re-seed them like the beta^t products).
__host__ __device__ inline void sched_store(TrainState* st, const HParams& hp, long long t) {
  const bool on = st->sched_off == 0;
  st->lr_t = hp.lr_d * (on ? sched_lr_factor(hp, t) : 1.0);
  st->kl_t = (float)(hp.kl_beta_d * (on ? sched_kl_factor(hp, t) : 1.0));
  st->kl_next = (float)(hp.kl_beta_d * (on ? sched_kl_factor(hp, t + 1) : 1.0));
  st->fb_t = on ? hp.free_bits : 0.f;  // no schedule: the same for every t
  // the KL anneal's ramp. Without a weight nothing is computed or stored: the word stays the 0 the host
  // seeded (set_hparams re-seeds it through sched_seed), and the default step does no more than before
  if (hp.tc_weight != 0.f) st->tc_t = on ? (float)((double)hp.tc_weight * sched_kl_factor(hp, t)) : 0.f;
}

#ifdef __HIPCC__
// The ONE place a step is advanced (one thread per step, see the protocol
// above): step, the Adam beta^t products and the schedule's effective values.
__device__ __forceinline__ void step_advance(TrainState* st, const HParams* hp) {
  const long long t = st->step + 1;
  st->step = t;
  st->b1pow *= hp->beta1_d;
  st->b2pow *= hp->beta2_d;
  sched_store(st, *hp, t);
}
#endif

struct VaeArgs {
  int M, B, D, H, Z;
  uint32_t rng_stream;   // distinguishes replicas / eval draws
  int train;             // 1: write backward intermediates
  int fuse_adam;         // 1: B3 applies Adam in its epilogues (+ streams the rest)
  const float* X;        // dataset [N, D]
  const int* idx;        // epoch index list [nbatches * B] (+ tail)
  const float *W1, *b1, *W2, *b2, *W3, *b3, *W4, *b4;
  float *gW1, *gb1, *gW2, *gb2, *gW3, *gb3, *gW4, *gb4;
  float *h1, *mulv, *eps, *z, *h3, *dlog, *dh3, *dmulv, *dh1, *xb;
  // split-K partial slabs handed from F1 -> F2 ([mu|lv] over 16-wide h1 slices)
  // and B1 -> B2 (dz over 16-wide dh3 slices): [row tile][H/16][16][width]
  float *slab_mv, *slab_dz;
  float* recon;          // optional sigmoid output [M, D] (eval / images)
  float* partials;       // [kPartials]
  TrainState* st;
  const HParams* hp;
  // optimizer arenas (fused Adam): param / grad / exp_avg / exp_avg_sq base
  float *P, *G, *Mo, *Vo;
  long long oW1, ob1, oW2, ob2;   // arena offsets of the epilogue-updated tensors
  long long s_beg, s_end;         // arena range Adam-streamed by B3 (fc3, fc4)
  unsigned long long* stamps;     // optional phase timestamps (profiling builds of a run)
  // optional [M, 2Z]: added to d[mu|lv] in B2 before they are stored and before the dh1 product (the
  // total-correlation penalty's share, vae_tc.hip); null: B2 is bit for bit the step without it
  const float* dmulv_add;
};

// stamps[((kernel*kStampBlocks + block)*8 + wave)*8 + slot] = s_memrealtime (100 MHz)
constexpr int kStampBlocks = 512;
constexpr int kStampKernels = 6;

struct VaeGrid {
  int f1, f2, f3, b1, b1_dh3, b2, b2_rows, b3, b3_w2, b3_w1, b3_stream;
  int th, ntm, sw, ntz, swz, groups;  // slab geometry (see vae_mlp.hip)
};

VaeGrid vae_grid(const VaeArgs& a);

}  // namespace mdt

extern "C" {
int mdt_vae_check(const mdt::VaeArgs* a);
int mdt_vae_forward(const mdt::VaeArgs* a, hipStream_t s);
int mdt_vae_encode(const mdt::VaeArgs* a, hipStream_t s);  // F1 only
int mdt_vae_backward(const mdt::VaeArgs* a, hipStream_t s, int part);
int mdt_vae_decode(const mdt::VaeArgs* a, const float* zin, hipStream_t s);
// adam.hip: one fused Adam pass over a flat arena of n (a multiple of 4) elements; the eval-path loss reduction
int mdt_adam_step(float* p, const float* g, float* m, float* v, long long n, const mdt::HParams* hp,
                  mdt::TrainState* st, hipStream_t s);
int mdt_loss_finalize(const mdt::HParams* hp, mdt::TrainState* st, const float* partials, int nkld, int nbce,
                      hipStream_t s);
}
