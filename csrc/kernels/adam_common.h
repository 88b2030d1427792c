// torch.optim.Adam arithmetic, shared by the streaming Adam kernel (adam.hip)
// and the weight-gradient epilogues that apply Adam in place (vae_mlp.hip).
#pragma once
#include "common.h"
#include "vae_mlp.h"

namespace mdt {

struct AdamC {
  float step_size, bc2s, b1, b2, eps, wd, gs, lr;
  int decoupled;
  // The weights 1 - beta of the two moment updates. torch passes `1 - beta2` as a
  // double scalar, so its f32 weight is (float)(1 - 0.999) = 0.001f; 1.f - (float)0.999
  // is 1.3e-5 below it (exp_avg_sq off by that factor: outside rtol 1e-5 once
  // g^2 > 77). The MLP-VAE kernels (vae_mlp.hip, adam.hip) ask for torch's value
  // (`torch_omb`); the conv-VAE kernels keep the f32 difference they have always
  // trained with (docs/KERNELS.md, "MLP-VAE shape domain"). The struct stays
  // within the 64 bytes the job kernels reserve for it.
  float omb1, omb2;
};
static_assert(sizeof(AdamC) <= 64, "conv_jobs.hip / comm_jobs.h reserve 64 bytes of LDS for AdamC");

// Compute once per block (thread 0, double precision like torch's Python-side
// scalars) and broadcast through LDS. beta^t comes from the running products
// F1 keeps in TrainState (t = st->step, 1-based), so no pow() on the device.
__device__ __forceinline__ AdamC adam_consts_block(const TrainState* st, const HParams* hp, AdamC* sh,
                                                   bool torch_omb = false) {
  if (threadIdx.x == 0) {
    const double bc1 = 1.0 - st->b1pow;
    const double bc2 = 1.0 - st->b2pow;
    AdamC c;
    const double lr_t = st->lr_t;  // lr_d * f_lr(t), recorded by the thread that advanced the step
    c.step_size = (float)(lr_t / bc1);
    c.bc2s = (float)sqrt(bc2);
    c.b1 = hp->beta1; c.b2 = hp->beta2; c.eps = hp->eps; c.wd = hp->weight_decay;
    c.gs = hp->grad_scale; c.lr = (float)lr_t; c.decoupled = hp->decoupled_wd;
    c.omb1 = torch_omb ? (float)(1.0 - hp->beta1_d) : 1.f - c.b1;
    c.omb2 = torch_omb ? (float)(1.0 - hp->beta2_d) : 1.f - c.b2;
    *sh = c;
  }
  __syncthreads();
  return *sh;
}

// The constants adam_consts_block will give AFTER the next step_advance, from
// the state before it: for a launch that runs ahead of the advancing one and
// hands them to an Adam epilogue inside it (the fused 28x28 step's f28_adamc;
// the conv kernels' 1.f - beta weights). Every line mirrors step_advance +
// sched_store + adam_consts_block above; the products are rounded as those
// store them (no contraction into 1 - beta^t), so the two agree bit for bit
// (tests/gpu/test_f28_epilogue_adam.py).
__device__ __forceinline__ AdamC adam_consts_next(const TrainState* st, const HParams* hp) {
#pragma clang fp contract(off)
  const long long t = st->step + 1;
  const double b1pow = st->b1pow * hp->beta1_d;
  const double b2pow = st->b2pow * hp->beta2_d;
  const bool on = st->sched_off == 0;
  const double lr_t = hp->lr_d * (on ? sched_lr_factor(*hp, t) : 1.0);
  const double bc1 = 1.0 - b1pow;
  const double bc2 = 1.0 - b2pow;
  AdamC c;
  c.step_size = (float)(lr_t / bc1);
  c.bc2s = (float)sqrt(bc2);
  c.b1 = hp->beta1; c.b2 = hp->beta2; c.eps = hp->eps; c.wd = hp->weight_decay;
  c.gs = hp->grad_scale; c.lr = (float)lr_t; c.decoupled = hp->decoupled_wd;
  c.omb1 = 1.f - c.b1; c.omb2 = 1.f - c.b2;
  return c;
}

__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, const AdamC& c) {
  float gr = g * c.gs;
  if (c.wd != 0.f) {
    if (c.decoupled) p *= (1.f - c.lr * c.wd);
    else gr = fmaf(c.wd, p, gr);
  }
  m = fmaf(c.omb1, gr - m, m);             // exp_avg.lerp_(g, 1-b1)
  v = fmaf(c.omb2, gr * gr, v * c.b2);     // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
  const float denom = sqrtf(v) / c.bc2s + c.eps;
  p = p - c.step_size * (m / denom);        // param.addcdiv_(m, denom, -step_size)
}

// Grid-stride streaming Adam over arena range [beg, end) (multiples of 4),
// executed by `nblk` blocks whose local index is `blk`.
__device__ __forceinline__ void adam_stream(float* P, const float* G, float* Mo, float* Vo, long long beg,
                                            long long end, int blk, int nblk, const AdamC& c) {
  const long long n4 = (end - beg) >> 2;
  float4* p4 = reinterpret_cast<float4*>(P + beg);
  const float4* g4 = reinterpret_cast<const float4*>(G + beg);
  float4* m4 = reinterpret_cast<float4*>(Mo + beg);
  float4* v4 = reinterpret_cast<float4*>(Vo + beg);
  for (long long i = (long long)blk * blockDim.x + threadIdx.x; i < n4; i += (long long)nblk * blockDim.x) {
    float4 p = p4[i], g = g4[i], m = m4[i], v = v4[i];
    adam_update(p.x, m.x, v.x, g.x, c);
    adam_update(p.y, m.y, v.y, g.y, c);
    adam_update(p.z, m.z, v.z, g.z, c);
    adam_update(p.w, m.w, v.w, g.w, c);
    p4[i] = p; m4[i] = m; v4[i] = v;
  }
}

}  // namespace mdt
