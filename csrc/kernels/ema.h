// Exponential moving average of a trial's parameter arena (see ema.hip and
// docs/KERNELS.md, "Weight averaging"). After optimizer step t (1-based):
//   d_t = min(decay, (1 + t) / (10 + t))   in double
//   e  <-  e + (1 - d_t) * (p - e)         one fmaf per element: e == p is a bitwise fixed point
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vae_mlp.h"

namespace mdt {

constexpr int kEmaThreads = 256;
constexpr int kEmaMaxBlocks = 2048;  // 256 CUs x 8 blocks; the rest is a grid-stride loop

// 1 - d_t as the float every element is multiplied by; the ramp is always on
__host__ __device__ inline float ema_omd(double decay, long long t) {
  const double ramp = (1.0 + (double)t) / (10.0 + (double)t);
  return (float)(1.0 - (decay < ramp ? decay : ramp));
}

struct EmaArgs {
  float* e;              // [n] the average, updated in place
  const float* p;        // [n] the parameters the step's optimizer tail just wrote
  long long n;
  // the step and the decay: from the trial's device state (st->step, hp->ema_decay), or, when st is
  // null, the explicit pair below (kernel-level tests)
  const TrainState* st;
  const HParams* hp;
  double decay;
  long long t;
};

}  // namespace mdt

extern "C" {
// 0, or 1: n < 1, 2: missing buffer, 3: decay outside [0, 1) or t < 1 (explicit pair), 4: launch failed
int mdt_ema_update(const mdt::EmaArgs* a, hipStream_t s);
// a <-> b over n floats in place; same codes (1, 2, 4), 5: the buffers overlap
int mdt_arena_swap(float* a, float* b, long long n, hipStream_t s);
}
