// Bernoulli resampling of data-set rows (see binarize.hip):
//   out[i, p] = b(X[idx[i], p]),  i < n, p < D,  out a compact [n, D] float32 buffer of {0, 1}.
//
// Modes: kBinThreshold  b(x) = x >= 0.5 (no RNG);
//        kBinBernoulli  b(x) = u < x with u one Philox4x32-10 word per pixel
//                       (static = epoch key 0 for the whole trial, dynamic = the epoch number).
//
// Philox counter = (q, row, epoch, kBinTag | split), key = the trial's seed:
//   q = p / 4 (the four output words serve pixels 4q .. 4q+3), row = idx[i] (the
//   global data-set row, never i: a row's draw does not depend on the shard, the
//   group size or the rank), split = 0 train / 1 test.
//   u = float(word >> 8) * 2^-24: exact in fp32, in [0, 1), so x = 0 never
//   fires and x = 1 always does.
//
// kBinTag = 0xB1A50000: the reparameterisation noise of every pass draws from
// counter (e, stream, step_lo, step_hi) under the same key, and step_hi = 0
// for any run shorter than 2^32 steps. A fourth counter word with non-zero
// high bits therefore meets none of those draws, whatever the stream words
// (rng_stream, EVAL_STREAM, the IW and latent streams) are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdt {

constexpr uint32_t kBinTag = 0xB1A50000u;
constexpr int kBinThreads = 256;
constexpr int kBinMaxBlocks = 2048;   // 256 CUs x 8 blocks; the rest is a grid-stride loop

enum BinMode : int { kBinThreshold = 0, kBinBernoulli = 1 };

struct BinarizeArgs {
  const float* X;      // [N, D] row-major
  const int32_t* idx;  // [n] rows of X
  float* out;          // [n, D]
  long long n, D, N;
  uint32_t seed_lo, seed_hi, epoch, split;
  int mode;            // BinMode
};

}  // namespace mdt

extern "C" {
// 0, or why the shape is outside the domain: 1 bad mode / split, 2 n < 0 or D < 1 or N < 1,
// 3 ceil(D/4) beyond the 2^32 range of the pixel-group counter word, 4 N beyond the 2^31 range of
// the int32 row index (the row counter word holds 2^32), 5 n*D beyond 2^62 elements
int mdt_binarize_check(long long n, long long D, long long N, int mode, int split);
int mdt_binarize_rows(const mdt::BinarizeArgs* a, hipStream_t s);
}
