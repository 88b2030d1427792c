// binarize_rows_k: out[i, p] = b(X[idx[i], p]) into a compact [n, D] buffer
// of {0, 1} (binarize.h has the modes and the Philox counter layout).
//
// Memory-bound (4 B read + 4 B written per pixel, ten Philox rounds per 16 B):
// one work item is a group of four pixels = one Philox call = one dwordx4 load
// and store when D % 4 == 0 and both bases are 16-byte aligned (then every row
// start is too); otherwise the same groups go through scalar accesses, word j
// still serving pixel 4q + j, so both paths draw the same bits. 256-thread
// blocks, at most kBinMaxBlocks of them, grid-stride over the n * ceil(D/4) groups.
//
// A row index outside [0, N) is never dereferenced: its pixels come out NaN.
#include "binarize.h"
#include "common.h"

namespace mdt {

__device__ __forceinline__ float bin_draw(uint32_t w, float x) {
  const float u = (float)(w >> 8) * 0x1p-24f;
  return u < x ? 1.f : 0.f;
}

template <bool kVec, bool kRng, typename G>
__device__ __forceinline__ void bin_loop(const BinarizeArgs& a, G Q, G total) {
  const G stride = (G)gridDim.x * kBinThreads;
  for (G g = (G)blockIdx.x * kBinThreads + threadIdx.x; g < total; g += stride) {
    const G i = g / Q;
    const uint32_t q = (uint32_t)(g - i * Q);
    const int32_t row = a.idx[i];
    const bool ok = row >= 0 && (long long)row < a.N;
    const float* src = a.X + (size_t)(ok ? row : 0) * (size_t)a.D + 4 * (size_t)q;
    float* dst = a.out + (size_t)i * (size_t)a.D + 4 * (size_t)q;
    u32x4 r{0u, 0u, 0u, 0u};
    if (kRng) r = philox4x32_10(u32x4{q, (uint32_t)row, a.epoch, kBinTag | a.split}, a.seed_lo, a.seed_hi);
    const float bad = __builtin_nanf("");
    if (kVec) {
      const float4 x = *reinterpret_cast<const float4*>(src);
      float4 o;
      if (kRng) {
        o = make_float4(bin_draw(r.x, x.x), bin_draw(r.y, x.y), bin_draw(r.z, x.z), bin_draw(r.w, x.w));
      } else {
        o = make_float4(x.x >= 0.5f ? 1.f : 0.f, x.y >= 0.5f ? 1.f : 0.f, x.z >= 0.5f ? 1.f : 0.f,
                        x.w >= 0.5f ? 1.f : 0.f);
      }
      if (!ok) o = make_float4(bad, bad, bad, bad);
      *reinterpret_cast<float4*>(dst) = o;
    } else {
      const uint32_t w[4] = {r.x, r.y, r.z, r.w};
      const long long left = a.D - 4 * (long long)q;   // >= 1
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < left) {
          const float x = src[j];
          const float o = kRng ? bin_draw(w[j], x) : (x >= 0.5f ? 1.f : 0.f);
          dst[j] = ok ? o : bad;
        }
      }
    }
  }
}

template <bool kVec, bool kRng>
__global__ __launch_bounds__(kBinThreads) void binarize_rows_k(const BinarizeArgs a) {
  const unsigned long long Q = (unsigned long long)((a.D + 3) / 4), total = (unsigned long long)a.n * Q;
  // 32-bit group arithmetic (a 32-bit division per group instead of a 64-bit one) while
  // g + stride cannot wrap: stride <= kBinMaxBlocks * kBinThreads = 2^19
  if (total <= 0xf0000000ull) {
    bin_loop<kVec, kRng, uint32_t>(a, (uint32_t)Q, (uint32_t)total);
  } else {
    bin_loop<kVec, kRng, unsigned long long>(a, Q, total);
  }
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_binarize_check(long long n, long long D, long long N, int mode, int split) {
  if ((mode != kBinThreshold && mode != kBinBernoulli) || (split != 0 && split != 1)) return 1;
  if (n < 0 || D < 1 || N < 1) return 2;
  if ((D + 3) / 4 > (1ll << 32)) return 3;
  if (N > (1ll << 31)) return 4;
  if ((unsigned long long)n > (1ull << 62) / (unsigned long long)D) return 5;
  return 0;
}

extern "C" int mdt_binarize_rows(const BinarizeArgs* a, hipStream_t s) {
  const int rc = mdt_binarize_check(a->n, a->D, a->N, a->mode, (int)a->split);
  if (rc) return rc;
  if (!a->X || !a->idx || !a->out) return 6;
  if (a->n == 0) return 0;
  const unsigned long long total = (unsigned long long)a->n * (unsigned long long)((a->D + 3) / 4);
  unsigned long long blocks = (total + kBinThreads - 1) / kBinThreads;
  if (blocks > (unsigned long long)kBinMaxBlocks) blocks = kBinMaxBlocks;
  const bool vec = a->D % 4 == 0 && ((uintptr_t)a->X & 15) == 0 && ((uintptr_t)a->out & 15) == 0;
  const bool rng = a->mode == kBinBernoulli;
  const dim3 grid((unsigned)blocks), block(kBinThreads);
  if (vec && rng) hipLaunchKernelGGL((binarize_rows_k<true, true>), grid, block, 0, s, *a);
  else if (vec) hipLaunchKernelGGL((binarize_rows_k<true, false>), grid, block, 0, s, *a);
  else if (rng) hipLaunchKernelGGL((binarize_rows_k<false, true>), grid, block, 0, s, *a);
  else hipLaunchKernelGGL((binarize_rows_k<false, false>), grid, block, 0, s, *a);
  return hipGetLastError() == hipSuccess ? 0 : 7;
}
