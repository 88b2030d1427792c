// Weight averaging (docs/KERNELS.md, "Weight averaging"): one streaming launch
// over the parameter arena after a step's optimizer tail, and the in-place
// exchange of two arenas that evaluation under the averaged weights uses.
//
// ema_update_k reads p, reads and writes e: 12 bytes per element, float4 per
// lane with a scalar tail, so any n >= 1 is served. The launch follows the
// step's optimizer tail on the same stream: the step counter it reads has been
// advanced by an earlier launch and plain loads see it.
#include "ema.h"
#include "common.h"

namespace mdt {

__global__ __launch_bounds__(kEmaThreads) void ema_update_k(const EmaArgs a, const int vec) {
  // 1 - d_t: one thread, in double, broadcast through LDS (as adam_consts_block forms Adam's constants)
  __shared__ float sh_omd;
  if (threadIdx.x == 0)
    sh_omd = a.st ? ema_omd(a.hp->ema_decay, (long long)a.st->step) : ema_omd(a.decay, a.t);
  __syncthreads();
  const float omd = sh_omd;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n4 = vec ? a.n >> 2 : 0;
  const float4* p4 = reinterpret_cast<const float4*>(a.p);
  float4* e4 = reinterpret_cast<float4*>(a.e);
  for (long long i = gid; i < n4; i += stride) {
    const float4 p = p4[i];
    float4 e = e4[i];
    e.x = fmaf(omd, p.x - e.x, e.x);
    e.y = fmaf(omd, p.y - e.y, e.y);
    e.z = fmaf(omd, p.z - e.z, e.z);
    e.w = fmaf(omd, p.w - e.w, e.w);
    e4[i] = e;
  }
  for (long long i = (n4 << 2) + gid; i < a.n; i += stride) {
    const float e = a.e[i];
    a.e[i] = fmaf(omd, a.p[i] - e, e);
  }
}

__global__ __launch_bounds__(kEmaThreads) void arena_swap_k(float* __restrict__ a, float* __restrict__ b,
                                                            const long long n, const int vec) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n4 = vec ? n >> 2 : 0;
  float4* a4 = reinterpret_cast<float4*>(a);
  float4* b4 = reinterpret_cast<float4*>(b);
  for (long long i = gid; i < n4; i += stride) {
    const float4 x = a4[i], y = b4[i];
    a4[i] = y;
    b4[i] = x;
  }
  for (long long i = (n4 << 2) + gid; i < n; i += stride) {
    const float x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

namespace {
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// one float4 per lane up to kEmaMaxBlocks blocks, then the grid-stride loop; the scalar form
// (a buffer off the 16-byte grid) gets one float per lane
inline int ema_grid(long long n, bool vec) {
  const long long work = vec ? (n + 3) / 4 : n;
  const long long g = (work + kEmaThreads - 1) / kEmaThreads;
  return (int)(g < 1 ? 1 : g > kEmaMaxBlocks ? kEmaMaxBlocks : g);
}
}  // namespace

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_ema_update(const EmaArgs* a, hipStream_t s) {
  if (a->n < 1) return 1;
  if (!a->e || !a->p || (a->st && !a->hp)) return 2;
  if (!a->st && !(a->decay >= 0.0 && a->decay < 1.0 && a->t >= 1)) return 3;
  const bool vec = aligned16(a->e) && aligned16(a->p);
  hipLaunchKernelGGL(ema_update_k, dim3(ema_grid(a->n, vec)), dim3(kEmaThreads), 0, s, *a, vec ? 1 : 0);
  return hipGetLastError() == hipSuccess ? 0 : 4;
}

extern "C" int mdt_arena_swap(float* a, float* b, long long n, hipStream_t s) {
  if (n < 1) return 1;
  if (!a || !b) return 2;
  if (a < b + n && b < a + n) return 5;
  const bool vec = aligned16(a) && aligned16(b);
  hipLaunchKernelGGL(arena_swap_k, dim3(ema_grid(n, vec)), dim3(kEmaThreads), 0, s, a, b, n, vec ? 1 : 0);
  return hipGetLastError() == hipSuccess ? 0 : 4;
}
