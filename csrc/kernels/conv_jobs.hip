// Horizontally fused conv-VAE launches ("job kernels") for MI355X (gfx950).
//
// Why: at the conv-VAE's batch sizes most launches of a training step are
// latency-bound -- a 28x28 step was 29 launches of which a dozen do < 2 us
// of work, and a kernel boundary in a replayed hipGraph costs ~1.5 us plus
// the fill/drain of the grid. Independent pieces of work of the same step
// (the weight gradient and the backward-data GEMM of one layer, a bias column
// sum, the loss reduction) therefore share ONE launch: each job owns a
// contiguous range of workgroups and runs the same device body as its
// stand-alone kernel (conv_igemm_dev.h, conv_thin.h, conv_small.h), so results
// are bitwise identical to the unfused sequence. Two streams with graph
// branches were measured slower on this stack (cross-stream graph edges,
// models/conv_vae.py::_backward_overlap), which is why the fusion is done
// inside a launch instead.
//
// A launch of jobs (kinds k0 < k1 < k2 after sorting) needs an instantiated
// jobs_k<J0, J1, J2>; the table below lists the combinations the 28x28 and
// 128x128 models' backward sweeps use. Any other combination reports "not
// fused" and the caller launches the jobs' stand-alone kernels instead.
#include <string.h>

#include <algorithm>

#include "conv_direct.h"
#include "conv_dwgrad.h"
#include "conv_igemm_dev.h"
#include "comm_jobs.h"
#include "conv_small.h"
#include "conv_thin.h"
#include "conv_thin_wg.h"
#include "conv_launch.h"
#include "conv_tiles.h"

namespace mdt {
using namespace tiles;

struct JobPack {
  JobBlob j[3];
  int start1, start2;  // first workgroup of job 1 / job 2
};

template <class T>
__device__ __forceinline__ const T& job_args(const JobBlob& j) {
  return *reinterpret_cast<const T*>(j.args);
}

struct JNone {
  static constexpr int ID = 0, LDS = 0;
  static __device__ __forceinline__ void run(const JobBlob&, uint8_t*, int) {}
};

// forward-type GEMM (bf16, vector gathers); aux = {tiles per plane, k-splits}
template <int MODE, int CFG, class TC>
struct JIg {
  static constexpr int ID = job_igemm(MODE, CFG), LDS = igemm_lds_bytes<TC>();
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    const int ntb = j.aux[0], ks = j.aux[1];
    const int r = b / ntb, t = b - r * ntb;
    const int cls = r / ks, kz = r - cls * ks;
    igemm_body<MODE, __bf16, true, TC>(job_args<IgArgs>(j), lds, t, ntb, kz, cls);
  }
};

template <int CFG, class TC>
struct JWg {
  static constexpr int ID = job_wgrad(CFG), LDS = wgrad_lds_bytes<TC>();
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    wgrad_body<__bf16, true, TC>(job_args<WgArgs>(j), lds, b, j.nblk);
  }
};

template <typename XT, int CFG, class TC>
struct JWgThin {
  static constexpr int ID = job_wgrad_thin(sizeof(XT) == 4, CFG), LDS = wgrad_lds_bytes<TC>();
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    wgrad_body<XT, false, TC>(job_args<WgArgs>(j), lds, b, j.nblk);
  }
};

template <typename XT>
struct JThinWg {
  static constexpr int ID = job_thin_wgm(sizeof(XT) == 4), LDS = thin_wgrad_mfma_lds_bytes();
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    thin_wgrad_mfma_body<XT>(job_args<WgArgs>(j), lds, b);
  }
};

template <int CO, typename TIN>
struct JThinConv {
  static constexpr int ID = job_thin_conv(CO, sizeof(TIN) == 4), LDS = thin_conv_lds_bytes<CO, 4>();
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    thin_conv_body<CO, 4, TIN>(job_args<ThinConvArgs>(j), lds, b);
  }
};

// patch-resident direct conv (the backward-data of the 64x64 / 32x32 layers):
// shares a launch with the layer's weight gradient
template <int CFG, class CF>
struct JDc {
  static constexpr int ID = job_dconv(CFG), LDS = CF::LDS;
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    dconv_body<CF>(job_args<DcArgs>(j), lds, xcd_remap(b, j.nblk));
  }
};

struct JColsum {
  static constexpr int ID = kJobColsum, LDS = 0;
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t*, int b) { colsum_body(job_args<ColsumArgs>(j), b); }
};

struct JLoss {
  static constexpr int ID = kJobLoss, LDS = 64;
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int) {
    loss_finalize_body(job_args<LossArgs>(j), reinterpret_cast<float*>(lds));
  }
};

struct JFinalize {
  static constexpr int ID = kJobFinalize, LDS = kFinalizeThreads * 4 + 64;
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    grad_finalize_body(job_args<FinalizeArgs>(j), reinterpret_cast<float*>(lds),
                       reinterpret_cast<AdamC*>(lds + kFinalizeThreads * 4), b);
  }
};

struct JWtrans {
  static constexpr int ID = kJobWtrans, LDS = kWtransLds;
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    wtrans_body(job_args<WtransArgs>(j), lds, b);
  }
};

// gradient all-reduce push / reduce+Adam over finalize units (comm_jobs.h)
struct JComm {
  static constexpr int ID = kJobComm, LDS = kCommLds;
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int b) {
    comm_unit_body(job_args<CommJobArgs>(j), lds, b);
  }
};

struct JLossStep {
  static constexpr int ID = kJobLossStep, LDS = 64;
  static __device__ __forceinline__ void run(const JobBlob& j, uint8_t* lds, int) {
    loss_step_body(job_args<LossArgs>(j), reinterpret_cast<float*>(lds));
  }
};

constexpr int cmax(int a, int b) { return a > b ? a : b; }

// ------------------------------------------------------------ multi-job ----
// Up to kMaxMultiJobs (8) independent jobs of any supported kind in ONE launch,
// dispatched per workgroup by a runtime switch (the fused 28x28 step's six
// weight gradients + its loss/step job). Unlike jobs_k it needs no
// instantiation per combination; its register allocation is the maximum over
// the bodies, which is what those bodies use anyway.
struct JobPackN {
  JobBlob j[kMaxMultiJobs];
  int start[kMaxMultiJobs + 1];
  int n;
  unsigned long long* stamps;  // profiling (null = off): per workgroup {start, end} s_memrealtime
};

// the largest weight-gradient tile's LDS (every W tile can run in jobs_multi_k)
constexpr int wgrad_lds_max() {
  int m = 0;
  for (int cfg = 0; cfg < kNumWgTiles; ++cfg)
    visit_wg_tile(cfg, [&m](auto t) { m = cmax(m, wgrad_lds_bytes<typename decltype(t)::type>()); });
  return m;
}
constexpr int kMultiLds = cmax(wgrad_lds_max(), cmax(cmax(JFinalize::LDS, JComm::LDS), JColsum::LDS + 64));

template <int CFG, class TC>
__device__ __forceinline__ bool run_wg_cfg(const JobBlob& j, uint8_t* lds, int b) {
  if (j.kind == job_wgrad(CFG)) {
    wgrad_body<__bf16, true, TC>(job_args<WgArgs>(j), lds, b, j.nblk);
    return true;
  }
  if (j.kind == job_wgrad_thin(false, CFG)) {
    wgrad_body<__bf16, false, TC>(job_args<WgArgs>(j), lds, b, j.nblk);
    return true;
  }
  if (j.kind == job_wgrad_thin(true, CFG)) {
    wgrad_body<float, false, TC>(job_args<WgArgs>(j), lds, b, j.nblk);
    return true;
  }
  return false;
}

// The kinds of jobs_multi_k besides the weight-gradient tiles (run_wg_cfg), as
// X(kind, statement that runs it): the device switch and the host's
// multi_kind_ok both expand this list, so neither can name a kind the other
// lacks. The first two are the single-split Linear weight gradients of the
// fused 28x28 step with Adam in their epilogue (conv_igemm_dev.h WgAdamArgs),
// in the two tile shapes they plan to.
#define MDT_WG_ADAM(TC) \
  wgrad_body<__bf16, true, TC, true>(job_args<WgAdamArgs>(j).w, lds, lb, j.nblk, &job_args<WgAdamArgs>(j))
#define MDT_MULTI_JOBS(X)                  \
  X(job_wgrad_adam(0), MDT_WG_ADAM(W0))    \
  X(job_wgrad_adam(1), MDT_WG_ADAM(W1))    \
  X(kJobLossStep, JLossStep::run(j, lds, lb)) \
  X(kJobLoss, JLoss::run(j, lds, lb))      \
  X(kJobFinalize, JFinalize::run(j, lds, lb)) \
  X(kJobComm, JComm::run(j, lds, lb))      \
  X(kJobColsum, JColsum::run(j, lds, lb))

__device__ __forceinline__ void run_multi_job(const JobBlob& j, uint8_t* lds, int lb) {
  static_assert(kNumWgTiles == 6, "one run_wg_cfg per weight-gradient tile");
  if (run_wg_cfg<0, W0>(j, lds, lb) || run_wg_cfg<1, W1>(j, lds, lb) || run_wg_cfg<2, W2>(j, lds, lb) ||
      run_wg_cfg<3, W3>(j, lds, lb) || run_wg_cfg<4, W4>(j, lds, lb) || run_wg_cfg<5, W5>(j, lds, lb))
    return;
  switch (j.kind) {
#define X(KIND, RUN) case KIND: RUN; break;
    MDT_MULTI_JOBS(X)
#undef X
    default: break;
  }
}

// The job table lives in DEVICE memory (packed once per plan by the host,
// static across graph replays): a runtime index into a kernel-argument struct
// makes the compiler copy the whole pack (2352 B for eight jobs) into per-lane scratch
// (measured 2368 B/lane, the launch ~10x slower), and selecting it with
// constant indices inlines every body eight times (1100+ SGPR spills).
__global__ void __launch_bounds__(256) jobs_multi_k(const JobPackN* __restrict__ p) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kMultiLds];
  const int b = blockIdx.x;
  // every start in ONE batch of scalar loads, then count the jobs this block
  // is past (starts ascend over [0, n)): a while loop over p->start was one
  // dependent load per job in front of the table's later (longest) jobs
  int st[kMaxMultiJobs];
#pragma unroll
  for (int k = 0; k < kMaxMultiJobs; ++k) st[k] = p->start[k];
  const int n = p->n;
  int i = 0, s0 = st[0];
#pragma unroll
  for (int k = 1; k < kMaxMultiJobs; ++k)
    if (k < n && b >= st[k]) {
      i = k;
      s0 = st[k];
    }
  unsigned long long* stamps = p->stamps;
  unsigned long long t0 = 0;
  if (stamps) t0 = __builtin_amdgcn_s_memrealtime();
  run_multi_job(p->j[i], lds, b - s0);
  if (stamps) {  // which job ran where and when: overlap of jobs inside one launch (bench/ddp_structure.py)
    __syncthreads();
    if (threadIdx.x == 0) {
      stamps[2 * b] = t0;
      stamps[2 * b + 1] = __builtin_amdgcn_s_memrealtime();
    }
  }
}

__host__ inline bool multi_kind_ok(int k) {
  for (int cfg = 0; cfg < kNumWgTiles; ++cfg)
    if (k == job_wgrad(cfg) || k == job_wgrad_thin(false, cfg) || k == job_wgrad_thin(true, cfg)) return true;
#define X(KIND, RUN) if (k == KIND) return true;
  MDT_MULTI_JOBS(X)
#undef X
  return false;
}

template <class A, class B, class C>
__global__ void __launch_bounds__(256) jobs_k(JobPack p) {
  // 1 KB aligned: the direct-conv bodies land LDS-DMA pieces at 1 KB offsets
  __shared__ __attribute__((aligned(1024))) uint8_t lds[cmax(cmax(A::LDS, B::LDS), cmax(C::LDS, 16))];
  const int b = blockIdx.x;
  if (b < p.start1) A::run(p.j[0], lds, b);
  else if (b < p.start2) B::run(p.j[1], lds, b - p.start1);
  else C::run(p.j[2], lds, b - p.start2);
}

}  // namespace mdt

using namespace mdt;

namespace {

typedef void (*PackLaunch)(const JobPack&, int, hipStream_t);

template <class A, class B, class C>
void launch_pack(const JobPack& p, int grid, hipStream_t s) {
  hipLaunchKernelGGL((jobs_k<A, B, C>), dim3(grid), dim3(256), 0, s, p);
}

struct Combo {
  int k0, k1, k2;
  PackLaunch fn;
};

#define COMBO3(A, B, C) {A::ID, B::ID, C::ID, &launch_pack<A, B, C>}
#define COMBO2(A, B) {A::ID, B::ID, 0, &launch_pack<A, B, JNone>}

using WgT5 = JWgThin<__bf16, 5, W5>;
using WgT5f = JWgThin<float, 5, W5>;
using ThinC32 = JThinConv<32, __bf16>;
using ThinC32f = JThinConv<32, float>;
using TwB = JThinWg<__bf16>;
using TwF = JThinWg<float>;
using Wg0 = JWg<0, W0>;
using Wg1 = JWg<1, W1>;
using IgC1 = JIg<kModeConv, 1, F1>;
using IgC4 = JIg<kModeConv, 4, F4>;
using IgC5 = JIg<kModeConv, 5, F5>;
using IgC6 = JIg<kModeConv, 6, F6>;
using IgT1 = JIg<kModeTconv, 1, F1>;
using IgT2 = JIg<kModeTconv, 2, F2>;
using IgT4 = JIg<kModeTconv, 4, F4>;
using IgT5 = JIg<kModeTconv, 5, F5>;
using IgT6 = JIg<kModeTconv, 6, F6>;
using DcJS2 = JDc<1, DcS2>;
using DcJT2 = JDc<2, DcT2>;

// kinds sorted ascending within each entry
const Combo kCombos[] = {
    // last layer: thin weight gradient || thin backward-data || loss reduction
    COMBO3(WgT5, ThinC32, JLoss),
    COMBO2(WgT5, ThinC32),
    COMBO3(TwB, ThinC32, JLoss),
    COMBO2(TwB, ThinC32),
    COMBO2(TwF, JFinalize),
    // transposed-conv layers: conv-mode backward-data || weight gradient
    COMBO2(IgC5, Wg0),
    COMBO2(IgC1, Wg0),
    COMBO2(IgC4, Wg0),
    COMBO2(IgC6, Wg0),  // 128x128: narrow column tiles of deep layers (BN split)
    COMBO3(IgC6, Wg0, JColsum),
    // decoder Linear (split-K backward-data) || weight gradient || its bias column sums
    COMBO3(IgT6, Wg1, JColsum),
    COMBO3(IgT5, Wg0, JColsum),
    COMBO3(IgT6, Wg0, JColsum),
    // encoder head || weight gradient || head bias column sums
    COMBO3(IgT4, Wg0, JColsum),
    // conv layers: parity-mode backward-data || weight gradient
    COMBO2(IgT6, Wg0),
    COMBO2(IgT4, Wg0),
    COMBO2(IgT1, Wg0),
    COMBO2(IgT2, Wg0),
    COMBO2(IgT5, Wg0),
    // backward-data || weight gradient || finalize+Adam of the layers whose
    // gradients the previous launches completed (spread optimizer)
    COMBO3(IgC1, Wg0, JFinalize),
    COMBO3(IgC4, Wg0, JFinalize),
    COMBO3(IgC5, Wg0, JFinalize),
    COMBO3(IgC6, Wg0, JFinalize),
    COMBO3(IgT1, Wg0, JFinalize),
    COMBO3(IgT2, Wg0, JFinalize),
    COMBO3(IgT4, Wg0, JFinalize),
    COMBO3(IgT6, Wg0, JFinalize),
    // optimizer tail: first-layer weight gradient || finalize+Adam of every
    // other layer; then first-layer finalize || transposed weight copies
    COMBO2(WgT5f, JFinalize),
    COMBO2(JFinalize, JWtrans),
    // step's first launch (batch gather + step begin + first layer) || the
    // transposed weight copies of the previous step's update (MDT_CONV_DEFER_WT=1)
    COMBO2(ThinC32f, JWtrans),
    // ... or the first decoder GEMM (MDT_CONV_DEFER_WT=2)
    COMBO2(IgC1, JWtrans),
    COMBO2(IgC4, JWtrans),
    COMBO2(IgC5, JWtrans),
    COMBO2(IgC6, JWtrans),
    // 128x128 32x32 <-> 16x16 layers: direct backward-data || im2col weight
    // gradient (the 64x64 <-> 32x32 pair's direct weight gradient runs 8-wave
    // workgroups in its own launch: 15.9 -> 14.2 us, profiles/r3_dconv2)
    COMBO2(Wg0, DcJS2),
    COMBO2(Wg0, DcJT2),
    // intra-group DDP with the fused xGMI all-reduce (comm_jobs.h): a backward
    // launch also pushes the gradients the previous launches completed; the
    // tail reduces + applies Adam (two comm jobs) after the first layer's
    // weight gradient pushed the rest
    COMBO3(IgC1, Wg0, JComm),
    COMBO3(IgC4, Wg0, JComm),
    COMBO3(IgC5, Wg0, JComm),
    COMBO3(IgC6, Wg0, JComm),
    COMBO3(IgT1, Wg0, JComm),
    COMBO3(IgT2, Wg0, JComm),
    COMBO3(IgT4, Wg0, JComm),
    COMBO3(IgT5, Wg0, JComm),
    COMBO3(IgT6, Wg0, JComm),
    COMBO3(Wg0, JComm, DcJS2),
    COMBO3(Wg0, JComm, DcJT2),
    COMBO2(TwF, JComm),
    COMBO2(WgT5f, JComm),
    COMBO2(JComm, JComm),
};

#undef COMBO3
#undef COMBO2

}  // namespace

extern "C" {

// Launch 2-3 jobs as ONE kernel. Returns 0 when launched, 1 when no fused
// kernel exists for this combination of kinds (nothing launched: the caller
// falls back to the stand-alone kernels), 2 on bad input.
int mdt_launch_jobs(const JobBlob* jobs, int n, hipStream_t s) {
  if (n < 2 || n > 3) return 2;
  const JobBlob* v[3] = {&jobs[0], &jobs[1], n > 2 ? &jobs[2] : nullptr};
  for (int i = 0; i < n; ++i)
    if (v[i]->kind <= 0 || v[i]->nblk <= 0) return 1;
  std::sort(v, v + n, [](const JobBlob* a, const JobBlob* b) { return a->kind < b->kind; });
  const int k2 = n > 2 ? v[2]->kind : 0;
  for (const Combo& c : kCombos) {
    if (c.k0 != v[0]->kind || c.k1 != v[1]->kind || c.k2 != k2) continue;
    JobPack p;
    memset(&p, 0, sizeof(p));
    p.j[0] = *v[0];
    p.j[1] = *v[1];
    if (n > 2) p.j[2] = *v[2];
    p.start1 = v[0]->nblk;
    p.start2 = v[0]->nblk + v[1]->nblk;
    const int grid = p.start2 + (n > 2 ? v[2]->nblk : 0);
    c.fn(p, grid, s);
    return (int)hipGetLastError() ? -1 : 0;
  }
  return 1;
}

// Pack 1..kMaxMultiJobs jobs of any supported kinds into a JobPackN image at
// `dst` (host memory, mdt_jobs_multi_bytes() bytes; the caller uploads it once).
// Returns the grid size, 0 for an unsupported kind, -1 for bad input.
int mdt_jobs_multi_bytes() { return (int)sizeof(JobPackN); }

int mdt_pack_jobs_multi_stamps(void* img, void* stamps) {
  reinterpret_cast<JobPackN*>(img)->stamps = reinterpret_cast<unsigned long long*>(stamps);
  return 0;
}

int mdt_pack_jobs_multi(const JobBlob* jobs, int n, void* dst) {
  if (n < 1 || n > kMaxMultiJobs) return -1;
  JobPackN p;
  memset(&p, 0, sizeof(p));
  int grid = 0;
  for (int i = 0; i < n; ++i) {
    if (jobs[i].nblk <= 0) return -1;
    if (!multi_kind_ok(jobs[i].kind)) return 0;
    p.j[i] = jobs[i];
    p.start[i] = grid;
    grid += jobs[i].nblk;
  }
  p.start[n] = grid;
  p.n = n;
  memcpy(dst, &p, sizeof(p));
  return grid;
}

// ONE jobs_multi_k launch over a packed table already in device memory.
int mdt_launch_jobs_multi(const void* dev_pack, int grid, hipStream_t s) {
  if (!dev_pack || grid <= 0) return 2;
  hipLaunchKernelGGL(jobs_multi_k, dim3(grid), dim3(256), 0, s, reinterpret_cast<const JobPackN*>(dev_pack));
  return (int)hipGetLastError() ? -1 : 0;
}

// Launch one job with its stand-alone kernel form (combine / colsum / loss).
int mdt_launch_job1(const JobBlob* j, hipStream_t s) {
  if (j->kind == kJobCombine) return launch_splitk_combine(*reinterpret_cast<const CombineArgs*>(j->args), j->nblk, s);
  return 1;
}

}  // extern "C"
