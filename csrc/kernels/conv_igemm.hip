// LDS-tiled implicit-GEMM convolution kernels for the conv-VAE on CDNA4
// (gfx950): bf16 operands, v_mfma_f32_16x16x32_bf16, f32 accumulation.
//
// Design (docs/KERNELS.md, "Conv/deconv VAE"):
//  * igemm_fwd_k — forward-type GEMM  Y[rows][cols] = sum_k A(row, k) * Bw[col][k]
//      kModeConv : rows = conv output pixels, k = (ky, kx, ci)   (conv fwd, convT bwd-data)
//      kModeTconv: rows = conv INPUT pixels of one stride-parity class (blockIdx.z),
//                  k = (ty, tx, co) over the taps that actually hit the class
//                  (conv bwd-data, convT fwd). No zero-insertion work: for the
//                  k4/s2 layers each class sees exactly 2x2 of the 16 taps.
//  * wgrad_k     — dW[co][k'] = sum_m G[m][co] * im2col(X)[m][k'] with the m
//                  reduction on the MFMA k axis: both operands are staged m-major
//                  (coalesced 16-B rows) and read with ds_read_b64_tr_b16, the
//                  CDNA4 transposing LDS read. Split over m into f32 partial
//                  slabs reduced deterministically by grad_finalize_k.
//  * grad_finalize_k / wtrans_k (conv_bf16.hip) — partial-slab reduction
//                  (+ fused Adam and bf16 cast), then an LDS-tiled transpose
//                  into the parity-ordered weights the kModeTconv GEMM reads.
// Tiles are 64-deep in k, double-buffered in LDS (register staging: loads for
// tile k+1 are in flight while the MFMAs of tile k run), XOR-swizzled images,
// blockIdx remapped so neighbouring tiles share an XCD's L2.
// Epilogues fuse bias, ReLU, the ReLU-backward mask of the produced gradient
// and the per-block column sums that become the next layer's bias gradient.
#include "conv_igemm_dev.h"
#include "conv_direct.h"
#include "conv_dwgrad.h"
#include "conv_thin_wg.h"
#include "conv_host.h"
#include "conv_launch.h"
#include "conv_tiles.h"

namespace mdt {

__global__ void __launch_bounds__(256) splitk_combine_k(CombineArgs c) {
  __shared__ float red[256];
  splitk_combine_body(c, red, blockIdx.x);
}

__global__ void __launch_bounds__(256) colsum_k(ColsumArgs c) { colsum_body(c, blockIdx.x); }

}  // namespace mdt

// =================================================================== host ====
// The planners these builders call live in conv_plan.hip.
namespace mdt {

int build_igemm(int mode, const void* A, const void* B16, ConvDesc d, const float* bias, int relu, void* y16,
                float* y32, const void* omask, float* colsum, float* ws, IgArgs* pa, FwdPlan* pq, CombineArgs* pc,
                int* nc) {
  FwdPlan q;
  const bool can_split = ws != nullptr && omask == nullptr && colsum == nullptr;
  if (!plan_fwd(mode, d, can_split, &q, false)) return 1;
  IgArgs a{};
  a.d = d;
  a.A = A;
  a.B = reinterpret_cast<const __bf16*>(B16);
  a.relu = relu;
  a.M = q.M; a.Ncols = q.Ncols; a.K = q.K; a.mtiles = q.mtiles; a.ntiles = q.ntiles; a.ktiles = q.ktiles;
  a.kt_per_split = q.kt_per_split;
  if (mode == kModeConv) {
    a.f_pix = make_fastdiv(d.OH * d.OW); a.f_w = make_fastdiv(d.OW);
    a.f_ch = make_fastdiv(d.C); a.f_tw = make_fastdiv(d.KW);
  } else {
    a.f_pix = make_fastdiv((d.H / d.S) * (d.W / d.S)); a.f_w = make_fastdiv(d.W / d.S);
    a.f_ch = make_fastdiv(d.CO); a.f_tw = make_fastdiv(d.KW / d.S);
  }
  *nc = 0;
  if (q.ksplit > 1) {
    a.slab = ws;
    const long long MN = (long long)q.M * q.Ncols;
    int rp = 1;
    while (rp < 64 && rp * 4 < q.ksplit) rp *= 2;
    const int cnt = 256 / rp;
    *pc = CombineArgs{ws, q.ksplit, q.M, q.Ncols, cnt, bias, relu, y32, reinterpret_cast<__bf16*>(y16)};
    *nc = cdiv(MN, cnt);
  } else {
    a.y16 = reinterpret_cast<__bf16*>(y16); a.y32 = y32; a.bias = bias;
    a.omask = reinterpret_cast<const __bf16*>(omask); a.colsum = colsum;
  }
  *pa = a;
  *pq = q;
  return 0;
}

int build_wgrad(const void* G16, const void* X, ConvDesc d, float* out, WgArgs* pa, WgradPlan* pq) {
  WgradPlan q;
  if (!plan_wgrad(d, &q)) return 1;
  WgArgs a{};
  a.d = d;
  a.G = reinterpret_cast<const __bf16*>(G16);
  a.X = X;
  a.out = out;
  a.M = q.M; a.K2 = q.K2; a.cotiles = q.cotiles; a.ktiles = q.ktiles; a.mtiles = q.mtiles;
  a.mt_per_split = q.mt_per_split;
  a.f_pix = make_fastdiv(d.OH * d.OW); a.f_w = make_fastdiv(d.OW);
  a.f_c = make_fastdiv(d.C); a.f_kw = make_fastdiv(d.KW);
  *pa = a;
  *pq = q;
  return 0;
}

template <typename XT>
__global__ void __launch_bounds__(256) thin_wgrad_k(WgArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[thin_wgrad_mfma_lds_bytes()];
  thin_wgrad_mfma_body<XT>(a, lds, blockIdx.x);
}

static unsigned long long* g_dc_stamps = nullptr;

// workgroups of a direct-conv launch over n images
template <class CF>
constexpr int dc_grid(int n) { return n * CF::RB * CF::NBB; }

int launch_splitk_combine(const CombineArgs& c, int nblk, hipStream_t s) {
  hipLaunchKernelGGL(splitk_combine_k, dim3(nblk), dim3(256), 0, s, c);
  return (int)hipGetLastError();
}

}  // namespace mdt

using namespace mdt;

namespace {

template <int MODE, typename AT, bool VEC, bool PRO = false>
int launch_fwd(const IgArgs& a, const FwdPlan& q, hipStream_t s) {
  const dim3 grid(q.mtiles * q.ntiles, q.ksplit, q.classes);
  int rc = 2;
  visit_fwd_tile(q.cfg, [&](auto t) {
    using TC = typename decltype(t)::type;
    // per-element gathers (thin inputs) exist for the 32-column tiles only
    if constexpr (VEC || TC::BN == 32) {
      hipLaunchKernelGGL((igemm_fwd_k<MODE, AT, VEC, TC, PRO>), grid, dim3(256), 0, s, a);
      rc = 0;
    }
  });
  return rc;
}

// VEC: bf16 vector gathers, every tile. Thin inputs (C % 8 != 0, f32 or bf16):
// k' tiles of 16 or 64 only.
template <bool VEC>
int launch_wg(const WgArgs& a, const WgradPlan& q, bool f32, hipStream_t s) {
  const dim3 grid(q.cotiles * q.ktiles * q.nsplit);
  int rc = 2;
  visit_wg_tile(q.cfg, [&](auto t) {
    using TC = typename decltype(t)::type;
    if constexpr (VEC) {
      hipLaunchKernelGGL((wgrad_k<__bf16, true, TC>), grid, dim3(256), 0, s, a);
      rc = 0;
    } else if constexpr (TC::BN != 32) {
      if (f32) hipLaunchKernelGGL((wgrad_k<float, false, TC>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((wgrad_k<__bf16, false, TC>), grid, dim3(256), 0, s, a);
      rc = 0;
    }
  });
  return rc;
}

}  // namespace

extern "C" {

// Forward-type implicit GEMM, launched on `s` or, with `g`, recorded: `g` the
// GEMM, `c` its split-K combine pass (kind kJobCombine, to run after `g`; else
// c->kind = 0). `ws` (f32, >= ksplit*M*Ncols) enables split-K for deep, narrow
// problems (then bias/relu/y16/y32 are applied by the combine pass; omask/colsum
// are not allowed with split-K).
// The two forms differ on these edges, as they always have:
//  * fwd calls and the A prologue have no job form (error 6; the bindings
//    refuse both before they get here);
//  * recorded, g->kind = 0 ("no job form", the caller launches it alone) for
//    f32 or thin operands and for direct configurations 4 and 5, where the
//    launch runs the per-element / direct kernel or reports error 3 / 5;
//  * recorded, the im2col planner is asked first, so a geometry it rejects is
//    error 1 even where the direct kernel would take it.
int mdt_igemm(JobBlob* g, JobBlob* c, int mode, const void* A, int a_is_f32, const void* B16, ConvDesc d,
              const float* bias, int relu, void* y16, float* y32, const void* omask, float* colsum, float* ws,
              int skip_combine, hipStream_t s, const APro* pro, int fwd) {
  const bool has_pro = pro && pro->slab;
  if (g && (fwd || has_pro)) return 6;
  IgArgs a;
  FwdPlan q;
  CombineArgs cb;
  int nc = 0;
  if (g) {
    if (build_igemm(mode, A, B16, d, bias, relu, y16, y32, omask, colsum, ws, &a, &q, &cb, &nc)) return 1;
    memset(g, 0, sizeof(*g));
    memset(c, 0, sizeof(*c));
  }
  const int dc = direct_cfg(mode, d, fwd != 0);
  if (dc >= 0) {  // the planner reported the direct tiling: never fall back silently
    if (g && (a_is_f32 || dc >= kNumDirectJobCfgs)) return 0;
    if (!g && (has_pro || a_is_f32)) return 5;
    DcArgs da{};
    da.A = reinterpret_cast<const __bf16*>(A);
    da.B = reinterpret_cast<const __bf16*>(B16);
    da.y16 = reinterpret_cast<__bf16*>(y16);
    da.y32 = y32;
    da.bias = bias;
    da.omask = reinterpret_cast<const __bf16*>(omask);
    da.colsum = colsum;
    da.stamps = g ? nullptr : g_dc_stamps;
    da.relu = relu;
    da.nimg = d.N;
    const bool known = visit_direct(dc, [&](auto t) {
      using CF = typename decltype(t)::type;
      if (g) {
        g->nblk = dc_grid<CF>(d.N);
      } else {
        hipLaunchKernelGGL((dconv_k<CF>), dim3(dc_grid<CF>(d.N)), dim3(CF::THREADS), 0, s, da);
      }
    });
    if (!known) return 2;
    if (!g) return (int)hipGetLastError();
    g->kind = job_dconv(dc);
    put_args(g, da);
    return 0;
  }
  if (g) {
    g->kind = !a_is_f32 && !q.thin ? job_igemm(mode, q.cfg) : 0;
    g->nblk = q.mtiles * q.ntiles * q.ksplit * q.classes;
    g->aux[0] = q.mtiles * q.ntiles;
    g->aux[1] = q.ksplit;
    put_args(g, a);
    if (nc > 0 && !skip_combine) {
      c->kind = kJobCombine;
      c->nblk = nc;
      put_args(c, cb);
    }
    return 0;
  }
  if (build_igemm(mode, A, B16, d, bias, relu, y16, y32, omask, colsum, ws, &a, &q, &cb, &nc)) return 1;
  int rc;
  if (has_pro) {
    // A from the producer's split-K slabs: conv-mode, bf16 vector gathers only
    if (mode != kModeConv || q.thin || a_is_f32 || pro->cin % 8 || pro->ks < 1) return 4;
    a.pro = *pro;
    rc = launch_fwd<kModeConv, __bf16, true, true>(a, q, s);
  } else if (mode == kModeConv && q.thin) {
    rc = a_is_f32 ? launch_fwd<kModeConv, float, false>(a, q, s) : launch_fwd<kModeConv, __bf16, false>(a, q, s);
  } else if (a_is_f32) {
    rc = 3;
  } else if (mode == kModeConv) {
    rc = launch_fwd<kModeConv, __bf16, true>(a, q, s);
  } else {
    rc = launch_fwd<kModeTconv, __bf16, true>(a, q, s);
  }
  if (rc) return rc;
  if (nc > 0 && !skip_combine) hipLaunchKernelGGL(splitk_combine_k, dim3(nc), dim3(256), 0, s, cb);
  return (int)hipGetLastError();
}

// Weight gradient into `out` ([nsplit] partial slabs), launched on `s` or, with
// `j`, recorded. Edges of the recorded form: the direct weight gradient
// (512-thread workgroups, its own launch) records NO job (kind 0, nblk 0, no
// arguments); an f32 input of a vector-gather layer records kind 0 where the
// launch reports error 3; a thin plan's tile is not checked (the launch: error 2).
int mdt_wgrad(JobBlob* j, const void* G16, const void* X, int x_is_f32, ConvDesc d, float* out, hipStream_t s) {
  WgArgs a;
  WgradPlan q;
  if (build_wgrad(G16, X, d, out, &a, &q)) return 1;
  const bool f32 = x_is_f32 != 0, direct = q.cfg >= kWgDirectBase && q.cfg != kWgThinMfma;
  if (j) {
    memset(j, 0, sizeof(*j));
    if (direct) return 0;
    const int kind = q.cfg == kWgThinMfma ? job_thin_wgm(f32)
                     : q.thin             ? job_wgrad_thin(f32, q.cfg)
                     : f32                ? 0
                                          : job_wgrad(q.cfg);
    return record_job(j, kind, q.cotiles * q.ktiles * q.nsplit, a);
  }
  if (q.cfg == kWgThinMfma) {
    if (f32) hipLaunchKernelGGL(thin_wgrad_k<float>, dim3(q.nsplit), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(thin_wgrad_k<__bf16>, dim3(q.nsplit), dim3(256), 0, s, a);
    return (int)hipGetLastError();
  }
  if (direct) {
    if (f32) return 3;
    const DwArgs da{reinterpret_cast<const __bf16*>(X), reinterpret_cast<const __bf16*>(G16), out, d.N, g_dc_stamps};
    if (q.cfg == kWgDirectBase) hipLaunchKernelGGL(dwgrad_k<DwL1>, dim3(d.N * 4), dim3(DwL1::THREADS), 0, s, da);
    else if (q.cfg == kWgDirectBase + 1) hipLaunchKernelGGL(dwgrad_k<DwL2>, dim3(d.N * 4), dim3(DwL2::THREADS), 0, s, da);
    else return 2;
    return (int)hipGetLastError();
  }
  int rc;
  if (!q.thin) rc = f32 ? 3 : launch_wg<true>(a, q, false, s);
  else rc = launch_wg<false>(a, q, f32, s);
  return rc ? rc : (int)hipGetLastError();
}

// The weight gradient as a job that applies Adam in its epilogue and writes no
// slab (jobs_multi_k only; there is no stand-alone kernel). P / Mo / Vo / w16
// point at the weight's arena segment; `adamc` at the AdamC an earlier launch
// stored (adam_consts_next). Returns 1 when the layer has no such form: more
// than one m-split, a thin or f32 input, a tile shape other than 64x64 / 64x32,
// rows not 16-B aligned.
int mdt_job_wgrad_adam(JobBlob* j, const void* G16, const void* X, int x_is_f32, ConvDesc d, float* P, float* Mo,
                       float* Vo, void* w16, const float* adamc) {
  WgAdamArgs a{};
  WgradPlan q;
  if (!P || !Mo || !Vo || !w16 || !adamc || x_is_f32) return 1;
  if (build_wgrad(G16, X, d, nullptr, &a.w, &q)) return 1;
  if (q.thin || q.cfg < 0 || q.cfg > 1 || q.nsplit != 1 || (q.K2 & 3)) return 1;
  if ((long long)d.CO * q.K2 >= (1ll << 28)) return 1;  // byte offsets in 32 bits
  if (((uintptr_t)P | (uintptr_t)Mo | (uintptr_t)Vo) & 15 || ((uintptr_t)w16 & 7)) return 1;
  a.P = P; a.Mo = Mo; a.Vo = Vo;
  a.w16 = reinterpret_cast<__bf16*>(w16);
  a.c = reinterpret_cast<const AdamC*>(adamc);
  return record_job(j, job_wgrad_adam(q.cfg), q.cotiles * q.ktiles, a);
}

// Profiling: per-workgroup s_memrealtime stamps ([grid][8]) of the direct kernels, or null.
void mdt_dconv_stamps(unsigned long long* p) { g_dc_stamps = p; }

// Per-row-block column sums of G16 [M][N] into `slab`, launched or recorded.
int mdt_colsum(JobBlob* j, const void* G16, int M, int N, int rows_per, float* slab, hipStream_t s) {
  if (N % 8 || rows_per < 1) return 1;
  const int gx = cdiv(N / 8, 256), nblk = gx * cdiv(M, rows_per);
  const ColsumArgs c{reinterpret_cast<const __bf16*>(G16), M, N, rows_per, gx, slab};
  if (j) return record_job(j, kJobColsum, nblk, c);
  hipLaunchKernelGGL(colsum_k, dim3(nblk), dim3(256), 0, s, c);
  return (int)hipGetLastError();
}

}  // extern "C"
