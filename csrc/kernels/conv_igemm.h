// Shared host/device definitions of the conv-VAE implicit-GEMM kernels
// (csrc/kernels/conv_igemm.hip) and their C++ bindings (csrc/runtime/conv_ops.cpp).
// Plain structs only: included by hipcc and g++ alike.
#pragma once
#include <stdint.h>

namespace mdt {

// Convolution geometry, always in "conv view": input (N,H,W,C) NHWC,
// output (N,OH,OW,CO), weight [CO][KH][KW][C]. A transposed conv is the
// conv whose backward-data is its forward (input = convT output).
struct ConvDesc {
  int N, H, W, C;
  int OH, OW, CO;
  int KH, KW, S, P;
};

// Unsigned division by a runtime constant with one mul-hi + add + shift
// (valid for numerators < 2^31): replaces the ~40-instruction integer divide
// in the per-chunk im2col address math.
struct FastDiv {
  uint32_t d, mul, shr;
};

inline FastDiv make_fastdiv(uint32_t d) {
  FastDiv f;
  f.d = d;
  f.shr = 0;
  while ((1u << f.shr) < d) ++f.shr;
  const uint64_t one = 1;
  f.mul = (uint32_t)(((one << 32) * ((one << f.shr) - d)) / d + 1);
  return f;
}

// Row-space GEMM kinds of the forward-type kernel.
enum IgemmMode : int {
  kModeConv = 0,   // rows = conv output pixels, k = (ky, kx, ci): conv fwd / convT bwd-data
  kModeTconv = 1,  // rows = conv INPUT pixels of one stride-parity class, k = (ty, tx, co):
                   // conv bwd-data / convT fwd, without the zero-insertion taps
};

// Launch plan of one forward-type GEMM (computed on the host, deterministic
// in the geometry so the trainer can size the partial-sum buffers up front).
struct FwdPlan {
  int cfg;          // forward tile index (conv_tiles.h), or kFwdDirectBase + direct configuration
  int BM, BN;
  int classes;      // 1, or S*S parity classes (kModeTconv)
  int M;            // GEMM rows per class
  int Ncols, K;     // GEMM columns / depth (per class)
  int mtiles, ntiles, ktiles;
  int ksplit, kt_per_split;
  int colsum_rows;  // rows of the per-block column-sum partials (classes * mtiles)
  int thin;         // 1: per-element im2col gather (channel count not a multiple of 8)
  int direct;       // > 0: patch-resident direct kernel configuration + 1 (conv_direct.h)
};

// Weight-gradient GEMM plan: dW[CO][KH*KW*C] = sum_m G[m][co] * im2col(X)[m][k'].
struct WgradPlan {
  int cfg;          // weight-gradient tile index, kWgDirectBase + DwL index, or kWgThinMfma
  int BM, BN;       // co tile x k' tile
  int M, K2;
  int cotiles, ktiles, mtiles;  // m-tiles of 64
  int nsplit, mt_per_split;
  int thin;
};

// Plan numbers (`cfg`) of the kernels that are no tile of the im2col families.
constexpr int kFwdDirectBase = 100;  // + direct configuration (conv_direct.h)
constexpr int kWgDirectBase = 100;   // + direct weight-gradient geometry (conv_dwgrad.h: DwL1, DwL2)
constexpr int kWgThinMfma = 110;     // MFMA single-channel weight gradient (conv_thin_wg.h)

// Gradient finalisation: per arena segment, g = sum over `nsplit` partial rows
// of width `numel` (deterministic order), then either stored to the gradient
// arena or consumed by a fused Adam + bf16 cast (+ parity-ordered transpose).
// Optional A-operand prologue: the producing layer ran split-K without a
// combine pass; A(row, k) = act(bias[c] + sum_s slab[s][off]) is formed while
// staging (c = off % cin) and written once to `out16` (the producer's output,
// needed later by the backward), saving the combine launch in between.
struct APro {
  const float* slab;  // [ks][A elements] partial sums of the producer (null: plain A)
  const float* bias;
  void* out16;        // bf16
  int ks, relu, cin;
  long long stride;   // elements per slab
};

struct GradSeg {
  long long off, numel;
  const float* slab;  // nullptr: the gradient arena already holds g
  int nsplit;
  int co, k, s, ci;   // weight geometry of the transposed copy ([CO][k][k][ci])
  long long toff;     // offset of the transposed copy in w16t, -1 if none
};

struct GradUnit {
  int seg, start, count;
};

// One 64(co) x 64(ci) tile of one tap of a weight segment for the transpose
// into the parity-ordered copy.
struct TrUnit {
  int seg, tap, co0, ci0;
};

// One job of a horizontally fused launch (conv_jobs.hip): an independent
// piece of work (a GEMM, a weight gradient, a column sum, ...) that runs on
// its own range of workgroups of a shared launch. `args` holds the job's
// kernel-argument struct; `kind` names the device body that interprets it.
constexpr int kJobArgBytes = 256;
struct JobBlob {
  int kind;       // 0 = none / not fusable
  int nblk;       // workgroups of this job (256 threads each)
  int aux[6];     // per-kind geometry (e.g. GEMM tiles per plane, k-splits)
  alignas(16) unsigned char args[kJobArgBytes];
};

// Job kind ids (see conv_jobs.hip for the instantiated combinations); the
// encoders below the enum spell the "+ ..." of each family.
enum JobKindBase : int {
  kJobIgemm = 1000,      // + mode*100 + cfg  (bf16, vector gathers)
  kJobWgrad = 2000,      // + cfg              (bf16, vector gathers)
  kJobWgradThin = 2050,  // + 20*f32 + cfg     (per-element gathers)
  kJobThinWgM = 2100,    // + f32               (MFMA single-channel weight gradient, conv_thin_wg.h)
  kJobWgradAdam = 2200,  // + cfg (0, 1)       (kJobWgrad of one m-split with Adam in its epilogue)
  kJobThinConv = 3000,   // + CO + 100*f32
  kJobThinTconv = 4000,  // + CO
  kJobColsum = 5000,
  kJobLoss = 5001,
  kJobCombine = 5002,
  kJobFinalize = 5003,
  kJobWtrans = 5004,
  kJobLossStep = 5005,   // loss reduction + step advance (fused 28x28 step)
  kJobComm = 5006,       // fused xGMI all-reduce + Adam over finalize units (comm_jobs.h)
  kJobDconv = 6000,      // + direct cfg       (patch-resident direct conv, conv_direct.h)
};

// The kinds of each family, encoded in one place: the builders, the J* wrappers
// of conv_jobs.hip and the multi-job dispatch all go through these.
constexpr int job_igemm(int mode, int cfg) { return kJobIgemm + mode * 100 + cfg; }
constexpr int job_wgrad(int cfg) { return kJobWgrad + cfg; }
constexpr int job_wgrad_thin(bool f32, int cfg) { return kJobWgradThin + (f32 ? 20 : 0) + cfg; }
constexpr int job_thin_wgm(bool f32) { return kJobThinWgM + (f32 ? 1 : 0); }
constexpr int job_wgrad_adam(int cfg) { return kJobWgradAdam + cfg; }
constexpr int job_thin_conv(int co, bool f32) { return kJobThinConv + co + (f32 ? 100 : 0); }
constexpr int job_dconv(int dc) { return kJobDconv + dc; }

// Up to kMaxMultiJobs jobs of any kind of the multi-job kernel (jobs_multi_k).
constexpr int kMaxMultiJobs = 8;

}  // namespace mdt
