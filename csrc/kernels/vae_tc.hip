// Total-correlation penalty of a training batch on MI355X (gfx950): value and
// gradient of Chen et al.'s minibatch estimator (beta-TCVAE) over the M rows of
// a step, for both VAE trainers. Everything is a function of the encoder rows
// mulv[M, 2Z] and the step's eps[M, Z] (definitions: models/latent.py with
// n = M, models/tc.py):
//
//   t[i,j,d] = log q(z_id | x_j)      J[i] = lse_j sum_d t      m[i,d] = lse_j t
//   tc_batch = sum_i (J[i] - sum_d m[i,d]) + M (Z - 1) log M
//   w[i,j,d] = exp(sum_d t - J[i]) - exp(t - m[i,d])            q = z_id - mu_jd, a = exp(-lv_jd)
//   g_z[i,d] = sum_j w (-q a)    g_mu[j,d] = sum_i w q a    g_lv[j,d] = sum_i w (q q a - 1) / 2
//
// Forward:
//   tc_pack_k      per (row, d): z = mu + eps exp(lv/2) and the packed pair
//                  operand, as latent_prep_k packs it (the step's eps, no draw).
//   latent_pair_k  unchanged (vae_latent.hip), n = M, with j-splits.
//   tc_merge_k     the splits in split order into m[i,d] and J[i].
// Backward (a flash-attention backward without the matrix products: w is
// recomputed from J and m, no pair is stored):
//   tc_bwd_k       one launch, two roles by blockIdx.z, each chunked over d. Row
//                  pass: lane = row i with its z in VGPRs, the j rows stream
//                  through LDS in tiles as in the pair kernel; g_z of its d-chunk,
//                  and the sums of the exponentials it forms anyway (S, SJ below).
//                  Column pass: lane = row j with its packed row in VGPRs, the i
//                  rows (z, m, J) stream through LDS; g_mu, g_lv of its d-chunk.
//                  Every workgroup forms sum_d t over all d. Both passes split
//                  the streamed side across workgroups.
//   tc_fold_k      partials in split order, the chain rule through z and the
//                  step's weight: tc_t (g_z + g_mu) and tc_t (g_z eps sd / 2 +
//                  g_lv), written to a buffer the MLP-VAE's B2 adds, or added
//                  in place to d[mu|lv] of the conv-VAE (bf16 copy rewritten).
//                  Workgroup 0 also forms tc_batch (with the log-sum-exps taken
//                  again from S and SJ: the pair kernel's fast exp is biased
//                  alike in every term) and adds it to epoch_tc.
//
// No atomics, every sum has a fixed order, no workgroup waits for another: a
// step repeats bitwise. Every index is bounded by M, Z and the split count.
#include <string.h>

#include "common.h"
#include "vae_tc.h"

namespace mdt {

// Every product and sum as written: sum_d t here must be the float the pair
// kernel folded into J (M = 1 gives w = 0, value 0 and gradient 0 exactly).
#pragma clang fp contract(off)

constexpr float kTcLog2Pi = 1.8378770664093453f;

// latent_pair_k's term (vae_latent.hip: lat_t), the same expression
__device__ __forceinline__ float tc_term(float z, float mu, float ah, float c) {
  const float q = z - mu;
  return fmaf(q * q, ah, c);
}

// ---------------------------------------------------------------- pack ----
__global__ void __launch_bounds__(kTcPackThreads) tc_pack_k(TcArgs a) {
  const int Z = a.Z, zt = lat_zt(Z);
  const int e = blockIdx.x * kTcPackThreads + threadIdx.x;
  if (e >= a.M * zt) return;
  const int i = e / zt, d = e - i * zt;
  if (d < Z) {
    const float mu = a.mulv[(size_t)i * 2 * Z + d], lv = a.mulv[(size_t)i * 2 * Z + Z + d];
    const float ep = a.eps[(size_t)i * Z + d];
    const float zz = mu + ep * expf(0.5f * lv);
    a.z[(size_t)i * Z + d] = zz;
    a.pk[e] = float4{mu, -0.5f * expf(-lv), -0.5f * (lv + kTcLog2Pi), 0.f};
  } else {
    a.pk[e] = float4{0.f, 0.f, 0.f, 0.f};  // t = 0: adds nothing to the joint
  }
}

// --------------------------------------------------------------- merge ----
// Thread = (accumulator k, row i), i fastest; latent_finish_k's merge (lat_merge)
// without the log n.
__global__ void __launch_bounds__(kTcPackThreads) tc_merge_k(TcArgs a) {
  const int zt = lat_zt(a.Z);
  const int e = blockIdx.x * kTcPackThreads + threadIdx.x;
  if (e >= a.M * (zt + 1)) return;
  const int k = e / a.M, i = e - k * a.M;
  float Mx = -INFINITY, S = 0.f;
#pragma unroll 4
  for (int sp = 0; sp < a.splits; ++sp) {
    const size_t o = ((size_t)sp * (zt + 1) + k) * a.M + i;
    const float m = a.acc_m[o], s = a.acc_s[o];
    if (m > Mx) {
      S = S * expf(Mx - m) + s;
      Mx = m;
    } else {
      S += s * expf(m - Mx);
    }
  }
  const float r = Mx + logf(S);  // M = 1: S = 1 and the result is the term itself
  if (k < zt) a.lse_d[(size_t)i * zt + k] = r;
  else a.lse_j[i] = r;
}

// ------------------------------------------------------------ backward ----
// Row pass: g_z of rows i (one per lane), dimensions [d0, d0 + DC), over the j
// rows of split sp; every workgroup forms sum_d t over all d (the row's z in
// VGPRs), as the column pass does. It also sums what it exponentiates anyway:
// S[i,d] = sum_j exp(t - m[i,d]) and, in chunk 0, SJ[i] = sum_j exp(sum_d t - J[i]).
// With exact m and J both are 1; m + log S and J + log SJ are the log-sum-exps
// with the pair kernel's fast-exp error taken out (tc_fold_k uses them for the
// value; the gradient's w does not need them).
template <int ZT, int DC>
__device__ __forceinline__ void tc_row_pass(const TcArgs& a, float4* tile, int ch) {
  const int lane = threadIdx.x, M = a.M, sp = blockIdx.y;
  const int i = blockIdx.x * kLatRowTile + lane;
  const int ic = i < M ? i : M - 1;
  const int d0 = ch * DC;
  float z[ZT];
#pragma unroll
  for (int d = 0; d < ZT; ++d) z[d] = d < a.Z ? a.z[(size_t)ic * a.Z + d] : 0.f;
  float cz[DC], cm[DC], g[DC], s[DC];
#pragma unroll
  for (int u = 0; u < DC; ++u) {
    cz[u] = d0 + u < a.Z ? a.z[(size_t)ic * a.Z + d0 + u] : 0.f;
    cm[u] = a.lse_d[(size_t)ic * ZT + d0 + u];
    g[u] = 0.f;
    s[u] = 0.f;
  }
  const float J = a.lse_j[ic];
  float sj = 0.f;
  const int jtn = (M + kLatJTile - 1) / kLatJTile;
  const int jt0 = sp * jtn / a.splits, jt1 = (sp + 1) * jtn / a.splits;
  for (int jt = jt0; jt < jt1; ++jt) {
    const int j0 = jt * kLatJTile;
    const int jn = M - j0 < kLatJTile ? M - j0 : kLatJTile;
    __syncthreads();
    const float4* src = a.pk + (size_t)j0 * ZT;
    for (int e = lane; e < jn * ZT; e += kLatRowTile) tile[e] = src[e];
    __syncthreads();
    for (int jj = 0; jj < jn; ++jj) {
      float tj = 0.f;
#pragma unroll
      for (int d = 0; d < ZT; ++d) {
        const float4 p = tile[jj * ZT + d];
        tj += tc_term(z[d], p.x, p.y, p.z);
      }
      const float pj = expf(tj - J);
      sj += pj;
#pragma unroll
      for (int u = 0; u < DC; ++u) {
        const float4 p = tile[jj * ZT + d0 + u];
        const float q = cz[u] - p.x;
        const float e = expf(fmaf(q * q, p.y, p.z) - cm[u]);
        s[u] += e;
        g[u] += (pj - e) * (q * (2.f * p.y));  // w (-q a) with a = -2 ah
      }
    }
  }
  if (i < M) {
    const size_t o = ((size_t)sp * M + i) * ZT + d0, oc = ((size_t)sp * M + i) * (ZT + 1);
#pragma unroll
    for (int u = 0; u < DC; ++u) {
      a.gz[o + u] = g[u];
      a.csum[oc + d0 + u] = s[u];
    }
    if (ch == 0) a.csum[oc + ZT] = sj;
  }
}

// Column pass: g_mu, g_lv of rows j (one per lane), dimensions [d0, d0 + DC),
// over the i rows of split sp. The LDS tile holds (z, m) per (i, d) and J per i.
template <int ZT, int DC>
__device__ __forceinline__ void tc_col_pass(const TcArgs& a, float4* tile4, int ch) {
  float2* tile = reinterpret_cast<float2*>(tile4);           // [kLatJTile][ZT]
  float* tj_of = reinterpret_cast<float*>(tile + kLatJTile * ZT);  // [kLatJTile]
  const int lane = threadIdx.x, M = a.M, sp = blockIdx.y;
  const int j = blockIdx.x * kLatRowTile + lane;
  const int jc = j < M ? j : M - 1;
  const int d0 = ch * DC;
  float mu[ZT], ah[ZT], cc[ZT];
#pragma unroll
  for (int d = 0; d < ZT; ++d) {
    const float4 p = a.pk[(size_t)jc * ZT + d];
    mu[d] = p.x; ah[d] = p.y; cc[d] = p.z;
  }
  float cmu[DC], cah[DC], ccc[DC], gm[DC], gl[DC];
#pragma unroll
  for (int u = 0; u < DC; ++u) {
    const float4 p = a.pk[(size_t)jc * ZT + d0 + u];
    cmu[u] = p.x; cah[u] = p.y; ccc[u] = p.z;
    gm[u] = 0.f; gl[u] = 0.f;
  }
  const int itn = (M + kLatJTile - 1) / kLatJTile;
  const int it0 = sp * itn / a.splits, it1 = (sp + 1) * itn / a.splits;
  for (int it = it0; it < it1; ++it) {
    const int i0 = it * kLatJTile;
    const int in = M - i0 < kLatJTile ? M - i0 : kLatJTile;
    __syncthreads();
    for (int e = lane; e < in * ZT; e += kLatRowTile) {
      const int r = e / ZT, d = e - r * ZT;
      tile[e] = float2{d < a.Z ? a.z[(size_t)(i0 + r) * a.Z + d] : 0.f, a.lse_d[(size_t)(i0 + r) * ZT + d]};
    }
    if (lane < in) tj_of[lane] = a.lse_j[i0 + lane];
    __syncthreads();
    for (int ii = 0; ii < in; ++ii) {
      float ti = 0.f;
#pragma unroll
      for (int d = 0; d < ZT; ++d) ti += tc_term(tile[ii * ZT + d].x, mu[d], ah[d], cc[d]);
      const float pj = expf(ti - tj_of[ii]);
#pragma unroll
      for (int u = 0; u < DC; ++u) {
        const float2 zm = tile[ii * ZT + d0 + u];
        const float q = zm.x - cmu[u];
        const float w = pj - expf(fmaf(q * q, cah[u], ccc[u]) - zm.y);
        const float qa = q * (-2.f * cah[u]);  // q a
        gm[u] += w * qa;
        gl[u] += w * (0.5f * (q * qa - 1.f));
      }
    }
  }
  if (j < M) {
    const size_t o = ((size_t)sp * M + j) * ZT + d0;
#pragma unroll
    for (int u = 0; u < DC; ++u) {
      a.gmu[o + u] = gm[u];
      a.glv[o + u] = gl[u];
    }
  }
}

// Grid (row tiles, splits, 2 ZT / DC): the row pass's chunks, then the column pass's; workgroup = one wave.
template <int ZT>
__global__ void __launch_bounds__(kLatRowTile) tc_bwd_k(TcArgs a) {
  __shared__ float4 tile[kLatJTile * ZT + kLatJTile / 4];
  constexpr int DC = ZT % 8 == 0 ? 8 : 4;
  constexpr int NCH = ZT / DC;
  if ((int)blockIdx.z < NCH) tc_row_pass<ZT, DC>(a, tile, (int)blockIdx.z);
  else tc_col_pass<ZT, DC>(a, tile, (int)blockIdx.z - NCH);
}

// ---------------------------------------------------------------- fold ----
__global__ void __launch_bounds__(kTcFoldThreads) tc_fold_k(TcArgs a) {
  __shared__ double sh[kTcFoldThreads];
  const int Z = a.Z, zt = lat_zt(Z), M = a.M;
  const int e = blockIdx.x * kTcFoldThreads + threadIdx.x;
  if (e < M * Z) {
    const int i = e / Z, d = e - i * Z;
    float gz = 0.f, gm = 0.f, gl = 0.f;
    for (int sp = 0; sp < a.splits; ++sp) {
      const size_t o = ((size_t)sp * M + i) * zt + d;
      gz += a.gz[o];
      gm += a.gmu[o];
      gl += a.glv[o];
    }
    const float w = *a.tcw;
    const float lv = a.mulv[(size_t)i * 2 * Z + Z + d];
    const float sd = expf(0.5f * lv);
    const float am = w * (gz + gm);
    const float al = w * (gz * a.eps[e] * sd * 0.5f + gl);
    const size_t om = (size_t)i * 2 * Z + d, ol = om + Z;
    if (a.add_out) {
      a.add_out[om] = am;
      a.add_out[ol] = al;
    }
    if (a.dmulv) {
      const float dm = a.dmulv[om] + am, dl = a.dmulv[ol] + al;
      a.dmulv[om] = dm;
      a.dmulv[ol] = dl;
      if (a.dmulv16) {
        __bf16* h = reinterpret_cast<__bf16*>(a.dmulv16);
        h[om] = (__bf16)dm;
        h[ol] = (__bf16)dl;
      }
    }
  }
  if (blockIdx.x != 0) return;
  // tc_batch as latent_finish_k forms the report's tc: per row (J - log M) -
  // sum_d (m - log M) in latent order (the pair kernel's order of sum_d t; the
  // terms are log-densities of size O(1) each, not O(log M), and the constant
  // M (Z - 1) log M never appears), the rows in double over a fixed tree
  const float logm = logf((float)M);
  double v = 0.0;
  // (this one workgroup has few waves to hide memory latency with: both loops load in batches of
  // independent loads and add afterwards, in the same order as one by one)
  for (int i = threadIdx.x; i < M; i += kTcFoldThreads) {
    float marg = 0.f;
    for (int d0 = 0; d0 < Z; d0 += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = d0 + u < Z ? a.lse_d[(size_t)i * zt + d0 + u] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (d0 + u < Z) marg += t[u] - logm;
    }
    v += (double)((a.lse_j[i] - logm) - marg);
  }
  // ... and the row pass's corrections log SJ[i] - sum_d log S[i,d]: the pair kernel's log-sum-exps
  // carry its fast exp's error, about one ulp the same way in every term, which over the M (Z + 1) terms
  // of the value would be M times one rounding. Four (i, k) per thread and turn; the split partials in
  // split order; S - 1 is tiny and exact enough in float for log1pf. M = 1: every S is exactly 1.
  const int nk = M * (Z + 1);
  const size_t sstride = (size_t)M * (zt + 1);
  for (int e0 = threadIdx.x; e0 < nk; e0 += 4 * kTcFoldThreads) {
    size_t o[4];
    double S[4];
    bool joint[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int e = e0 + u * kTcFoldThreads < nk ? e0 + u * kTcFoldThreads : e0;
      const int i = e / (Z + 1), k = e - i * (Z + 1);
      joint[u] = k == Z;
      o[u] = (size_t)i * (zt + 1) + (k < Z ? k : zt);
      S[u] = 0.0;
    }
#pragma unroll 4
    for (int sp = 0; sp < a.splits; ++sp) {
#pragma unroll
      for (int u = 0; u < 4; ++u) S[u] += (double)a.csum[(size_t)sp * sstride + o[u]];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double c = (double)log1pf((float)(S[u] - 1.0));
      if (e0 + u * kTcFoldThreads < nk) v += joint[u] ? c : -c;
    }
  }
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = kTcFoldThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double val = sh[0];
    a.value[0] = val;
    if (a.st) a.st->epoch_tc += val;
  }
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_tc_check(const TcArgs* a) {
  if (a->Z < 1 || a->Z > kLatMaxZ) return 1;
  if (a->M < 1 || a->M > kMaxBatch) return 2;
  if (a->splits < 1 || a->splits > kLatMaxSplits || a->splits > lat_cdiv(a->M, kLatJTile)) return 4;
  if (!a->mulv || !a->eps || !a->z || !a->pk || !a->acc_m || !a->acc_s || !a->lse_d || !a->lse_j || !a->gz ||
      !a->gmu || !a->glv || !a->csum || !a->tcw || !a->value)
    return 5;
  return 0;
}

extern "C" int mdt_tc_forward(const TcArgs* a, hipStream_t s) {
  int rc = mdt_tc_check(a);
  if (rc) return rc;
  const int zt = lat_zt(a->Z);
  hipLaunchKernelGGL(tc_pack_k, dim3((unsigned)lat_cdiv((long long)a->M * zt, kTcPackThreads)), dim3(kTcPackThreads), 0,
                     s, *a);
  LatentArgs l;
  memset(&l, 0, sizeof(l));
  l.n = a->M; l.Z = a->Z; l.splits = a->splits;
  l.z = a->z; l.pk = a->pk; l.acc_m = a->acc_m; l.acc_s = a->acc_s;
  rc = mdt_latent_pair_operands(&l, s);
  if (rc) return rc;
  hipLaunchKernelGGL(tc_merge_k, dim3((unsigned)lat_cdiv((long long)a->M * (zt + 1), kTcPackThreads)),
                     dim3(kTcPackThreads), 0, s, *a);
  return (int)hipGetLastError();
}

template <int ZT>
static void launch_bwd(const TcArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(tc_bwd_k<ZT>, dim3((unsigned)lat_cdiv(a->M, kLatRowTile), (unsigned)a->splits,
                                        (unsigned)(2 * (ZT / tc_chunk(ZT)))),
                     dim3(kLatRowTile), 0, s, *a);
}

extern "C" int mdt_tc_backward(const TcArgs* a, hipStream_t s) {
  const int rc = mdt_tc_check(a);
  if (rc) return rc;
  switch (lat_zt(a->Z)) {
    case 4: launch_bwd<4>(a, s); break;
    case 8: launch_bwd<8>(a, s); break;
    case 12: launch_bwd<12>(a, s); break;
    case 16: launch_bwd<16>(a, s); break;
    case 20: launch_bwd<20>(a, s); break;
    case 24: launch_bwd<24>(a, s); break;
    case 28: launch_bwd<28>(a, s); break;
    case 32: launch_bwd<32>(a, s); break;
    case 36: launch_bwd<36>(a, s); break;
    case 40: launch_bwd<40>(a, s); break;
    case 44: launch_bwd<44>(a, s); break;
    case 48: launch_bwd<48>(a, s); break;
    case 52: launch_bwd<52>(a, s); break;
    case 56: launch_bwd<56>(a, s); break;
    case 60: launch_bwd<60>(a, s); break;
    case 64: launch_bwd<64>(a, s); break;
    default: return 1;
  }
  return (int)hipGetLastError();
}

extern "C" int mdt_tc_fold(const TcArgs* a, hipStream_t s) {
  const int rc = mdt_tc_check(a);
  if (rc) return rc;
  if (!a->add_out && !a->dmulv) return 5;
  hipLaunchKernelGGL(tc_fold_k, dim3((unsigned)lat_cdiv((long long)a->M * a->Z, kTcFoldThreads)), dim3(kTcFoldThreads),
                     0, s, *a);
  return (int)hipGetLastError();
}
