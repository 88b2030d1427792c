// Latent report of a VAE over the n rows of a pass on MI355X (gfx950): per-
// dimension KL, active units and the aggregate-posterior split of the KL term
// into index-code mutual information, total correlation and dimension-wise KL
// (Hoffman & Johnson; Chen et al., beta-TCVAE; definitions: models/latent.py).
//
// Everything is a function of the encoder rows mulv[n, 2Z] (mu | lv), so the
// pass is model-agnostic. Per batch the trainers' encoders write mulv and
//
//   latent_collect_k  copies the batch's rows to pass rows cursor*B + i and
//                     advances the pass cursor (one workgroup; the encoder's
//                     first kernel advanced the step).
//
// Once per pass, after the last batch:
//
//   latent_prep_k     per (row, d): eps (Philox), z = mu + eps exp(lv/2) and the
//                     packed pair operand (mu, -exp(-lv)/2, -(lv + log 2pi)/2);
//                     per row lq_cond and lp in latent order; per 16 rows double
//                     partials of sum mu, sum mu^2, sum kl_d, sum exp(lv).
//   latent_pair_k     the hot path: n^2 Z evaluations of
//                       t[i,j,d] = log q(z_id | x_j) = (z_id - mu_jd)^2 * (-a_jd/2) - (lv_jd + log 2pi)/2
//                     (the direct form: the expanded one cancels at lv ~ -12)
//                     folded into Z + 1 online log-sum-exps per row i: one per
//                     dimension over j and one of sum_d t over j. No pair is
//                     ever stored.
//   latent_finish_k   merges the j-splits in split order, forms lq_joint and
//                     lq_marg per row and per-workgroup double partials of the
//                     four row means.
//   latent_fold_k     one workgroup: the statistics partials into kl_per_dim /
//                     mu_var / post_var and the row partials into LatentState,
//                     both in a fixed order.
//
// No atomics anywhere and every sum has a fixed order: a pass repeats bitwise,
// and the number of j-splits depends on n alone (lat_splits).
#include "common.h"
#include "vae_latent.h"
#include "vae_mlp_dev.h"

namespace mdt {

// ------------------------------------------------- MLP-VAE: slabs -> mulv ----
// F1 leaves [mu|lv] as split-K slabs. This is iw_sample_k's summation (phase 1
// and the first lines of phase 2 of vae_iw.hip, same expressions in the same
// order), so mulv is bitwise the importance-weighted pass's. One block per 16
// rows.
__global__ void __launch_bounds__(kThreads) latent_mulv_k(VaeArgs a) {
  __shared__ __attribute__((aligned(16))) float part[2][16][64];
  const SlabGeo geo(a.H, a.Z);
  const int ti = blockIdx.x;
  const int i0 = ti * 16;
  const int Z2 = 2 * a.Z;
  {
    const int quads = geo.sw / 4;
    const int pairs = 16 * quads;
    const int t = threadIdx.x;
    if (t < 2 * pairs) {
      const int half = t / pairs, pr = t - half * pairs;
      const int r = pr / quads, cq = pr - r * quads;
      const float4* base = reinterpret_cast<const float4*>(a.slab_mv + ((size_t)(ti * geo.th) * 16 + r) * geo.sw) + cq;
      const size_t sstride = (size_t)16 * geo.sw / 4;
      float4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = base[min(half * 16 + u, geo.th - 1) * sstride];
      __builtin_amdgcn_sched_barrier(0);
      float4 acc4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const float m = half * 16 + u < geo.th ? 1.f : 0.f;
        acc4.x += v[u].x * m; acc4.y += v[u].y * m; acc4.z += v[u].z * m; acc4.w += v[u].w * m;
      }
      *reinterpret_cast<float4*>(&part[half][r][cq * 4]) = acc4;
    }
  }
  __syncthreads();
  const int e = threadIdx.x;
  const int r = e / a.Z, c = e - r * a.Z;
  const int i = i0 + r;
  if (e < 16 * a.Z && i < a.M) {
    const float mu = part[0][r][c] + part[1][r][c] + a.b2[c];
    const float lv = part[0][r][a.Z + c] + part[1][r][a.Z + c] + a.b2[a.Z + c];
    a.mulv[(size_t)i * Z2 + c] = mu;
    a.mulv[(size_t)i * Z2 + a.Z + c] = lv;
  }
}

// The rest of the file forms every product and sum as written: lq_cond (prep)
// and the j = i term of the joint (pair) must be the same float, and n = 1
// gives mi = tc = 0 exactly.
#pragma clang fp contract(off)

constexpr float kLog2Pi = 1.8378770664093453f;

// ------------------------------------------------------------- collect ----
constexpr int kLatColThreads = 256;

__global__ void __launch_bounds__(kLatColThreads) latent_collect_k(const float* mulv, int M, int B, int Z, float* rows,
                                                                   long long rows_cap, LatentState* lst) {
  const int cursor = lst->st.cursor;
  const long long r0 = (long long)cursor * B;
  const int w = 2 * Z;
  if (r0 + M <= rows_cap) {
    float* dst = rows + (size_t)r0 * w;
    for (int e = threadIdx.x; e < M * w; e += kLatColThreads) dst[e] = mulv[e];
  }
  __syncthreads();  // every thread has read the cursor
  if (threadIdx.x == 0) {
    int cur = cursor + 1;
    if (lst->st.nbatches > 0 && cur >= lst->st.nbatches) cur = 0;
    lst->st.cursor = cur;
  }
}

// ---------------------------------------------------------------- prep ----
// Block = kLatPrepRows rows; thread (wave g, lane d) takes dimension d of rows
// g, g + 4, ... of the block. The per-row sums run over d in latent order (one
// thread per row); the statistics are double: per thread over its 4 rows, the
// four waves in wave order.
constexpr int kLatPrepThreads = 256;

__device__ __forceinline__ float lat_t(float z, float mu, float ah, float c) {
  const float q = z - mu;
  return fmaf(q * q, ah, c);
}

__global__ void __launch_bounds__(kLatPrepThreads) latent_prep_k(LatentArgs a) {
  __shared__ float tcn[kLatPrepRows][kLatMaxZ + 1], tpr[kLatPrepRows][kLatMaxZ + 1];
  __shared__ double ds[4][4][kLatMaxZ];
  const int Z = a.Z, zt = lat_zt(Z);
  const int d = threadIdx.x & 63, g = threadIdx.x >> 6;
  const long long r0 = (long long)blockIdx.x * kLatPrepRows;
  double sm = 0.0, sq = 0.0, sk = 0.0, se = 0.0;
  for (int r = g; r < kLatPrepRows; r += 4) {
    const long long i = r0 + r;
    if (i >= a.n) break;
    if (d < Z) {
      const float mu = a.mulv[(size_t)i * 2 * Z + d], lv = a.mulv[(size_t)i * 2 * Z + Z + d];
      const uint32_t ctr = (uint32_t)((unsigned long long)i * (unsigned long long)Z + (unsigned long long)d);
      const u32x4 bits = philox4x32_10(u32x4{ctr, kLatentStream, 0u, 0u}, a.hp->seed_lo, a.hp->seed_hi);
      const float ep = normal_from_bits(bits.x, bits.y);
      const float zz = mu + ep * expf(0.5f * lv);
      const float ah = -0.5f * expf(-lv), c = -0.5f * (lv + kLog2Pi);
      a.eps[(size_t)i * Z + d] = ep;
      a.z[(size_t)i * Z + d] = zz;
      a.pk[(size_t)i * zt + d] = float4{mu, ah, c, 0.f};
      tcn[r][d] = lat_t(zz, mu, ah, c);
      tpr[r][d] = -0.5f * (zz * zz + kLog2Pi);
      const double mud = (double)mu, lvd = (double)lv, ev = exp(lvd);
      sm += mud;
      sq += mud * mud;
      sk += 0.5 * (mud * mud + ev - lvd - 1.0);
      se += ev;
    } else if (d < zt) {
      a.pk[(size_t)i * zt + d] = float4{0.f, 0.f, 0.f, 0.f};  // t = 0: adds nothing to the joint
    }
  }
  if (d < Z) { ds[g][0][d] = sm; ds[g][1][d] = sq; ds[g][2][d] = sk; ds[g][3][d] = se; }
  __syncthreads();
  if (threadIdx.x < kLatPrepRows && r0 + threadIdx.x < a.n) {
    const int r = threadIdx.x;
    float tc = 0.f, tp = 0.f;
    for (int c = 0; c < Z; ++c) { tc += tcn[r][c]; tp += tpr[r][c]; }
    a.lq_cond[r0 + r] = tc;
    a.lp[r0 + r] = tp;
  }
  if (g == 0 && d < Z) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      a.stat[((size_t)blockIdx.x * 4 + q) * Z + d] = ((ds[0][q][d] + ds[1][q][d]) + ds[2][q][d]) + ds[3][q][d];
  }
}

// ---------------------------------------------------------------- pair ----
// Grid (i tiles, j splits); workgroup = one wave, lane = row i. The lane keeps
// its row's z and the Z + 1 accumulator pairs (max, scaled sum) in VGPRs
// (3 ZT + 2 of them: the kernel is built per ZT = ceil4(Z), dimensions past Z
// carry t = 0). The j rows stream through LDS in tiles of kLatJTile packed
// rows (a straight copy of pk); every lane reads the same (j, d) float4: a
// broadcast, conflict-free. One exp per update:
//   d = t - m;  e = exp(-|d|);  d > 0 ? (s = s e + 1, m = t) : (s += e)
// and the first update (m = -inf, s = 0) gives m = t, s = 1.
__device__ __forceinline__ void lse_push(float& m, float& s, float t) {
  const float d = t - m;
  const float e = __expf(-fabsf(d));
  const bool up = d > 0.f;
  s = up ? fmaf(s, e, 1.f) : s + e;
  m = up ? t : m;
}

template <int ZT>
__global__ void __launch_bounds__(kLatRowTile, 2) latent_pair_k(LatentArgs a) {
  __shared__ float4 tile[kLatJTile * ZT];
  const int lane = threadIdx.x;
  const long long n = a.n;
  const int sp = blockIdx.y;
  const long long i = (long long)blockIdx.x * kLatRowTile + lane;
  const long long ic = i < n ? i : n - 1;
  float z[ZT], m[ZT], s[ZT];
#pragma unroll
  for (int d = 0; d < ZT; ++d) {
    z[d] = d < a.Z ? a.z[(size_t)ic * a.Z + d] : 0.f;
    m[d] = -INFINITY;
    s[d] = 0.f;
  }
  float mj = -INFINITY, sj = 0.f;
  const long long jtn = (n + kLatJTile - 1) / kLatJTile;
  const long long jt0 = sp * jtn / a.splits, jt1 = (sp + 1) * jtn / a.splits;
  for (long long jt = jt0; jt < jt1; ++jt) {
    const long long j0 = jt * kLatJTile;
    const int jn = (int)(n - j0 < kLatJTile ? n - j0 : kLatJTile);
    __syncthreads();
    const float4* src = a.pk + (size_t)j0 * ZT;
    for (int e = lane; e < jn * ZT; e += kLatRowTile) tile[e] = src[e];
    __syncthreads();
    for (int jj = 0; jj < jn; ++jj) {
      float tj = 0.f;
#pragma unroll
      for (int d = 0; d < ZT; ++d) {
        const float4 p = tile[jj * ZT + d];
        const float t = lat_t(z[d], p.x, p.y, p.z);
        tj += t;
        lse_push(m[d], s[d], t);
      }
      lse_push(mj, sj, tj);
    }
  }
  if (i < n) {
    const size_t base = (size_t)sp * (ZT + 1);
#pragma unroll
    for (int d = 0; d < ZT; ++d) {
      a.acc_m[(base + d) * n + i] = m[d];
      a.acc_s[(base + d) * n + i] = s[d];
    }
    a.acc_m[(base + ZT) * n + i] = mj;
    a.acc_s[(base + ZT) * n + i] = sj;
  }
}

// -------------------------------------------------------------- finish ----
constexpr int kLatFinThreads = kLatFinRows;  // one row per thread: 157 workgroups at n = 10 000
constexpr int kLatFoldThreads = 256;

// Fixed tree over the workgroup's N doubles; the result is valid in thread 0.
template <int N>
__device__ __forceinline__ double lat_tree(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = N / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// log-sum-exp of accumulator k of row i over the splits (in split order), minus log n
__device__ __forceinline__ float lat_merge(const LatentArgs& a, int zt, int k, long long i, float logn) {
  float M = -INFINITY, S = 0.f;
#pragma unroll 4
  for (int sp = 0; sp < a.splits; ++sp) {  // one read of each pair; the loads do not depend on the running values
    const size_t o = ((size_t)sp * (zt + 1) + k) * a.n + i;
    const float m = a.acc_m[o], s = a.acc_s[o];
    if (m > M) {
      S = S * expf(M - m) + s;
      M = m;
    } else {
      S += s * expf(m - M);
    }
  }
  return M + (logf(S) - logn);  // n equal terms (collapsed dimensions, n = 1): S = n and the result is M exactly
}

__global__ void __launch_bounds__(kLatFinThreads) latent_finish_k(LatentArgs a) {
  __shared__ double sh[kLatFinThreads];
  const int zt = lat_zt(a.Z);
  const long long i = (long long)blockIdx.x * kLatFinThreads + threadIdx.x;
  const float logn = logf((float)a.n);
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < a.n) {
    float marg = 0.f;
    for (int d = 0; d < a.Z; ++d) marg += lat_merge(a, zt, d, i, logn);
    const float joint = lat_merge(a, zt, zt, i, logn);
    a.lq_joint[i] = joint;
    a.lq_marg[i] = marg;
    const double cond = (double)a.lq_cond[i], lp = (double)a.lp[i];
    v[0] = cond - (double)joint;
    v[1] = (double)joint - (double)marg;
    v[2] = (double)marg - lp;
    v[3] = cond - lp;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double t = lat_tree<kLatFinThreads>(v[q], sh);
    if (threadIdx.x == 0) a.part[(size_t)blockIdx.x * 4 + q] = t;
  }
}

// One workgroup. Thread (wave g, lane d) folds the statistics partials of
// dimension d of blocks g, g + 4, ... in block order (one thread's chain of
// dependent loads and adds over all 625 blocks cost 0.12 ms more at n = 10 000),
// the four waves combine in wave order; every thread folds a strided share of
// the row partials, then the fixed tree.
__global__ void __launch_bounds__(kLatFoldThreads) latent_fold_k(LatentArgs a, long long nblk_prep, long long nblk_fin) {
  __shared__ double sh[kLatFoldThreads];
  __shared__ double fs[4][4][kLatMaxZ];
  __shared__ double kld[kLatMaxZ];
  const double inv_n = 1.0 / (double)a.n;
  const int d = threadIdx.x & 63, g = threadIdx.x >> 6;
  if (d < a.Z) {
    double sm = 0.0, sq = 0.0, sk = 0.0, se = 0.0;
#pragma unroll 4
    for (long long b = g; b < nblk_prep; b += 4) {
      const double* p = a.stat + (size_t)b * 4 * a.Z + d;
      sm += p[0]; sq += p[a.Z]; sk += p[2 * a.Z]; se += p[3 * a.Z];
    }
    fs[g][0][d] = sm; fs[g][1][d] = sq; fs[g][2][d] = sk; fs[g][3][d] = se;
  }
  __syncthreads();
  if (g == 0 && d < a.Z) {
    const double sm = ((fs[0][0][d] + fs[1][0][d]) + fs[2][0][d]) + fs[3][0][d];
    const double sq = ((fs[0][1][d] + fs[1][1][d]) + fs[2][1][d]) + fs[3][1][d];
    const double sk = ((fs[0][2][d] + fs[1][2][d]) + fs[2][2][d]) + fs[3][2][d];
    const double se = ((fs[0][3][d] + fs[1][3][d]) + fs[2][3][d]) + fs[3][3][d];
    const double mean = sm * inv_n;
    const double var = sq * inv_n - mean * mean;  // double: exact to ~1e-12 of mean^2
    kld[d] = sk * inv_n;
    a.kl_per_dim[d] = (float)kld[d];
    a.mu_var[d] = (float)(var > 0.0 ? var : 0.0);
    a.post_var[d] = (float)(se * inv_n);
  }
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (long long b = threadIdx.x; b < nblk_fin; b += kLatFoldThreads) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] += a.part[(size_t)b * 4 + q];
  }
  double tot[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) tot[q] = lat_tree<kLatFoldThreads>(v[q], sh);
  if (threadIdx.x == 0) {
    double kl = 0.0;
    for (int c = 0; c < a.Z; ++c) kl += kld[c];
    LatentState* st = a.lst;
    st->kl = kl;
    st->mi = tot[0] * inv_n;
    st->tc = tot[1] * inv_n;
    st->dwkl = tot[2] * inv_n;
    st->sampled_kl = tot[3] * inv_n;
  }
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_latent_check(const LatentArgs* a) {
  if (a->Z < 1 || a->Z > kLatMaxZ) return 1;
  if (a->n < 1) return 2;
  if ((unsigned long long)a->n * (unsigned long long)a->Z > (1ull << 32)) return 3;
  if (a->splits < 1 || a->splits > kLatMaxSplits || a->splits > lat_cdiv(a->n, kLatJTile)) return 4;
  if (!a->mulv || !a->eps || !a->z || !a->pk || !a->lq_cond || !a->lp || !a->lq_joint || !a->lq_marg || !a->acc_m ||
      !a->acc_s || !a->stat || !a->part || !a->kl_per_dim || !a->mu_var || !a->post_var || !a->lst || !a->hp)
    return 5;
  return 0;
}

template <int ZT>
static void launch_pair(const LatentArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(latent_pair_k<ZT>, dim3((unsigned)lat_cdiv(a->n, kLatRowTile), (unsigned)a->splits),
                     dim3(kLatRowTile), 0, s, *a);
}

static int launch_pair_zt(const LatentArgs* a, hipStream_t s) {
  switch (lat_zt(a->Z)) {
    case 4: launch_pair<4>(a, s); break;
    case 8: launch_pair<8>(a, s); break;
    case 12: launch_pair<12>(a, s); break;
    case 16: launch_pair<16>(a, s); break;
    case 20: launch_pair<20>(a, s); break;
    case 24: launch_pair<24>(a, s); break;
    case 28: launch_pair<28>(a, s); break;
    case 32: launch_pair<32>(a, s); break;
    case 36: launch_pair<36>(a, s); break;
    case 40: launch_pair<40>(a, s); break;
    case 44: launch_pair<44>(a, s); break;
    case 48: launch_pair<48>(a, s); break;
    case 52: launch_pair<52>(a, s); break;
    case 56: launch_pair<56>(a, s); break;
    case 60: launch_pair<60>(a, s); break;
    case 64: launch_pair<64>(a, s); break;
    default: return 1;
  }
  return (int)hipGetLastError();
}

extern "C" int mdt_latent_pair(const LatentArgs* a, hipStream_t s) {
  const int rc = mdt_latent_check(a);
  if (rc) return rc;
  return launch_pair_zt(a, s);
}

// The pair kernel over operands the caller packed itself (vae_tc.hip): the
// same domain, and only the buffers the kernel touches.
extern "C" int mdt_latent_pair_operands(const LatentArgs* a, hipStream_t s) {
  if (a->Z < 1 || a->Z > kLatMaxZ) return 1;
  if (a->n < 1) return 2;
  if ((unsigned long long)a->n * (unsigned long long)a->Z > (1ull << 32)) return 3;
  if (a->splits < 1 || a->splits > kLatMaxSplits || a->splits > lat_cdiv(a->n, kLatJTile)) return 4;
  if (!a->z || !a->pk || !a->acc_m || !a->acc_s) return 5;
  return launch_pair_zt(a, s);
}

extern "C" int mdt_latent_report(const LatentArgs* a, hipStream_t s) {
  int rc = mdt_latent_check(a);
  if (rc) return rc;
  const long long nblk_prep = lat_cdiv(a->n, kLatPrepRows), nblk_fin = lat_cdiv(a->n, kLatFinThreads);
  hipLaunchKernelGGL(latent_prep_k, dim3((unsigned)nblk_prep), dim3(kLatPrepThreads), 0, s, *a);
  rc = mdt_latent_pair(a, s);
  if (rc) return rc;
  hipLaunchKernelGGL(latent_finish_k, dim3((unsigned)nblk_fin), dim3(kLatFinThreads), 0, s, *a);
  hipLaunchKernelGGL(latent_fold_k, dim3(1), dim3(kLatFoldThreads), 0, s, *a, nblk_prep, nblk_fin);
  return (int)hipGetLastError();
}

extern "C" int mdt_latent_collect(const float* mulv, int M, int B, int Z, float* rows, long long rows_cap, void* lst,
                                  hipStream_t s) {
  if (M < 1 || M > B || Z < 1 || Z > kLatMaxZ) return 1;
  if (!mulv || !rows || !lst || rows_cap < M) return 5;
  hipLaunchKernelGGL(latent_collect_k, dim3(1), dim3(kLatColThreads), 0, s, mulv, M, B, Z, rows, rows_cap,
                     reinterpret_cast<LatentState*>(lst));
  return (int)hipGetLastError();
}

extern "C" int mdt_latent_mulv(const VaeArgs* a, hipStream_t s) {
  const int rc = mdt_vae_check(a);
  if (rc) return rc;
  if (!a->slab_mv || !a->mulv || !a->b2) return 5;
  hipLaunchKernelGGL(latent_mulv_k, dim3((a->M + 15) / 16), dim3(kThreads), 0, s, *a);
  return (int)hipGetLastError();
}
