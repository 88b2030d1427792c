// Importance-weighted test log-likelihood of the MLP-VAE on MI355X (gfx950).
//
// For a batch of M rows and K latent draws per row (Burda et al., IWAE):
//   logw[k,i]       = -bce[k,i] + sum_c(-z^2/2 + eps^2/2 + lv/2)     (log p(x,z) - log q(z|x))
//   row_nll[i]      = -(logsumexp_k logw[k,i] - log K)
//   row_neg_elbo[i] = -mean_k logw[k,i]
// The encoder runs once per batch (vae_f1 of vae_mlp.hip, on the pass's own
// state); the K samples are then processed in chunks of S, three launches each:
//
//   iw_sample_k   sum the [mu|lv] slabs, eps (Philox) and z for the S samples,
//                 the prior term per (sample, row), h3 = relu(z W3^T + b3) for
//                 the S*M virtual rows v = s*M + i            (F2's structure)
//   iw_dec_bce_k  logits = h3 W4^T + b4 on exact-f32 MFMA and their BCE against
//                 image row v % M, summed per virtual row. A workgroup owns 32
//                 virtual rows (their h3 tile staged once in LDS) and walks all
//                 D columns, so the row sum finishes in the workgroup and the
//                 logits are never stored. W4 (1.25 MB) streams from L2.
//   iw_reduce_k   online logsumexp (running max + scaled sum) and running sum of
//                 logw per row across chunks; after the last chunk the per-row
//                 results, the batch totals (double, fixed order) and the cursor.
//
// No atomics anywhere: every sum has a fixed order, so a pass is bitwise
// reproducible (eager or graph-replayed).
#include "common.h"
#include "vae_iw.h"
#include "vae_mlp_dev.h"

namespace mdt {

// The clamped logit-form BCE term of EpiBce (vae_mlp.hip).
__device__ __forceinline__ float bce_logit_term(float t, float x) {
  const float sp_pos = fmaxf(t, 0.f) + log1pf(expf(-fabsf(t)));  // -log(1-p)
  const float sp_neg = sp_pos - t;                                 // -log p
  return x * fminf(sp_neg, 100.f) + (1.f - x) * fminf(sp_pos, 100.f);
}

// -------------------------------------------------------------- sample ----
// Block (sample s, row tile ti, group g), 8 waves: vae_f2 with the sample in
// the Philox counter word ((k*B + i)*Z + c, B the trainer's batch size: a tail
// batch draws what a full batch would), the prior term instead of the KLD and
// h3 written at the virtual row. Group 0 stores eps / z / prior (and mu / lv
// from sample 0). Requires Z <= 32, Z % 4 == 0, H <= 512 (mdt_vae_check).
__global__ void __launch_bounds__(kThreads) iw_sample_k(IwArgs a) {
  __shared__ __attribute__((aligned(16))) float part[2][16][64];
  __shared__ __attribute__((aligned(16))) float zt[16][36];
  __shared__ float pt[16][33];
  const SlabGeo geo(a.H, a.Z);
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int tiles_i = cdiv_d(a.M, 16);
  const int s = blockIdx.x / (tiles_i * geo.groups);
  const int rem = blockIdx.x - s * tiles_i * geo.groups;
  const int ti = rem / geo.groups, g = rem - ti * geo.groups;
  const int i0 = ti * 16;
  const int Z2 = 2 * a.Z;
  const int q = lane >> 4;
  const int jt = g * kWaves + w;
  const int j = jt * 16 + (lane & 15);
  float4 w3v[2];
  float w3m[2];
  {
    const float* wr = a.W3 + (size_t)min(j, a.H - 1) * a.Z;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int k0 = c * 16 + 4 * q;
      w3v[c] = *reinterpret_cast<const float4*>(wr + min(k0, a.Z - 4));
      w3m[c] = (j < a.H && k0 < a.Z) ? 1.f : 0.f;
    }
  }
  const float bj = a.b3[min(j, a.H - 1)];
  // phase 1: two half-sums over the slabs, float4 per (row, quad)
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
  // phase 2: one (row, latent) element per thread (16*Z <= 512)
  const long long stp = a.ist->st.step - 1;  // 0-based batch index: F1 of this batch already advanced it
  const uint32_t step_lo = (uint32_t)((unsigned long long)stp & 0xffffffffu);
  const uint32_t step_hi = (uint32_t)((unsigned long long)stp >> 32);
  const int e = threadIdx.x;
  const int r = e / a.Z, c = e - r * a.Z;
  const int i = i0 + r;
  const bool mine = e < 16 * a.Z;
  const bool valid = mine && i < a.M;
  float mu = 0.f, lv = 0.f, ep = 0.f, zz = 0.f;
  if (mine) {
    mu = part[0][r][c] + part[1][r][c] + a.b2[c];
    lv = part[0][r][a.Z + c] + part[1][r][a.Z + c] + a.b2[a.Z + c];
    const float sd = expf(0.5f * lv);
    const uint32_t ctr = ((uint32_t)(a.k0 + s) * (uint32_t)a.B + (uint32_t)i) * (uint32_t)a.Z + (uint32_t)c;
    const u32x4 bits = philox4x32_10(u32x4{ctr, kIwStream, step_lo, step_hi}, a.hp->seed_lo, a.hp->seed_hi);
    ep = normal_from_bits(bits.x, bits.y);
    zz = valid ? mu + ep * sd : 0.f;
    zt[r][c] = zz;
    // log p(z) - log q(z|x) per latent (the 2 pi terms cancel), from the unrounded z
    pt[r][c] = valid ? -0.5f * zz * zz + 0.5f * ep * ep + 0.5f * lv : 0.f;
  }
  __syncthreads();
  {
    const int rr0 = lane & 15;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int k0 = cc * 16 + 4 * q;
      const float4 av = *reinterpret_cast<const float4*>(&zt[rr0][min(k0, 32)]);
      const bool in = k0 < a.Z;  // select, not multiply: unwritten LDS may hold NaN bits
      acc = mfma16x16x4(in ? av.x : 0.f, w3v[cc].x * w3m[cc], acc);
      acc = mfma16x16x4(in ? av.y : 0.f, w3v[cc].y * w3m[cc], acc);
      acc = mfma16x16x4(in ? av.z : 0.f, w3v[cc].z * w3m[cc], acc);
      acc = mfma16x16x4(in ? av.w : 0.f, w3v[cc].w * w3m[cc], acc);
    }
    if (j < a.H) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int ii = i0 + 4 * q + rr;
        if (ii < a.M) a.h3[((size_t)s * a.M + ii) * a.H + j] = fmaxf(acc[rr] + bj, 0.f);
      }
    }
  }
  if (g == 0) {
    if (valid) {
      const size_t v = (size_t)s * a.M + i;
      a.eps[v * a.Z + c] = ep;
      a.z[v * a.Z + c] = zz;
      if (s == 0) {
        a.mulv[(size_t)i * Z2 + c] = mu;
        a.mulv[(size_t)i * Z2 + a.Z + c] = lv;
      }
    }
    if (e < 16 && i0 + e < a.M) {  // row e of the tile: its Z terms in latent order
      float t = 0.f;
      for (int cc = 0; cc < a.Z; ++cc) t += pt[e][cc];
      a.prior[(size_t)s * a.M + i0 + e] = t;
    }
  }
}

// ------------------------------------------------------- decoder + BCE ----
// Workgroup = kIwRowTile (2 x 16) virtual rows, all D columns. The h3 tile is
// staged in LDS once ([32][ceil16(H) + 4] floats, zero past H and past the
// last row; the +4 keeps the 16 rows of a float4 fragment read on distinct
// banks); wave w takes column tiles w, w+8, ...: per 16-deep k chunk one
// dwordx4 of W4 per lane feeds both row tiles (8 MFMAs), the loads of kIwNcw
// chunks issued back to back. Each lane keeps the BCE of its 8 rows over its
// columns; the 16 lanes of a row combine by butterfly, the 8 waves through LDS
// in wave order.
constexpr int kIwNcw = 5;

__global__ void __launch_bounds__(kThreads) iw_dec_bce_k(IwArgs a) {
  extern __shared__ __attribute__((aligned(16))) float at[];
  __shared__ float red[kWaves][kIwRowTile];
  const int V = a.S * a.M;
  const int hp16 = cdiv_d(a.H, 16) * 16, lda = hp16 + 4, nch = hp16 / 16;
  const int v0 = blockIdx.x * kIwRowTile;
  {
    const int q4 = hp16 / 4;
    for (int e = threadIdx.x; e < kIwRowTile * q4; e += kThreads) {
      const int r = e / q4, k4 = e - r * q4;
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (v0 + r < V && 4 * k4 < a.H) v = *reinterpret_cast<const float4*>(a.h3 + (size_t)(v0 + r) * a.H + 4 * k4);
      *reinterpret_cast<float4*>(at + r * lda + 4 * k4) = v;
    }
  }
  __syncthreads();
  const int w = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int r = lane & 15, q = lane >> 4;
  const int tiles_j = cdiv_d(a.D, 16);
  float rl[2][4];
  const float* xrow[2][4];
  bool ok[2][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int v = v0 + mt * 16 + 4 * q + rr;
      ok[mt][rr] = v < V;
      xrow[mt][rr] = a.xb + (size_t)((ok[mt][rr] ? v : 0) % a.M) * a.D;  // virtual row -> image row
      rl[mt][rr] = 0.f;
    }
  const float* a0p = at + r * lda + 4 * q;
  const float* a1p = at + (16 + r) * lda + 4 * q;
  for (int jt = w; jt < tiles_j; jt += kWaves) {
    const int j = jt * 16 + r;
    const int jc = min(j, a.D - 1);
    const float* wrow = a.W4 + (size_t)jc * a.H + 4 * q;
    const float bj = a.b4[jc];
    float x[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) x[mt][rr] = xrow[mt][rr][jc];
    f32x4 acc[2][2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) acc[mt][0] = acc[mt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc0 = 0; kc0 < nch; kc0 += kIwNcw) {
      float4 b[kIwNcw];
#pragma unroll
      for (int u = 0; u < kIwNcw; ++u) {
        // past-the-end chunks and k >= H load a clamped in-bounds address; their
        // A values are zero (staging) or the chunk is skipped below
        const int k0 = min(kc0 + u, nch - 1) * 16;
        b[u] = *reinterpret_cast<const float4*>(wrow + min(k0, a.H - 4 - 4 * q));
      }
      __builtin_amdgcn_sched_barrier(0);  // all loads of the round in flight before the first MFMA
#pragma unroll
      for (int u = 0; u < kIwNcw; ++u) {
        if (kc0 + u < nch) {  // wave-uniform
          const int k0 = (kc0 + u) * 16;
          const float4 a0 = *reinterpret_cast<const float4*>(a0p + k0);
          const float4 a1 = *reinterpret_cast<const float4*>(a1p + k0);
          acc[0][0] = mfma16x16x4(a0.x, b[u].x, acc[0][0]);
          acc[1][0] = mfma16x16x4(a1.x, b[u].x, acc[1][0]);
          acc[0][1] = mfma16x16x4(a0.y, b[u].y, acc[0][1]);
          acc[1][1] = mfma16x16x4(a1.y, b[u].y, acc[1][1]);
          acc[0][0] = mfma16x16x4(a0.z, b[u].z, acc[0][0]);
          acc[1][0] = mfma16x16x4(a1.z, b[u].z, acc[1][0]);
          acc[0][1] = mfma16x16x4(a0.w, b[u].w, acc[0][1]);
          acc[1][1] = mfma16x16x4(a1.w, b[u].w, acc[1][1]);
        }
      }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float t = (acc[mt][0][rr] + acc[mt][1][rr]) + bj;
        const float term = bce_logit_term(t, x[mt][rr]);
        rl[mt][rr] += (j < a.D && ok[mt][rr]) ? term : 0.f;
      }
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      float v = rl[mt][rr];
      v += __shfl_xor(v, 1, 64);
      v += __shfl_xor(v, 2, 64);
      v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64);
      if (r == 0) red[w][mt * 16 + 4 * q + rr] = v;
    }
  __syncthreads();
  if (threadIdx.x < kIwRowTile && v0 + (int)threadIdx.x < V) {
    float t = 0.f;
#pragma unroll
    for (int s = 0; s < kWaves; ++s) t += red[s][threadIdx.x];
    a.bce[v0 + threadIdx.x] = t;
  }
}

// -------------------------------------------------------------- reduce ----
// One workgroup. Thread t owns batch rows t, t + 256, ...: the chunk's S
// log-weights of a row are folded, in sample order, into the row's running
// max / scaled sum (the values sit near -540 with a spread of ~10 nats: a
// plain exp underflows) and running sum. After the last chunk: the per-row
// results at cursor*B + i, the batch totals in double (per-thread sums in row
// order, then a fixed tree), added to the pass state by thread 0, which also
// advances the cursor.
constexpr int kIwRedThreads = 256;

__global__ void __launch_bounds__(kIwRedThreads) iw_reduce_k(IwArgs a) {
  __shared__ double sn[kIwRedThreads], se[kIwRedThreads];
  const int cursor = a.ist->st.cursor;
  const float logk = logf((float)a.K);
  double tn = 0.0, te = 0.0;
  for (int i = threadIdx.x; i < a.M; i += kIwRedThreads) {
    float m = -INFINITY, ss = 0.f, ls = 0.f;
    if (!a.first) { m = a.lse_m[i]; ss = a.lse_s[i]; ls = a.lw_sum[i]; }
    for (int s = 0; s < a.S; ++s) {
      const size_t v = (size_t)s * a.M + i;
      const float lw = a.prior[v] - a.bce[v];
      if (lw > m) {
        ss = ss * expf(m - lw) + 1.f;
        m = lw;
      } else {
        ss += expf(lw - m);
      }
      ls += lw;
    }
    if (a.last) {
      const float nll = -(m + logf(ss) - logk);
      const float ne = -ls / (float)a.K;
      const long long o = (long long)cursor * a.B + i;
      if (o < a.rows_cap) {
        a.row_nll[o] = nll;
        a.row_neg_elbo[o] = ne;
      }
      tn += (double)nll;
      te += (double)ne;
    } else {
      a.lse_m[i] = m; a.lse_s[i] = ss; a.lw_sum[i] = ls;
    }
  }
  if (!a.last) return;
  sn[threadIdx.x] = tn;
  se[threadIdx.x] = te;
  __syncthreads();
  for (int o = kIwRedThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sn[threadIdx.x] += sn[threadIdx.x + o];
      se[threadIdx.x] += se[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    IwState* st = a.ist;
    st->nll += sn[0];
    st->neg_elbo += se[0];
    int cur = cursor + 1;
    if (st->st.nbatches > 0 && cur >= st->st.nbatches) cur = 0;
    st->st.cursor = cur;
  }
}

}  // namespace mdt

using namespace mdt;

static inline int iw_cdiv(int a, int b) { return (a + b - 1) / b; }

extern "C" int mdt_iw_check(const IwArgs* a) {
  if (a->M <= 0 || a->M > a->B || a->B > kMaxBatch) return 1;
  if (a->Z > 32 || a->Z <= 0 || (a->Z & 3) || 16 * a->Z > kThreads) return 2;
  if ((a->D & 3) || (a->H & 3) || a->H > 16 * 32) return 3;
  if (a->K < 1 || a->S < 1 || a->k0 < 0 || a->k0 + a->S > a->K) return 4;
  if ((unsigned long long)a->K * (unsigned long long)a->B * (unsigned long long)a->Z > (1ull << 32)) return 4;
  if ((long long)a->S * a->M > (long long)a->cap_rows) return 5;
  if (kIwRowTile * (iw_cdiv(a->H, 16) * 16 + 4) * (int)sizeof(float) > kIwMaxLds) return 6;
  if (!a->slab_mv || !a->xb || !a->h3 || !a->prior || !a->bce || !a->eps || !a->z || !a->mulv || !a->lse_m ||
      !a->lse_s || !a->lw_sum || !a->row_nll || !a->row_neg_elbo || !a->ist || !a->hp)
    return 7;
  return 0;
}

// The reduce kernel alone (conv-VAE pass: prior / bce come from conv_iw.hip).
extern "C" int mdt_iw_reduce(const IwArgs* a, hipStream_t s) {
  if (a->M <= 0 || a->M > a->B || a->K < 1 || a->S < 1 || a->S > a->K) return 1;
  if (!a->prior || !a->bce || !a->lse_m || !a->lse_s || !a->lw_sum || !a->row_nll || !a->row_neg_elbo || !a->ist) return 7;
  hipLaunchKernelGGL(iw_reduce_k, dim3(1), dim3(kIwRedThreads), 0, s, *a);
  return (int)hipGetLastError();
}

extern "C" int mdt_iw_chunk(const IwArgs* a, hipStream_t s) {
  const int rc = mdt_iw_check(a);
  if (rc) return rc;
  const SlabGeo geo(a->H, a->Z);
  const int V = a->S * a->M;
  const size_t lds = (size_t)kIwRowTile * (iw_cdiv(a->H, 16) * 16 + 4) * sizeof(float);
  hipLaunchKernelGGL(iw_sample_k, dim3(a->S * iw_cdiv(a->M, 16) * geo.groups), dim3(kThreads), 0, s, *a);
  hipLaunchKernelGGL(iw_dec_bce_k, dim3(iw_cdiv(V, kIwRowTile)), dim3(kThreads), lds, s, *a);
  hipLaunchKernelGGL(iw_reduce_k, dim3(1), dim3(kIwRedThreads), 0, s, *a);
  return (int)hipGetLastError();
}
