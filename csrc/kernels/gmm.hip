// Ex-post Gaussian-mixture prior (models/gmm.py): EM for K full-covariance
// components on rows z [n, Z], float32 throughout, three launches per
// iteration and no [n, K, Z] temporary.
//
//   gmm_prepare_k   grid K, one workgroup per component. With `fold` it first
//                   sums the M-step's per-strip records in strip order into the
//                   component's next (pi, mu, cov); so the fold and the next
//                   iteration's prepare are one launch. Then cov_k + reg I sits
//                   in LDS (stride 65), a right-looking Cholesky runs column by
//                   column (scale the column, rank-1 update of the trailing
//                   lower triangle, two barriers a column), thread c solves
//                   L w = e_c by forward substitution for column c of
//                   W_k = L_k^-1 (a column is one thread's, so no barrier), and
//                   c_k = log pi_k - sum log L_ii - Z/2 log 2 pi. A pivot that
//                   is not positive sets the component's status word and is
//                   replaced by 1 so the launch ends; the host raises after the
//                   call. Workgroup 0 also folds the E-step's per-tile sums of
//                   ll, in double, in a fixed tree.
//   gmm_estep_k     one workgroup per 128-row tile, which lives in LDS. For
//                   each k in turn W_k and mu_k are staged in LDS, the next
//                   pair's global loads in flight under the MFMA loop (two
//                   buffers, one barrier per k). Y = (Z_tile - mu_k) W_k^T runs
//                   on the exact-f32 MFMA 16x16x4, a wave owning 32 rows and
//                   every 16-wide block of outputs; mu_k is subtracted from the
//                   A fragment before the product (W (z - mu), never
//                   W z - W mu), and the all-zero blocks above W_k's diagonal
//                   are skipped (10 of 16 block pairs at Z = 64). |y|^2 comes
//                   from the accumulators: squares summed over a lane's
//                   blocks, then over the 16 lanes of a row by four
//                   exchanges. lp [128, K] stays in LDS; after the last k a
//                   max / sum pass per row gives ll and r = exp(lp - ll), and
//                   the tile's sum of ll goes to its own slot. No atomics.
//   gmm_mstep_k     grid (k, strip of row tiles); strips are a function of
//                   (n, K). S = sum_n (r_nk d_n) d_n^T with d = z_n - mu_old_k:
//                   the MFMA's k dimension is the rows, so the value a lane
//                   loads for (row, column) is the B operand as it is and the A
//                   operand after one multiply by r. The Z x Z accumulator is
//                   in registers, the blocks on and below the diagonal only;
//                   N_k and sum r d ride along in the same lanes. A wave takes
//                   every fourth group of four rows; the four waves' sums meet
//                   in LDS in wave order and go to [strip][k][1 + Z + Z Z].
//                   z is re-read K times, from L2.
#include "common.h"
#include "gmm.h"

namespace mdt {

namespace {

enum : int { kGmmFold = 1, kGmmInit = 2, kGmmChol = 4, kGmmFoldLl = 8, kGmmResetStatus = 16 };

constexpr int kGmmLdC = kGmmMaxZ + 1;  // prepare: LDS stride of the factor

__global__ __launch_bounds__(kGmmThreads) void gmm_prepare_k(GmmArgs a, int flags, int strips, int hist_at) {
  __shared__ float A[kGmmMaxZ * kGmmLdC];
  __shared__ float Wl[kGmmMaxZ * kGmmLdC];
  __shared__ float dm[kGmmMaxZ];
  __shared__ float diagL[kGmmMaxZ];
  __shared__ double red[kGmmThreads];
  const int k = blockIdx.x, tid = threadIdx.x, Z = a.Z, K = a.K, ZZ = Z * Z, rec = gmm_rec(Z);

  if ((flags & kGmmFoldLl) && k == 0) {  // mean ll of the last E-step: tile sums, strided then a tree, in double
    const int tiles = gmm_tiles(a.n);
    double s = 0.0;
    for (int t = tid; t < tiles; t += kGmmThreads) s += (double)a.llpart[t];
    red[tid] = s;
    __syncthreads();
    for (int o = kGmmThreads / 2; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) a.ll_hist[hist_at] = (float)(red[0] / (double)a.n);
  }

  const bool fold = (flags & (kGmmFold | kGmmInit)) != 0, init = (flags & kGmmInit) != 0;
  float pik = fold ? 0.f : a.pi[k];
  if (fold) {
    // the start: every component takes the one record of the whole data, centred on 0
    const int kk = init ? 0 : k, KK = init ? 1 : K;
    const float* p0 = a.mpart + (size_t)kk * rec;
    const size_t step = (size_t)KK * rec;
    float N = 0.f;
    for (int s = 0; s < strips; ++s) N += p0[s * step];
    const bool live = N > kGmmDeadWeight * (float)a.n;
    for (int i = tid; i < Z; i += kGmmThreads) {
      float v = 0.f;
      for (int s = 0; s < strips; ++s) v += p0[s * step + 1 + i];
      dm[i] = v / N;
    }
    __syncthreads();
    float* cv = a.cov_out + (size_t)k * ZZ;
    if (live) {
      for (int e = tid; e < ZZ; e += kGmmThreads) {
        const int i = e / Z, j = e - i * Z;
        if (j > i) continue;  // the lower triangle is computed, the upper is its mirror
        float v = 0.f;
        for (int s = 0; s < strips; ++s) v += p0[s * step + 1 + Z + e];
        v = v / N - dm[i] * dm[j];
        cv[i * Z + j] = v;
        cv[j * Z + i] = v;
      }
      const int row = (int)(((long long)(2 * k + 1) * a.n) / (2 * K));
      for (int i = tid; i < Z; i += kGmmThreads)
        a.mu_out[k * Z + i] = init ? a.z[(size_t)row * Z + i] : a.mu[k * Z + i] + dm[i];
    } else if (a.cov_out != a.cov) {  // a dead component keeps its mean and covariance
      for (int e = tid; e < ZZ; e += kGmmThreads) cv[e] = a.cov[(size_t)k * ZZ + e];
      for (int i = tid; i < Z; i += kGmmThreads) a.mu_out[k * Z + i] = a.mu[k * Z + i];
    }
    pik = init ? 1.f / (float)K : N / (float)a.n;
    if (tid == 0) a.pi_out[k] = pik;
    __syncthreads();  // cov_out is read back below
  }
  if (!(flags & kGmmChol)) return;

  const float* cv = (fold ? a.cov_out : a.cov) + (size_t)k * ZZ;
  for (int e = tid; e < ZZ; e += kGmmThreads) {
    const int i = e / Z, j = e - i * Z;
    A[i * kGmmLdC + j] = cv[e] + (i == j ? a.reg : 0.f);
    Wl[i * kGmmLdC + j] = 0.f;
  }
  float logdet = 0.f;
  bool bad_any = false;
  for (int j = 0; j < Z; ++j) {
    __syncthreads();  // the staging, or the previous column's trailing update
    const float p = A[j * kGmmLdC + j];
    const bool bad = !(p > 0.f);
    const float l = bad ? 1.f : sqrtf(p);
    bad_any |= bad;
    if (tid == 0) {
      diagL[j] = l;
      logdet += logf(l);
    }
    for (int i = j + 1 + tid; i < Z; i += kGmmThreads) A[i * kGmmLdC + j] /= l;
    __syncthreads();
    const int m = Z - j - 1;
    for (int e = tid; e < m * m; e += kGmmThreads) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) A[i * kGmmLdC + c] -= A[i * kGmmLdC + j] * A[c * kGmmLdC + j];
    }
  }
  __syncthreads();
  if (tid < Z) {  // column tid of L^-1
    for (int i = tid; i < Z; ++i) {
      float s = i == tid ? 1.f : 0.f;
      for (int m = tid; m < i; ++m) s -= A[i * kGmmLdC + m] * Wl[m * kGmmLdC + tid];
      Wl[i * kGmmLdC + tid] = s / diagL[i];
    }
  }
  __syncthreads();
  for (int e = tid; e < ZZ; e += kGmmThreads) {
    const int i = e / Z, j = e - i * Z;
    a.W[(size_t)k * ZZ + e] = Wl[i * kGmmLdC + j];
  }
  if (tid == 0) {
    a.c[k] = logf(pik) - logdet - (float)(0.91893853320467274178 * (double)Z);
    if (bad_any || (flags & kGmmResetStatus)) a.status[k] = bad_any ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(kGmmThreads) void gmm_estep_k(GmmArgs a) {
  extern __shared__ __attribute__((aligned(16))) float gmm_lds[];
  const int Z = a.Z, K = a.K, n = a.n, zp = gmm_zpad(Z), ld = gmm_ld(Z), zb = zp >> 4, ZZ = Z * Z, ldp = K + 1;
  float* zt = gmm_lds;                  // [128][ld] the row tile, zero past Z and past n
  float* Wb = zt + kGmmTile * ld;       // [2][zp][ld]
  float* mub = Wb + 2 * zp * ld;        // [2][64]
  float* lp = mub + 2 * kGmmMaxZ;       // [128][K + 1]
  float* lls = lp + kGmmTile * ldp;     // [128]
  float* red = lls + kGmmTile;          // [8]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int row0 = blockIdx.x * kGmmTile;

  for (int e = tid; e < kGmmTile * zp; e += kGmmThreads) {
    const int rr = e / zp, cc = e - rr * zp, g = row0 + rr;
    zt[rr * ld + cc] = (g < n && cc < Z) ? a.z[(size_t)g * Z + cc] : 0.f;
  }
  for (int e = tid; e < zp * zp; e += kGmmThreads) {
    const int o = e / zp, i = e - o * zp;
    Wb[o * ld + i] = (o < Z && i < Z) ? a.W[o * Z + i] : 0.f;
  }
  if (tid < kGmmMaxZ) mub[tid] = tid < Z ? a.mu[tid] : 0.f;
  __syncthreads();

  for (int k = 0; k < K; ++k) {
    const float* Wc = Wb + (k & 1) * zp * ld;
    const float* mc = mub + (k & 1) * kGmmMaxZ;
    // the next component's factor and mean: loads now, LDS stores after the MFMA loop
    const bool more = k + 1 < K;
    float wn[16], mn = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int e = tid + q * kGmmThreads;
      wn[q] = 0.f;
      if (more && e < zp * zp) {
        const int o = e / zp, i = e - o * zp;
        if (o < Z && i < Z) wn[q] = a.W[(size_t)(k + 1) * ZZ + o * Z + i];
      }
    }
    if (more && tid < Z) mn = a.mu[(k + 1) * Z + tid];

    f32x4 acc[2][4];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int ob = 0; ob < 4; ++ob) acc[rb][ob] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) {
      if (ib < zb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int i = ib * 16 + 4 * s + lq;
          const float m = mc[i];
          const float a0 = zt[(wave * 32 + lr) * ld + i] - m;
          const float a1 = zt[(wave * 32 + 16 + lr) * ld + i] - m;
#pragma unroll
          for (int ob = ib; ob < 4; ++ob) {  // W_k is lower triangular: output block ob needs input blocks <= ob
            if (ob < zb) {
              const float b = Wc[(ob * 16 + lr) * ld + i];
              acc[0][ob] = mfma16x16x4(a0, b, acc[0][ob]);
              acc[1][ob] = mfma16x16x4(a1, b, acc[1][ob]);
            }
          }
        }
      }
    }
    // |y|^2 of row 16 rb + 4 lq + j: this lane's blocks, then the 16 lanes of the row
    const float ck = a.c[k];
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float q = 0.f;
#pragma unroll
        for (int ob = 0; ob < 4; ++ob)
          if (ob < zb) q = fmaf(acc[rb][ob][j], acc[rb][ob][j], q);
        q += __shfl_xor(q, 1, 64);
        q += __shfl_xor(q, 2, 64);
        q += __shfl_xor(q, 4, 64);
        q += __shfl_xor(q, 8, 64);
        if (lr == 0) lp[(wave * 32 + rb * 16 + 4 * lq + j) * ldp + k] = ck - 0.5f * q;
      }
    if (more) {
      float* Wn = Wb + ((k + 1) & 1) * zp * ld;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int e = tid + q * kGmmThreads;
        if (e < zp * zp) {
          const int o = e / zp, i = e - o * zp;
          Wn[o * ld + i] = wn[q];
        }
      }
      if (tid < kGmmMaxZ) mub[((k + 1) & 1) * kGmmMaxZ + tid] = mn;
    }
    __syncthreads();
  }

  float llv = 0.f;
  if (tid < kGmmTile) {
    const float* p = lp + tid * ldp;
    float m = p[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, p[k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(p[k] - m);
    llv = m + logf(s);
    lls[tid] = llv;
    if (row0 + tid < n) a.ll[row0 + tid] = llv;
    else llv = 0.f;
  }
  llv = wave_sum(llv);
  if (lane == 0) red[wave] = llv;
  __syncthreads();
  if (tid == 0) a.llpart[blockIdx.x] = red[0] + red[1];
  if (a.r != nullptr) {
    for (int e = tid; e < kGmmTile * K; e += kGmmThreads) {
      const int rr = e / K, kk = e - rr * K;
      if (row0 + rr < n) a.r[(size_t)row0 * K + e] = expf(lp[rr * ldp + kk] - lls[rr]);
    }
  }
}

// the accumulator of block (ib, jb), jb <= ib
__device__ __forceinline__ constexpr int gmm_tri(int ib, int jb) { return ib * (ib + 1) / 2 + jb; }

// K: the components of this launch and the stride of r (1 for the start, whose r is 1 and whose centre is 0)
__global__ __launch_bounds__(kGmmThreads) void gmm_mstep_k(GmmArgs a, int K, int strip_tiles, int init) {
  __shared__ float out[1 + kGmmMaxZ + kGmmMaxZ * kGmmMaxZ];
  const int k = blockIdx.x, strip = blockIdx.y, Z = a.Z, zb = gmm_zpad(Z) >> 4, n = a.n, rec = gmm_rec(Z);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
  const int rbeg = strip * strip_tiles * kGmmTile, rend = min(n, rbeg + strip_tiles * kGmmTile);

  float m[4], sd[4], Ns = 0.f;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const int col = b * 16 + lr;
    m[b] = (!init && col < Z) ? a.mu[k * Z + col] : 0.f;
    sd[b] = 0.f;
  }
  f32x4 acc[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  // lane (lr, lq) of a step holds row base + lq, columns 16 b + lr
  for (int base = rbeg + wave * 4; base < rend; base += 16) {
    const int g = base + lq;
    const bool ok = g < rend;
    const float rv = !ok ? 0.f : init ? 1.f : a.r[(size_t)g * K + k];
    float d[4], ra[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = b * 16 + lr;
      d[b] = (ok && col < Z) ? a.z[(size_t)g * Z + col] - m[b] : 0.f;
      ra[b] = rv * d[b];
      sd[b] += ra[b];
    }
    Ns += rv;
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
      if (ib < zb) {
#pragma unroll
        for (int jb = 0; jb <= ib; ++jb) acc[gmm_tri(ib, jb)] = mfma16x16x4(ra[ib], d[jb], acc[gmm_tri(ib, jb)]);
      }
  }
  // the four row groups of the wave
  Ns += __shfl_xor(Ns, 16, 64);
  Ns += __shfl_xor(Ns, 32, 64);
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    sd[b] += __shfl_xor(sd[b], 16, 64);
    sd[b] += __shfl_xor(sd[b], 32, 64);
  }
  // the four waves, in wave order
  for (int w = 0; w < kGmmThreads / kWave; ++w) {
    if (wave == w) {
      if (lane == 0) out[0] = (w ? out[0] : 0.f) + Ns;
      if (lq == 0) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int col = b * 16 + lr;
          if (col < Z) out[1 + col] = (w ? out[1 + col] : 0.f) + sd[b];
        }
      }
#pragma unroll
      for (int ib = 0; ib < 4; ++ib)
#pragma unroll
        for (int jb = 0; jb <= ib; ++jb)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int i = ib * 16 + 4 * lq + q, j = jb * 16 + lr;
            if (i < Z && j < Z) {
              float* o = out + 1 + Z + i * Z + j;
              *o = (w ? *o : 0.f) + acc[gmm_tri(ib, jb)][q];
            }
          }
    }
    __syncthreads();
  }
  float* dst = a.mpart + ((size_t)strip * K + k) * rec;
  for (int e = tid; e < rec; e += kGmmThreads) {
    if (e >= 1 + Z) {
      const int i = (e - 1 - Z) / Z, j = (e - 1 - Z) - i * Z;
      if ((j >> 4) > (i >> 4)) continue;  // blocks above the diagonal are neither computed nor read
    }
    dst[e] = out[e];
  }
}

int gmm_sizes(const GmmArgs* a) {
  if (a->K < 1 || a->K > kGmmMaxK) return 3;
  if (a->n <= a->K || a->n > kGmmMaxRows) return 1;
  if (a->Z < 1 || a->Z > kGmmMaxZ) return 2;
  return 0;
}

bool gmm_ok() { return hipGetLastError() == hipSuccess; }

void gmm_prepare(const GmmArgs& a, int flags, int hist_at, hipStream_t s) {
  const int strips = gmm_strips(a.n, (flags & kGmmInit) ? 1 : a.K);
  const int grid = (flags & ~kGmmFoldLl) ? a.K : 1;
  hipLaunchKernelGGL(gmm_prepare_k, dim3((unsigned)grid), dim3(kGmmThreads), 0, s, a, flags, strips, hist_at);
}

bool gmm_estep(const GmmArgs& a, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&gmm_estep_k),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)gmm_estep_lds(kGmmMaxZ, kGmmMaxK));
  if (attr != hipSuccess) return false;
  hipLaunchKernelGGL(gmm_estep_k, dim3((unsigned)gmm_tiles(a.n)), dim3(kGmmThreads), gmm_estep_lds(a.Z, a.K), s, a);
  return true;
}

void gmm_mstep(const GmmArgs& a, bool init, hipStream_t s) {
  const int K = init ? 1 : a.K;
  hipLaunchKernelGGL(gmm_mstep_k, dim3((unsigned)K, (unsigned)gmm_strips(a.n, K)), dim3(kGmmThreads), 0, s, a, K,
                     gmm_strip_tiles(a.n, K), init ? 1 : 0);
}

}  // namespace

}  // namespace mdt

extern "C" int mdt_gmm_check(const mdt::GmmArgs* a) {
  const int rc = mdt::gmm_sizes(a);
  if (rc) return rc;
  return a->z && a->pi && a->mu && a->cov && a->W && a->c && a->status && a->ll && a->llpart && a->mpart ? 0 : 4;
}

extern "C" int mdt_gmm_fit(const mdt::GmmArgs* a, int iters, hipStream_t s) {
  using namespace mdt;
  int rc = mdt_gmm_check(a);
  if (rc) return rc;
  if (iters < 0 || iters > kGmmMaxIters) return 5;
  if (!a->r || !a->ll_hist) return 4;
  GmmArgs b = *a;
  b.pi_out = b.pi, b.mu_out = b.mu, b.cov_out = b.cov;
  gmm_mstep(b, true, s);
  gmm_prepare(b, kGmmInit | kGmmChol | kGmmResetStatus, 0, s);
  for (int t = 0; t < iters; ++t) {
    if (!gmm_estep(b, s)) return 9;
    gmm_mstep(b, false, s);
    gmm_prepare(b, kGmmFold | kGmmChol | kGmmFoldLl, t, s);
  }
  if (!gmm_estep(b, s)) return 9;
  gmm_prepare(b, kGmmFoldLl, iters, s);
  return gmm_ok() ? 0 : 9;
}

extern "C" int mdt_gmm_em_step(const mdt::GmmArgs* a, hipStream_t s) {
  using namespace mdt;
  const int rc = mdt_gmm_check(a);
  if (rc) return rc;
  if (!a->r || !a->pi_out || !a->mu_out || !a->cov_out) return 4;
  gmm_prepare(*a, kGmmChol | kGmmResetStatus, 0, s);
  if (!gmm_estep(*a, s)) return 9;
  gmm_mstep(*a, false, s);
  gmm_prepare(*a, kGmmFold, 0, s);
  return gmm_ok() ? 0 : 9;
}

extern "C" int mdt_gmm_score(const mdt::GmmArgs* a, hipStream_t s) {
  using namespace mdt;
  const int rc = mdt_gmm_check(a);
  if (rc) return rc;
  GmmArgs b = *a;
  b.r = nullptr;
  gmm_prepare(b, kGmmChol | kGmmResetStatus, 0, s);
  if (!gmm_estep(b, s)) return 9;
  return gmm_ok() ? 0 : 9;
}
