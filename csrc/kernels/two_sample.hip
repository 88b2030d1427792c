// Two-sample statistics of generated against held-out images: the per-row table
// behind the kernel MMD and the 1-NN two-sample test (models/sample_report.py).
//
// For the union U of na real and nb fake rows [*, D] and every row i, over all
// other rows j:  d2 = max(0, q_i + q_j - 2 G_ij) with G = U U^T and q the rows'
// squared norms; the nearest d2 to a real and to a fake row, and the sums of
// exp(-d2 / h_s) over the real and over the fake rows at three bandwidths.
//
//   ts_norms_k  q[i], one wave per row.
//   ts_pair_k   one workgroup per (row tile, strip of column tiles). G comes from the
//               exact-f32 MFMA 32x32x2 (a k-ordered fma chain per element): a
//               128 x 128 tile per 256 threads, 2 x 2 MFMA tiles per wave, K in
//               LDS chunks of 32 with the tail of D zero-filled. Both operands
//               are tiles of U, read in place through the two base pointers.
//               The workgroup's own 128 rows are the MFMA's B operand, so an
//               own row sits on a lane (two per lane) with its two minima and
//               six sums in registers, and the 32 accumulator registers of a
//               lane are 32 rows of the strip's current tile: the running
//               state needs no cross-lane step until the strip ends. Then the
//               two lane halves and the two waves that share a row combine in
//               a fixed order and one partial per (strip, row) is written.
//               G is symmetric, so a pair of tiles is multiplied once (the
//               schedule: two_sample.h): where the tile also serves the rows of
//               the strip's tile, each of its rows is reduced over the lanes
//               (the own rows) right in the epilogue, the two waves that share
//               it combine through LDS, and one partial per (offset, row) is
//               written.
//   ts_fold_k   merges a row's partials in strip, then offset order, the sums
//               in double.
//
// No atomics and a strip count that depends on na + nb alone: results repeat
// bitwise. The (na + nb)^2 matrix never exists.
#include "common.h"
#include "two_sample.h"

namespace mdt {

namespace {

constexpr float kTsInf = __builtin_huge_valf();

__device__ __forceinline__ const float* ts_row(const TwoSampleArgs& a, int u) {
  return u < a.na ? a.real + (size_t)u * a.D : a.fake + (size_t)(u - a.na) * a.D;
}

__global__ __launch_bounds__(kTsNormThreads) void ts_norms_k(TwoSampleArgs a) {
  const int u = blockIdx.x * (kTsNormThreads / kWave) + wave_id();
  if (u >= a.na + a.nb) return;
  const float* p = ts_row(a, u);
  float s = 0.f;
  for (int k = lane_id(); k < a.D; k += kWave) s = fmaf(p[k], p[k], s);
  s = wave_sum(s);
  if (lane_id() == 0) a.q[u] = s;
}

// Four consecutive k of one row, zero past the row's end (and for a row past the union's)
template <bool VEC>
__device__ __forceinline__ float4 ts_load4(const float* p, int k, int D) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p == nullptr) return v;
  if (VEC) {  // D % 4 == 0 and 16-byte aligned rows: k < D covers all four
    if (k < D) v = *reinterpret_cast<const float4*>(p + k);
  } else {
    if (k < D) v.x = p[k];
    if (k + 1 < D) v.y = p[k + 1];
    if (k + 2 < D) v.z = p[k + 2];
    if (k + 3 < D) v.w = p[k + 3];
  }
  return v;
}

// The running state of one own row
struct TsRow {
  float dmin[2];                 // nearest real, nearest fake
  float ksum[2][kTsBandwidths];  // over the real, over the fake rows
};

// exp(d2 * c) with c = hi + lo: expf of the rounded product, corrected to first
// order by the product's rounding error and the low word (|r| < 1e-5)
__device__ __forceinline__ float ts_kernel_value(float d2, float hi, float lo) {
  const float t = d2 * hi;
  const float r = fmaf(d2, lo, fmaf(d2, hi, -t));
  const float e = expf(t);
  return fmaf(e, r, e);
}

// One accumulator tile pair of a lane into its two own rows: per element the
// masks for j = i, rows past the union's end and the kind of j.
// TRANS: the tile also serves the rows of the strip's tile (never the diagonal
// tile). Each such row is reduced over the lane's two own rows (masked by their
// kind), then over the 32 lanes of the half by an xor butterfly (every lane ends
// with the same value), and lane r keeps the row of its accumulator slot
// (m, reg) = (r >> 4, r & 15) in `keep`.
template <bool TRANS>
__device__ __forceinline__ void ts_epilogue(const TwoSampleArgs& a, const f32x16 (&acc)[2][2], const float* qs,
                                            int t0, int wr, int h, int r, const int (&o)[2], const float (&qo)[2],
                                            TsRow (&st)[2], TsRow& keep) {
  const int N = a.na + a.nb;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int tl = wr * 64 + m * 32 + 8 * g + 4 * h;
      const float4 q4 = *reinterpret_cast<const float4*>(qs + tl);
      const float qt[4] = {q4.x, q4.y, q4.z, q4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = t0 + tl + e;
        TsRow row;  // TRANS: row t over this lane's own rows
        row.dmin[0] = row.dmin[1] = kTsInf;
#pragma unroll
        for (int s = 0; s < kTsBandwidths; ++s) row.ksum[0][s] = row.ksum[1][s] = 0.f;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const float d2 = fmaxf(0.f, fmaf(-2.f, acc[m][n][4 * g + e], qo[n] + qt[e]));
          float k[kTsBandwidths];
#pragma unroll
          for (int s = 0; s < kTsBandwidths; ++s) k[s] = ts_kernel_value(d2, a.c_hi[s], a.c_lo[s]);
          {
            const bool valid = t < N && t != o[n];
            const bool real = t < a.na;
            const float dv = valid ? d2 : kTsInf;
            st[n].dmin[0] = fminf(st[n].dmin[0], real ? dv : kTsInf);
            st[n].dmin[1] = fminf(st[n].dmin[1], real ? kTsInf : dv);
#pragma unroll
            for (int s = 0; s < kTsBandwidths; ++s) {
              const float kv = valid ? k[s] : 0.f;
              st[n].ksum[0][s] += real ? kv : 0.f;
              st[n].ksum[1][s] += real ? 0.f : kv;
            }
          }
          if (TRANS) {
            const bool valid = o[n] < N;
            const bool real = o[n] < a.na;
            const float dv = valid ? d2 : kTsInf;
            row.dmin[0] = fminf(row.dmin[0], real ? dv : kTsInf);
            row.dmin[1] = fminf(row.dmin[1], real ? kTsInf : dv);
#pragma unroll
            for (int s = 0; s < kTsBandwidths; ++s) {
              const float kv = valid ? k[s] : 0.f;
              row.ksum[0][s] += real ? kv : 0.f;
              row.ksum[1][s] += real ? 0.f : kv;
            }
          }
        }
        if (TRANS) {
#pragma unroll
          for (int off = 1; off < 32; off <<= 1) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              row.dmin[c] = fminf(row.dmin[c], __shfl_xor(row.dmin[c], off, 64));
#pragma unroll
              for (int s = 0; s < kTsBandwidths; ++s) row.ksum[c][s] += __shfl_xor(row.ksum[c][s], off, 64);
            }
          }
          if (r == 16 * m + 4 * g + e) keep = row;
        }
      }
      // the scheduler's window: four rows' expf chains and butterflies at a time
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kTsThreads, 2) void ts_pair_k(TwoSampleArgs a) {
  // A: the strip's current tile, B: the own tile, [row][kTsLd]; qs: norms of A's rows;
  // tr: per wave column, A's rows reduced over that wave's own rows.
  // After the strip the A region carries the cross-wave combine of the own rows.
  __shared__ __attribute__((aligned(16))) float lds[2 * kTsTile * kTsLd + kTsTile + 2 * kTsTile * kTsCols];
  float* As = lds;
  float* Bs = lds + kTsTile * kTsLd;
  float* qs = lds + 2 * kTsTile * kTsLd;
  float* tr = qs + kTsTile;

  const int N = a.na + a.nb, D = a.D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
  const int own0 = blockIdx.x * kTsTile;
  const int tiles = (N + kTsTile - 1) / kTsTile, offs = tiles / 2 + 1;
  const int per = (offs + (int)gridDim.y - 1) / (int)gridDim.y;
  const int d_begin = blockIdx.y * per;
  const int d_end = min(offs, d_begin + per);

  // staging: thread -> rows srow + 32 i (i < 4), four k at sk of the chunk
  const int srow = tid >> 3, sk = (tid & 7) * 4;
  const float* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = own0 + srow + 32 * i;
    pb[i] = u < N ? ts_row(a, u) : nullptr;
  }

  int o[2];
  float qo[2];
  TsRow st[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    o[n] = own0 + wc * 64 + n * 32 + r;
    qo[n] = o[n] < N ? a.q[o[n]] : 0.f;
    st[n].dmin[0] = st[n].dmin[1] = kTsInf;
#pragma unroll
    for (int s = 0; s < kTsBandwidths; ++s) st[n].ksum[0][s] = st[n].ksum[1][s] = 0.f;
  }

  for (int d = d_begin; d < d_end; ++d) {
    const int ct = blockIdx.x + d < tiles ? blockIdx.x + d : blockIdx.x + d - tiles;
    const int t0 = ct * kTsTile;
    const bool trans = d >= 1 && 2 * d < tiles;  // the tile serves the rows of tile ct as well
    const float* pa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = t0 + srow + 32 * i;
      pa[i] = u < N ? ts_row(a, u) : nullptr;
    }
    __syncthreads();  // the previous tile's epilogue has read qs
    if (tid < kTsTile) qs[tid] = t0 + tid < N ? a.q[t0 + tid] : 0.f;

    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;

    float4 ra[4], rb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = ts_load4<VEC>(pa[i], sk, D);
      rb[i] = ts_load4<VEC>(pb[i], sk, D);
    }
    for (int k0 = 0; k0 < D; k0 += kTsBK) {
      __syncthreads();  // the previous chunk's fragments are read
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<float4*>(As + (srow + 32 * i) * kTsLd + sk) = ra[i];
        *reinterpret_cast<float4*>(Bs + (srow + 32 * i) * kTsLd + sk) = rb[i];
      }
      __syncthreads();
      if (k0 + kTsBK < D) {  // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          ra[i] = ts_load4<VEC>(pa[i], k0 + kTsBK + sk, D);
          rb[i] = ts_load4<VEC>(pb[i], k0 + kTsBK + sk, D);
        }
      }
      // lane half h takes k = 8 c + 4 h + j of the chunk in MFMA step (c, j), from both
      // operands alike: one 16-byte read feeds four steps
#pragma unroll
      for (int c = 0; c < kTsBK / 8; ++c) {
        float4 av[2], bv[2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
          av[m] = *reinterpret_cast<const float4*>(As + (wr * 64 + m * 32 + r) * kTsLd + 8 * c + 4 * h);
#pragma unroll
        for (int n = 0; n < 2; ++n)
          bv[n] = *reinterpret_cast<const float4*>(Bs + (wc * 64 + n * 32 + r) * kTsLd + 8 * c + 4 * h);
        const float af[2][4] = {{av[0].x, av[0].y, av[0].z, av[0].w}, {av[1].x, av[1].y, av[1].z, av[1].w}};
        const float bf[2][4] = {{bv[0].x, bv[0].y, bv[0].z, bv[0].w}, {bv[1].x, bv[1].y, bv[1].z, bv[1].w}};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) acc[m][n] = mfma32x32x2(af[m][j], bf[n][j], acc[m][n]);
      }
    }

    TsRow keep;
    if (!trans) {
      ts_epilogue<false>(a, acc, qs, t0, wr, h, r, o, qo, st, keep);
      continue;
    }
    keep.dmin[0] = keep.dmin[1] = kTsInf;
#pragma unroll
    for (int s = 0; s < kTsBandwidths; ++s) keep.ksum[0][s] = keep.ksum[1][s] = 0.f;
    ts_epilogue<true>(a, acc, qs, t0, wr, h, r, o, qo, st, keep);
    {  // lane (r, h) holds row (r >> 4) * 32 + rowmap(r & 15, h) of its wave's 64: through LDS to the other wave column
      const int tl = wr * 64 + (r >> 4) * 32 + 8 * ((r & 15) >> 2) + 4 * h + (r & 3);
      float4* p = reinterpret_cast<float4*>(tr + (wc * kTsTile + tl) * kTsCols);
      p[0] = make_float4(keep.dmin[0], keep.dmin[1], keep.ksum[0][0], keep.ksum[0][1]);
      p[1] = make_float4(keep.ksum[0][2], keep.ksum[1][0], keep.ksum[1][1], keep.ksum[1][2]);
    }
    __syncthreads();  // the next write of tr follows the next tile's k loop and its barriers
    if (tid < kTsTile && t0 + tid < N) {
      const float4* p0 = reinterpret_cast<const float4*>(tr + tid * kTsCols);
      const float4* p1 = reinterpret_cast<const float4*>(tr + (kTsTile + tid) * kTsCols);
      const float4 x0 = p0[0], x1 = p0[1], y0 = p1[0], y1 = p1[1];
      float4* dst = reinterpret_cast<float4*>(a.tpart + ((size_t)(d - 1) * N + t0 + tid) * kTsCols);
      dst[0] = make_float4(fminf(x0.x, y0.x), fminf(x0.y, y0.y), x0.z + y0.z, x0.w + y0.w);
      dst[1] = make_float4(x1.x + y1.x, x1.y + y1.y, x1.z + y1.z, x1.w + y1.w);
    }
  }

  // Combine the lanes and waves that share an own row: lane half 0 with 1, then wave row 0 with 1.
#pragma unroll
  for (int n = 0; n < 2; ++n) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      st[n].dmin[c] = fminf(st[n].dmin[c], __shfl_xor(st[n].dmin[c], 32, 64));
#pragma unroll
      for (int s = 0; s < kTsBandwidths; ++s) st[n].ksum[c][s] += __shfl_xor(st[n].ksum[c][s], 32, 64);
    }
  }
  __syncthreads();  // every wave is done with As
  float* red = As;  // [kTsTile][kTsCols]
  if (wr == 1 && h == 0) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      float* p = red + (wc * 64 + n * 32 + r) * kTsCols;
      p[0] = st[n].dmin[0];
      p[1] = st[n].dmin[1];
#pragma unroll
      for (int s = 0; s < kTsBandwidths; ++s) {
        p[2 + s] = st[n].ksum[0][s];
        p[2 + kTsBandwidths + s] = st[n].ksum[1][s];
      }
    }
  }
  __syncthreads();
  if (wr == 0 && h == 0) {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      if (o[n] >= N) continue;
      const float* p = red + (wc * 64 + n * 32 + r) * kTsCols;
      float v[kTsCols];
      v[0] = fminf(st[n].dmin[0], p[0]);
      v[1] = fminf(st[n].dmin[1], p[1]);
#pragma unroll
      for (int s = 0; s < kTsBandwidths; ++s) {
        v[2 + s] = st[n].ksum[0][s] + p[2 + s];
        v[2 + kTsBandwidths + s] = st[n].ksum[1][s] + p[2 + kTsBandwidths + s];
      }
      float4* dst = reinterpret_cast<float4*>(a.part + ((size_t)blockIdx.y * N + o[n]) * kTsCols);
      dst[0] = make_float4(v[0], v[1], v[2], v[3]);
      dst[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
  }
}

__global__ __launch_bounds__(kTsFoldThreads) void ts_fold_k(TwoSampleArgs a) {
  const int N = a.na + a.nb;
  const int u = blockIdx.x * kTsFoldThreads + threadIdx.x;
  if (u >= N) return;
  float dmin[2] = {kTsInf, kTsInf};
  double sum[2 * kTsBandwidths] = {0, 0, 0, 0, 0, 0};
  for (int s = 0; s < a.strips; ++s) {
    const float4* p = reinterpret_cast<const float4*>(a.part + ((size_t)s * N + u) * kTsCols);
    const float4 lo = p[0], hi = p[1];
    dmin[0] = fminf(dmin[0], lo.x);
    dmin[1] = fminf(dmin[1], lo.y);
    sum[0] += lo.z; sum[1] += lo.w; sum[2] += hi.x;
    sum[3] += hi.y; sum[4] += hi.z; sum[5] += hi.w;
  }
  const int toffs = ts_toffsets(N);
  for (int d = 0; d < toffs; ++d) {
    const float4* p = reinterpret_cast<const float4*>(a.tpart + ((size_t)d * N + u) * kTsCols);
    const float4 lo = p[0], hi = p[1];
    dmin[0] = fminf(dmin[0], lo.x);
    dmin[1] = fminf(dmin[1], lo.y);
    sum[0] += lo.z; sum[1] += lo.w; sum[2] += hi.x;
    sum[3] += hi.y; sum[4] += hi.z; sum[5] += hi.w;
  }
  float4* dst = reinterpret_cast<float4*>(a.out + (size_t)u * kTsCols);
  dst[0] = make_float4(dmin[0], dmin[1], (float)sum[0], (float)sum[1]);
  dst[1] = make_float4((float)sum[2], (float)sum[3], (float)sum[4], (float)sum[5]);
}

}  // namespace

}  // namespace mdt

extern "C" int mdt_two_sample_check(const mdt::TwoSampleArgs* a) {
  using namespace mdt;
  if (a->na < 2 || a->na > kTsMaxRows || a->nb < 2 || a->nb > kTsMaxRows) return 1;
  if (a->D < 1 || a->D > kTsMaxD) return 2;
  if (a->strips != ts_strips((long long)a->na + a->nb)) return 3;
  if (!a->real || !a->fake || !a->q || !a->part || !a->tpart || !a->out) return 5;
  return 0;
}

extern "C" int mdt_two_sample_rows(const mdt::TwoSampleArgs* a, hipStream_t s) {
  using namespace mdt;
  const int rc = mdt_two_sample_check(a);
  if (rc) return rc;
  const int N = a->na + a->nb;
  const int tiles = ts_tiles(N);
  hipLaunchKernelGGL(ts_norms_k, dim3((unsigned)ts_cdiv(N, kTsNormThreads / kWave)), dim3(kTsNormThreads), 0, s, *a);
  const bool vec = a->D % 4 == 0 && (reinterpret_cast<uintptr_t>(a->real) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a->fake) & 15) == 0;
  const dim3 grid((unsigned)tiles, (unsigned)a->strips);
  if (vec) hipLaunchKernelGGL(ts_pair_k<true>, grid, dim3(kTsThreads), 0, s, *a);
  else hipLaunchKernelGGL(ts_pair_k<false>, grid, dim3(kTsThreads), 0, s, *a);
  hipLaunchKernelGGL(ts_fold_k, dim3((unsigned)ts_cdiv(N, kTsFoldThreads)), dim3(kTsFoldThreads), 0, s, *a);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}
