// Precision, recall, density and coverage on k-NN radii (models/prdc.py): the
// per-row table (rad, cnt, dminx) of real [na, D] against fake [nb, D].
//
// d2 = max(0, fma(-2, G, q_i + q_j)) with G a tile of X Y^T, the exact-f32
// 128 x 128 Gram tile of pair_tile.h, and q the rows' squared norms. The
// workgroup's own 128 rows are the MFMA's B operand, so an own row sits on a lane (two per lane) and the 32
// accumulator registers of a lane are 32 rows of the current column tile.
//
//   prdc_norms_k    q[u], one wave per row; clears cnt and sets dminx to +inf.
//   prdc_radius_k   same-set tiles only. One workgroup per (row tile of either
//                   set, strip of that set's column tiles). Per own row a sorted
//                   list of kPrdcMaxK registers whose last slot is the current
//                   k-th smallest: slots below 8 - k hold -inf, so one compare
//                   against slot 7 rejects an element whatever k is, and an
//                   insertion is a min/max chain with no index. Self pairs and
//                   rows past the set's end enter as +inf. After the strip the
//                   four (wave row, lane half) holders of an own row merge
//                   through LDS; one list per (strip, row) is written. The
//                   same-set Gram matrix's symmetry is not used: the rows taken
//                   the other way sit across lanes, and a k-list has no
//                   cross-lane merge that is cheaper than the tile itself.
//   prdc_radfold_k  merges a row's strip lists, writes rad.
//   prdc_member_k   cross tiles only, each multiplied once and used both ways.
//                   One workgroup per (real tile, strip of fake tiles). The real
//                   row on the lane counts the fake radii that hold it and keeps
//                   its nearest fake in registers until the strip ends. For the
//                   fake row in an accumulator slot the count over the real rows
//                   is a wave ballot and a population count per lane half; the
//                   minimum is a reduce-scatter over the half's 32 lanes (31
//                   exchanges for 32 slots), after which lane r holds slot r.
//                   Workgroups combine by integer atomics only (add on the
//                   counts, unsigned min on the bits of d2 >= 0), so results do
//                   not depend on their order.
//   prdc_out_k      out[u] = (rad, cnt, dminx) as float32; cnt < 2^15 is exact.
#include "common.h"
#include "pair_tile.h"
#include "prdc.h"

namespace mdt {

namespace {

constexpr float kPrdcInf = __builtin_huge_valf();
constexpr unsigned kPrdcInfBits = 0x7F800000u;

__device__ __forceinline__ const float* prdc_row(const PrdcArgs& a, int u) {
  return u < a.na ? a.real + (size_t)u * a.D : a.fake + (size_t)(u - a.na) * a.D;
}

__global__ __launch_bounds__(kPrdcRowThreads) void prdc_norms_k(PrdcArgs a) {
  const int u = blockIdx.x * (kPrdcRowThreads / kWave) + wave_id();
  if (u >= a.na + a.nb) return;
  const float s = pair_row_norm(prdc_row(a, u), a.D);
  if (lane_id() == 0) {
    a.q[u] = s;
    a.cnt[u] = 0;
    a.dminx[u] = kPrdcInfBits;
  }
}

// A row's k smallest so far in slots [8 - k, 8), ascending; slots below hold -inf.
struct PrdcList {
  float v[kPrdcMaxK];
};

__device__ __forceinline__ void prdc_list_init(PrdcList& l, int k) {
#pragma unroll
  for (int s = 0; s < kPrdcMaxK; ++s) l.v[s] = s < kPrdcMaxK - k ? -kPrdcInf : kPrdcInf;
}

// x < the k-th smallest (slot 7) enters; an equal value would leave the list as it is
__device__ __forceinline__ void prdc_list_insert(PrdcList& l, float x) {
  if (!(x < l.v[kPrdcMaxK - 1])) return;
#pragma unroll
  for (int s = 0; s < kPrdcMaxK; ++s) {
    const float lo = fminf(l.v[s], x);
    x = fmaxf(l.v[s], x);
    l.v[s] = lo;
  }
}

// The k values of another list of the same row (its -inf slots are not values)
__device__ __forceinline__ void prdc_list_merge(PrdcList& l, const float* p, int k) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  const float x[kPrdcMaxK] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
  for (int s = 0; s < kPrdcMaxK; ++s)
    if (s >= kPrdcMaxK - k) prdc_list_insert(l, x[s]);
}

__device__ __forceinline__ void prdc_list_store(const PrdcList& l, float* p) {
  *reinterpret_cast<float4*>(p) = make_float4(l.v[0], l.v[1], l.v[2], l.v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(l.v[4], l.v[5], l.v[6], l.v[7]);
}

template <bool VEC>
__global__ __launch_bounds__(kPairThreads, 2) void prdc_radius_k(PrdcArgs a) {
  // A: the strip's current tile, B: the own tile, [row][kPairLd]; qs: norms of A's rows.
  // After the strip the A | B region carries the four lists of every own row.
  __shared__ __attribute__((aligned(16))) float lds[2 * kPairTile * kPairLd + kPairTile];
  float* As = lds;
  float* Bs = lds + kPairTile * kPairLd;
  float* qs = lds + 2 * kPairTile * kPairLd;

  const int D = a.D, N = a.na + a.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
  // the set this workgroup works in: its rows X [ns, D], at union rows base ..
  const int ta = prdc_tiles(a.na);
  const bool in_real = (int)blockIdx.x < ta;
  const float* X = in_real ? a.real : a.fake;
  const int ns = in_real ? a.na : a.nb, base = in_real ? 0 : a.na;
  const int own0 = (in_real ? blockIdx.x : blockIdx.x - ta) * kPairTile;
  const int tiles = prdc_tiles(ns);
  const int per = (tiles + (int)gridDim.y - 1) / (int)gridDim.y;
  const int c_begin = blockIdx.y * per;
  const int c_end = min(tiles, c_begin + per);

  const int srow = tid >> 3;
  const float* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = own0 + srow + 32 * i;
    pb[i] = u < ns ? X + (size_t)u * D : nullptr;
  }

  int o[2];
  float qo[2];
  PrdcList st[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    o[n] = own0 + wc * 64 + n * 32 + r;
    qo[n] = o[n] < ns ? a.q[base + o[n]] : 0.f;
    prdc_list_init(st[n], a.k);
  }

  for (int ct = c_begin; ct < c_end; ++ct) {
    const int t0 = ct * kPairTile;
    const float* pa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = t0 + srow + 32 * i;
      pa[i] = u < ns ? X + (size_t)u * D : nullptr;
    }
    __syncthreads();  // the previous tile's epilogue has read qs
    if (tid < kPairTile) qs[tid] = t0 + tid < ns ? a.q[base + t0 + tid] : 0.f;

    f32x16 acc[2][2];
    pair_gram128<VEC>(pa, pb, D, As, Bs, tid, acc);

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
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            const float d2 = pair_d2(acc[m][n][4 * g + e], qo[n], qt[e]);
            prdc_list_insert(st[n], t < ns && t != o[n] ? d2 : kPrdcInf);
          }
        }
      }
    }
  }

  // The four holders of an own row, (wave row, lane half): lists through LDS, merged by one thread per row.
  __syncthreads();  // every wave is done with As and Bs
  float* red = lds;  // [4][kPairTile][kPrdcMaxK]
#pragma unroll
  for (int n = 0; n < 2; ++n)
    prdc_list_store(st[n], red + ((size_t)(wr * 2 + h) * kPairTile + wc * 64 + n * 32 + r) * kPrdcMaxK);
  __syncthreads();
  if (tid < kPairTile && own0 + tid < ns) {
    PrdcList l;
    prdc_list_init(l, a.k);
#pragma unroll
    for (int c = 0; c < 4; ++c) prdc_list_merge(l, red + ((size_t)c * kPairTile + tid) * kPrdcMaxK, a.k);
    prdc_list_store(l, a.lists + ((size_t)blockIdx.y * N + base + own0 + tid) * kPrdcMaxK);
  }
}

__global__ __launch_bounds__(kPrdcRowThreads) void prdc_radfold_k(PrdcArgs a) {
  const int N = a.na + a.nb;
  const int u = blockIdx.x * kPrdcRowThreads + threadIdx.x;
  if (u >= N) return;
  PrdcList l;
  prdc_list_init(l, a.k);
  for (int s = 0; s < a.strips; ++s) prdc_list_merge(l, a.lists + ((size_t)s * N + u) * kPrdcMaxK, a.k);
  a.rad[u] = l.v[kPrdcMaxK - 1];
}

// Lower the stored minimum of row u to d2 (>= 0, or +inf); the plain read only spares atomics
__device__ __forceinline__ void prdc_min_to(unsigned* p, float d2) {
  const unsigned bits = __float_as_uint(d2);
  if (bits < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, bits);
}

template <bool VEC>
__global__ __launch_bounds__(kPairThreads, 2) void prdc_member_k(PrdcArgs a) {
  // A: the strip's current fake tile, B: the own real tile; qs, rs: norms and radii of A's rows
  __shared__ __attribute__((aligned(16))) float lds[2 * kPairTile * kPairLd + 2 * kPairTile];
  float* As = lds;
  float* Bs = lds + kPairTile * kPairLd;
  float* qs = lds + 2 * kPairTile * kPairLd;
  float* rs = qs + kPairTile;

  const int D = a.D, na = a.na, nb = a.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
  const int own0 = blockIdx.x * kPairTile;
  const int tiles = prdc_tiles(nb);
  const int per = (tiles + (int)gridDim.y - 1) / (int)gridDim.y;
  const int c_begin = blockIdx.y * per;
  const int c_end = min(tiles, c_begin + per);

  const int srow = tid >> 3;
  const float* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int u = own0 + srow + 32 * i;
    pb[i] = u < na ? a.real + (size_t)u * D : nullptr;
  }

  int o[2], cnt_o[2];
  bool vo[2];
  float qo[2], ro[2], dmin_o[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    o[n] = own0 + wc * 64 + n * 32 + r;
    vo[n] = o[n] < na;
    qo[n] = vo[n] ? a.q[o[n]] : 0.f;
    ro[n] = vo[n] ? a.rad[o[n]] : 0.f;
    cnt_o[n] = 0;
    dmin_o[n] = kPrdcInf;
  }

  for (int ct = c_begin; ct < c_end; ++ct) {
    const int t0 = ct * kPairTile;
    const float* pa[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = t0 + srow + 32 * i;
      pa[i] = u < nb ? a.fake + (size_t)u * D : nullptr;
    }
    __syncthreads();  // the previous tile's epilogue has read qs and rs
    if (tid < kPairTile) {
      const bool v = t0 + tid < nb;
      qs[tid] = v ? a.q[na + t0 + tid] : 0.f;
      rs[tid] = v ? a.rad[na + t0 + tid] : 0.f;
    }

    f32x16 acc[2][2];
    pair_gram128<VEC>(pa, pb, D, As, Bs, tid, acc);

    float mv[32];  // per accumulator slot 16 m + reg: the nearest of this lane's two real rows
    int keepc = 0;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int tl = wr * 64 + m * 32 + 8 * g + 4 * h;
        const float4 q4 = *reinterpret_cast<const float4*>(qs + tl);
        const float4 r4 = *reinterpret_cast<const float4*>(rs + tl);
        const float qt[4] = {q4.x, q4.y, q4.z, q4.w};
        const float rt[4] = {r4.x, r4.y, r4.z, r4.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool vt = t0 + tl + e < nb;
          float d[2];
          int c_lo = 0, c_hi = 0;
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            d[n] = pair_d2(acc[m][n][4 * g + e], qo[n], qt[e]);
            // the real row on the lane against the fake row's radius
            cnt_o[n] += vt && d[n] <= rt[e] ? 1 : 0;
            dmin_o[n] = fminf(dmin_o[n], vt ? d[n] : kPrdcInf);
            // the fake row of the slot against the radii of the real rows on the lanes: lane half h holds
            // row tl + e of its own, so the two halves of the ballot are two rows' counts
            const unsigned long long in = __ballot(vo[n] && d[n] <= ro[n]);
            c_lo += __popc((unsigned)in);
            c_hi += __popc((unsigned)(in >> 32));
          }
          if (r == 16 * m + 4 * g + e) keepc = h ? c_hi : c_lo;
          mv[16 * m + 4 * g + e] = fminf(vo[0] ? d[0] : kPrdcInf, vo[1] ? d[1] : kPrdcInf);
        }
        // the scheduler's window: four slots' compares, ballots and counts at a time
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // reduce-scatter of the 32 slots over the 32 lanes of a half: at distance off a lane keeps the
    // slots whose bit `off` equals its own and takes the partner's minima of them; lane r ends with slot r
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
      const bool up = (r & off) != 0;
#pragma unroll
      for (int i = 0; i < off; ++i) {
        const float lo = mv[i], hi = mv[i + off];
        mv[i] = fminf(up ? hi : lo, __shfl_xor(up ? lo : hi, off, 64));
      }
    }
    {  // lane (r, h) holds slot (m, reg) = (r >> 4, r & 15): row 32 m + 8 (reg >> 2) + 4 h + (reg & 3) of its wave's 64
      const int t = t0 + wr * 64 + (r >> 4) * 32 + 8 * ((r & 15) >> 2) + 4 * h + (r & 3);
      if (t < nb) {
        if (keepc) atomicAdd(a.cnt + na + t, keepc);
        prdc_min_to(a.dminx + na + t, mv[0]);
      }
    }
  }

  // The two lane halves that share a real row, then every holder straight to the row's words
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    cnt_o[n] += __shfl_xor(cnt_o[n], 32, 64);
    dmin_o[n] = fminf(dmin_o[n], __shfl_xor(dmin_o[n], 32, 64));
    if (h == 0 && vo[n]) {
      if (cnt_o[n]) atomicAdd(a.cnt + o[n], cnt_o[n]);
      prdc_min_to(a.dminx + o[n], dmin_o[n]);
    }
  }
}

__global__ __launch_bounds__(kPrdcRowThreads) void prdc_out_k(PrdcArgs a) {
  const int u = blockIdx.x * kPrdcRowThreads + threadIdx.x;
  if (u >= a.na + a.nb) return;
  float* dst = a.out + (size_t)u * kPrdcCols;
  dst[0] = a.rad[u];
  dst[1] = (float)a.cnt[u];
  dst[2] = __uint_as_float(a.dminx[u]);
}

}  // namespace

}  // namespace mdt

extern "C" int mdt_prdc_check(const mdt::PrdcArgs* a) {
  using namespace mdt;
  if (a->k < 1 || a->k > kPrdcMaxK) return 4;
  if (a->na <= a->k || a->na > kPrdcMaxRows || a->nb <= a->k || a->nb > kPrdcMaxRows) return 1;
  if (a->D < 1 || a->D > kPrdcMaxD) return 2;
  if (a->strips != prdc_strips(a->na, a->nb)) return 3;
  if (!a->real || !a->fake || !a->q || !a->rad || !a->cnt || !a->dminx || !a->lists || !a->out) return 5;
  return 0;
}

extern "C" int mdt_prdc_rows(const mdt::PrdcArgs* a, hipStream_t s) {
  using namespace mdt;
  const int rc = mdt_prdc_check(a);
  if (rc) return rc;
  const int N = a->na + a->nb;
  const int ta = prdc_tiles(a->na), tb = prdc_tiles(a->nb);
  const dim3 rows((unsigned)prdc_cdiv(N, kPrdcRowThreads)), tile(kPairThreads);
  hipLaunchKernelGGL(prdc_norms_k, dim3((unsigned)prdc_cdiv(N, kPrdcRowThreads / kWave)), dim3(kPrdcRowThreads), 0, s, *a);
  const bool vec = a->D % 4 == 0 && (reinterpret_cast<uintptr_t>(a->real) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a->fake) & 15) == 0;
  const dim3 rgrid((unsigned)(ta + tb), (unsigned)a->strips), mgrid((unsigned)ta, (unsigned)a->strips);
  if (vec) hipLaunchKernelGGL(prdc_radius_k<true>, rgrid, tile, 0, s, *a);
  else hipLaunchKernelGGL(prdc_radius_k<false>, rgrid, tile, 0, s, *a);
  hipLaunchKernelGGL(prdc_radfold_k, rows, dim3(kPrdcRowThreads), 0, s, *a);
  if (vec) hipLaunchKernelGGL(prdc_member_k<true>, mgrid, tile, 0, s, *a);
  else hipLaunchKernelGGL(prdc_member_k<false>, mgrid, tile, 0, s, *a);
  hipLaunchKernelGGL(prdc_out_k, rows, dim3(kPrdcRowThreads), 0, s, *a);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}
