// Lloyd's k-means (models/ndb.py) on rows x [n, D] with K <= 256 centroids,
// float32 throughout: three launches per iteration, no [n, K] distance matrix
// and no atomics.
//
//   kmeans_assign_k  one workgroup of four waves per band of 64 or 32 rows
//                    (km_band: 32 while 64-row bands would leave compute units
//                    idle) against every centroid, the count padded to 32-wide
//                    MFMA tiles. S = X C^T runs on the exact-f32 MFMA 32x32x2
//                    with the accumulators in registers: a wave owns one 32-row
//                    tile of the band and every WC-th column tile (at most 4
//                    accumulators, 64 registers). D goes through LDS in chunks
//                    of 32, two buffers: the next chunk's global loads are
//                    issued before the current chunk's MFMAs and stored after
//                    them, one barrier a chunk, so X is read from HBM once an
//                    iteration and the centroids come from L2. The tail of D
//                    and rows past n are zero-filled in the staging loads
//                    (16-byte loads when D % 4 == 0, scalar ones otherwise).
//                    The thread that stages a row's four floats also squares
//                    them: |x|^2 needs no pass of its own. Epilogue: the score
//                    c2[k] - 2 S[i, k] (a padded column scores +inf), the
//                    minimum over a lane's columns, over the 32 lanes of a row
//                    by shuffles and over the waves through LDS, the lowest k
//                    winning every tie; label, mind = max(0, x2 + min) and the
//                    band's count of changed labels.
//   kmeans_update_k  grid (64-column slabs of D, row splits of 1024 rows). The
//                    label-segmented column sums are an MFMA whose k dimension
//                    is the rows: the A operand is the one-hot of the labels,
//                    made in registers (lane (m, kk) holds label[row kk] == m),
//                    the B operand is X as it lies in memory (a half wave loads
//                    32 consecutive floats of one row). A product is exact, so
//                    a sum is one f32 chain over the split's rows in order.
//                    Wave w owns the cells of the 32-cell tiles w and w + 4.
//                    The labels of the split sit in LDS; slab 0 also counts
//                    them per cell.
//   kmeans_fold_k    grid (K, 2048-column segments). Sums the splits' partials
//                    in split order, divides by the count (0: the centroid
//                    stays as it is, bit for bit) and leaves the segment's part
//                    of |c|^2. With other flags it gathers the starting
//                    centroids from their rows; workgroup (0, 0) adds the
//                    bands' changed-label counts, or sums mind over the real
//                    rows in double in a fixed order.
//
// Every sum has one order and no workgroup waits for another: a fit repeats
// bitwise.
#include "common.h"
#include "pair_tile.h"
#include "kmeans.h"

namespace mdt {

namespace {

enum : int { kKmGather = 1, kKmFold = 2, kKmC2 = 4, kKmMoved = 8, kKmInertia = 16 };

constexpr float kKmInf = __builtin_huge_valf();
constexpr int kKmNone = 0x7fffffff;

// the better of two (score, cell): the lower score, the lower cell on a tie
__device__ __forceinline__ void km_better(float& v, int& i, float ov, int oi) {
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}

// rows [0, n0) are a.real's, rows [n0, n0 + n1) a.fake's
template <int BM, bool VEC>
__global__ __launch_bounds__(kKmThreads) void kmeans_assign_k(KmeansArgs a, int n0, int n1, int prev) {
  constexpr int RT = BM / 32;   // row tiles of the band
  constexpr int WC = 4 / RT;    // waves that share a row tile, each with every WC-th column tile
  constexpr int NT = 8 / WC;    // column tiles of a wave at K = 256
  extern __shared__ __attribute__((aligned(16))) float km_lds[];
  __shared__ float x2s[BM];
  __shared__ float wv[WC][BM];
  __shared__ int wi[WC][BM];

  const int D = a.D, K = a.K, n = n0 + n1, kt = km_kpad(K) >> 5, segs = km_segs(D);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int rt = wave % RT, cw = wave / RT;
  const int row0 = blockIdx.x * BM;
  const int buf = (BM + (kt << 5)) * kKmLd;  // floats per buffer: the band's rows, then the centroids

  // staging: thread -> rows srow + 32 i of the band and of the centroids, four columns at sk of the chunk
  const int srow = tid >> 3, sk = (tid & 7) * 4;
  const float* px[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int g = row0 + srow + 32 * i;
    px[i] = g >= n ? nullptr : g < n0 ? a.real + (size_t)g * D : a.fake + (size_t)(g - n0) * D;
  }
  const float* pc = a.cent + (size_t)srow * D;  // row srow + 32 i: pc + 32 i D, while that row is below K

  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  float4 rx[RT], rc[8];
  float x2p[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) x2p[i] = 0.f;

  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      rx[i] = pair_load4<VEC>(px[i], k0 + sk, D);
      x2p[i] = fmaf(rx[i].x, rx[i].x, x2p[i]);
      x2p[i] = fmaf(rx[i].y, rx[i].y, x2p[i]);
      x2p[i] = fmaf(rx[i].z, rx[i].z, x2p[i]);
      x2p[i] = fmaf(rx[i].w, rx[i].w, x2p[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < kt) rc[i] = pair_load4<VEC>(srow + 32 * i < K ? pc + (size_t)(32 * i) * D : nullptr, k0 + sk, D);
  };
  auto store = [&](float* dst) {
#pragma unroll
    for (int i = 0; i < RT; ++i) *reinterpret_cast<float4*>(dst + (srow + 32 * i) * kKmLd + sk) = rx[i];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (i < kt) *reinterpret_cast<float4*>(dst + (BM + srow + 32 * i) * kKmLd + sk) = rc[i];
  };

  load(0);
  store(km_lds);
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < D; k0 += kKmBK, cur ^= 1) {
    const bool more = k0 + kKmBK < D;
    if (more) load(k0 + kKmBK);  // in flight under this chunk's MFMAs
    const float* Xs = km_lds + cur * buf;
    const float* Cs = Xs + BM * kKmLd;
    // lane half h takes column 8 c + 4 h + q of the chunk in MFMA step (c, q), from both operands alike
#pragma unroll
    for (int c = 0; c < kKmBK / 8; ++c) {
      const float4 av = *reinterpret_cast<const float4*>(Xs + (rt * 32 + r) * kKmLd + 8 * c + 4 * h);
      const float af[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
      for (int j = 0; j < NT; ++j)
        if (cw + WC * j < kt) {
          const float4 bv = *reinterpret_cast<const float4*>(Cs + ((cw + WC * j) * 32 + r) * kKmLd + 8 * c + 4 * h);
          const float bf[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[j] = mfma32x32x2(af[q], bf[q], acc[j]);
        }
    }
    if (more) store(km_lds + (cur ^ 1) * buf);  // the buffer every wave left at the previous barrier
    __syncthreads();
  }

  // |x|^2 of a staged row: its eight threads are neighbours in one wave
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    float s = x2p[i];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if ((tid & 7) == 0) x2s[srow + 32 * i] = s;
  }

  // accumulator register reg of lane (r, h): row (reg & 3) + 8 (reg >> 2) + 4 h of the wave's 32, column
  // 32 (cw + WC j) + r
  float c2v[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int col = (cw + WC * j) * 32 + r;
    c2v[j] = kKmInf;
    if (col < K) {
      const float* c2 = a.ws + km_layout(a.na, a.nb, D, K).c2 + (size_t)col * segs;
      float s = c2[0];
      for (int g = 1; g < segs; ++g) s += c2[g];
      c2v[j] = s;
    }
  }
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    float bv = kKmInf;
    int bi = kKmNone;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = (cw + WC * j) * 32 + r;
      if (col < K) km_better(bv, bi, fmaf(-2.f, acc[j][reg], c2v[j]), col);
    }
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      km_better(bv, bi, ov, oi);
    }
    if (r == 0) {
      const int rl = rt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      wv[cw][rl] = bv;
      wi[cw][rl] = bi;
    }
  }
  __syncthreads();

  if (tid < 64) {  // wave 0: a thread per row of the band
    bool changed = false;
    const int g = row0 + tid;
    if (tid < BM && g < n) {
      float bv = wv[0][tid];
      int bi = wi[0][tid];
#pragma unroll
      for (int w = 1; w < WC; ++w) km_better(bv, bi, wv[w][tid], wi[w][tid]);
      if (bi >= K) bi = 0;  // only a row with a NaN has no finite score
      changed = !prev || a.labels[g] != bi;
      a.labels[g] = bi;
      a.mind[g] = fmaxf(0.f, x2s[tid] + bv);
    }
    const unsigned long long m = __ballot(changed);
    if (tid == 0) reinterpret_cast<int*>(a.ws + km_layout(a.na, a.nb, D, K).band)[blockIdx.x] = __popcll(m);
  }
}

__global__ __launch_bounds__(kKmThreads) void kmeans_update_k(KmeansArgs a) {
  __shared__ int lab[kKmSplitRows];
  constexpr int U = 8;  // MFMA steps (pairs of rows) whose loads are in flight together
  const int D = a.D, K = a.K, kt = km_kpad(K) >> 5;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int split = blockIdx.y, rbeg = split * kKmSplitRows, rend = min(a.na, rbeg + kKmSplitRows);
  const KmLayout L = km_layout(a.na, a.nb, D, K);

  for (int e = tid; e < kKmSplitRows; e += kKmThreads) lab[e] = rbeg + e < rend ? a.labels[rbeg + e] : -1;
  __syncthreads();
  if (blockIdx.x == 0) {  // kKmThreads == kKmMaxK: a thread per cell
    int c = 0;
    for (int e = 0; e < rend - rbeg; ++e) c += lab[e] == tid ? 1 : 0;
    reinterpret_cast<int*>(a.ws + L.cnt)[split * kKmMaxK + tid] = c;
  }
  if (wave >= kt) return;

  const int col0 = blockIdx.x * kKmSlab + r, col1 = col0 + 32;
  const bool ok0 = col0 < D, ok1 = col1 < D, two = wave + 4 < kt;
  const int m0 = wave * 32 + r, m1 = m0 + 128;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // lane (r, h) of a step holds row base + h: its label for the A operand, columns col0 and col1 for B
  for (int base = rbeg; base < rend; base += 2 * U) {
    float b0[U], b1[U];
    int lb[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int g = base + 2 * u + h;
      const bool ok = g < rend;
      const float* p = a.real + (size_t)g * D;
      b0[u] = ok && ok0 ? p[col0] : 0.f;
      b1[u] = ok && ok1 ? p[col1] : 0.f;
      lb[u] = ok ? lab[g - rbeg] : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float h0 = lb[u] == m0 ? 1.f : 0.f;
      acc[0][0] = mfma32x32x2(h0, b0[u], acc[0][0]);
      acc[0][1] = mfma32x32x2(h0, b1[u], acc[0][1]);
      if (two) {
        const float h1 = lb[u] == m1 ? 1.f : 0.f;
        acc[1][0] = mfma32x32x2(h1, b0[u], acc[1][0]);
        acc[1][1] = mfma32x32x2(h1, b1[u], acc[1][1]);
      }
    }
  }

  float* part = a.ws + L.part + (size_t)split * K * D;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int m = wave * 32 + i * 128 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
      if (m < K && (i == 0 || two)) {
        if (ok0) part[(size_t)m * D + col0] = acc[i][0][reg];
        if (ok1) part[(size_t)m * D + col1] = acc[i][1][reg];
      }
    }
}

__global__ __launch_bounds__(kKmThreads) void kmeans_fold_k(KmeansArgs a, int flags, int t, int nbands) {
  __shared__ float scratch[16];
  __shared__ double red[kKmThreads];
  const int D = a.D, K = a.K, tid = threadIdx.x;
  const KmLayout L = km_layout(a.na, a.nb, D, K);

  if (flags & kKmC2) {
    const int k = blockIdx.x, seg = blockIdx.y, R = km_splits(a.na), segs = km_segs(D);
    int count = 0;
    if (flags & kKmFold) {
      const int* cnt = reinterpret_cast<const int*>(a.ws + L.cnt);
      for (int s = 0; s < R; ++s) count += cnt[s * kKmMaxK + k];
      if (a.counts != nullptr && seg == 0 && tid == 0) a.counts[k] = count;
    }
    const float* src = (flags & kKmGather) ? a.real + (size_t)a.init[k] * D : nullptr;
    float* c = a.cent + (size_t)k * D;
    float s2 = 0.f;
    for (int col = seg * kKmFoldCols + tid; col < min(D, (seg + 1) * kKmFoldCols); col += kKmThreads) {
      float v;
      if (src != nullptr) {
        c[col] = v = src[col];
      } else if (count > 0) {
        const float* p = a.ws + L.part + (size_t)k * D + col;
        float s = 0.f;
        for (int q = 0; q < R; ++q) s += p[(size_t)q * K * D];
        c[col] = v = s / (float)count;
      } else {
        v = c[col];
      }
      s2 = fmaf(v, v, s2);
    }
    s2 = block_sum(s2, scratch);
    if (tid == 0) a.ws[L.c2 + (size_t)k * segs + seg] = s2;
  }
  if (blockIdx.x != 0 || blockIdx.y != 0) return;  // block-uniform

  if (flags & kKmMoved) {
    const int* band = reinterpret_cast<const int*>(a.ws + L.band);
    int s = 0;
    for (int b = tid; b < nbands; b += kKmThreads) s += band[b];
    red[tid] = (double)s;  // exact: at most 2^17 rows
  } else if (flags & kKmInertia) {
    double s = 0.0;
    for (int i = tid; i < a.na; i += kKmThreads) s += (double)a.mind[i];
    red[tid] = s;
  } else {
    return;
  }
  __syncthreads();
  for (int o = kKmThreads / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    if (flags & kKmMoved) a.moved[t] = (int)red[0];
    else a.inertia[0] = red[0];
  }
}

int km_sizes(const KmeansArgs* a) {
  if (a->na < 2 || a->na > kKmMaxRows || a->nb < 0 || a->nb == 1 || a->nb > kKmMaxRows) return 1;
  if (a->D < 1 || a->D > kKmMaxD) return 2;
  if (a->K < 2 || a->K > kKmMaxK) return 3;
  return 0;
}

bool km_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int BM, bool VEC>
bool km_assign_launch(const KmeansArgs& a, int n0, int n1, int prev, hipStream_t s) {
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&kmeans_assign_k<BM, VEC>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)km_assign_lds(BM, kKmMaxK));
  if (attr != hipSuccess) return false;
  hipLaunchKernelGGL((kmeans_assign_k<BM, VEC>), dim3((unsigned)km_cdiv(n0 + n1, BM)), dim3(kKmThreads),
                     km_assign_lds(BM, km_kpad(a.K)), s, a, n0, n1, prev);
  return true;
}

// -> the bands of the launch, or 0 when it could not be made
int km_assign(const KmeansArgs& a, int n0, int n1, int prev, hipStream_t s) {
  const bool vec = a.D % 4 == 0;
  const int bm = km_band(n0 + n1);
  const bool ok = bm == 64 ? (vec ? km_assign_launch<64, true>(a, n0, n1, prev, s) : km_assign_launch<64, false>(a, n0, n1, prev, s))
                           : (vec ? km_assign_launch<32, true>(a, n0, n1, prev, s) : km_assign_launch<32, false>(a, n0, n1, prev, s));
  return ok ? km_bands(n0 + n1) : 0;
}

void km_update(const KmeansArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(kmeans_update_k, dim3((unsigned)km_cdiv(a.D, kKmSlab), (unsigned)km_splits(a.na)), dim3(kKmThreads), 0,
                     s, a);
}

void km_fold(const KmeansArgs& a, int flags, int t, int nbands, hipStream_t s) {
  const dim3 grid = (flags & kKmC2) ? dim3((unsigned)a.K, (unsigned)km_segs(a.D)) : dim3(1, 1);
  hipLaunchKernelGGL(kmeans_fold_k, grid, dim3(kKmThreads), 0, s, a, flags, t, nbands);
}

bool km_ok() { return hipGetLastError() == hipSuccess; }

}  // namespace

}  // namespace mdt

extern "C" int mdt_kmeans_check(const mdt::KmeansArgs* a) {
  using namespace mdt;
  const int rc = km_sizes(a);
  if (rc) return rc;
  if (!a->real || !a->ws || !a->cent || !a->labels || (a->nb > 0 && !a->fake)) return 5;
  return km_aligned(a->real) && km_aligned(a->ws) && km_aligned(a->cent) && (a->nb == 0 || km_aligned(a->fake)) ? 0 : 5;
}

extern "C" int mdt_kmeans_rows(const mdt::KmeansArgs* a, hipStream_t s) {
  using namespace mdt;
  const int rc = mdt_kmeans_check(a);
  if (rc) return rc;
  if (a->K > a->na) return 3;  // the starting centroids are distinct real rows
  if (a->T < 1 || a->T > kKmMaxIters) return 4;
  if (!a->init || !a->mind || !a->moved || !a->inertia) return 5;
  KmeansArgs b = *a;
  b.counts = nullptr;
  km_fold(b, kKmGather | kKmC2, 0, 0, s);
  for (int t = 0; t < b.T; ++t) {
    const int bands = km_assign(b, b.na, 0, t > 0, s);
    if (!bands) return 9;
    km_update(b, s);
    km_fold(b, kKmFold | kKmC2 | kKmMoved, t, bands, s);
  }
  if (!km_assign(b, b.na, b.nb, 0, s)) return 9;
  km_fold(b, kKmInertia, 0, 0, s);
  return km_ok() ? 0 : 9;
}

extern "C" int mdt_kmeans_assign(const mdt::KmeansArgs* a, int prev, hipStream_t s) {
  using namespace mdt;
  const int rc = mdt_kmeans_check(a);
  if (rc) return rc;
  if (!a->mind || !a->moved) return 5;
  km_fold(*a, kKmC2, 0, 0, s);
  const int bands = km_assign(*a, a->na, a->nb, prev, s);
  if (!bands) return 9;
  km_fold(*a, kKmMoved, 0, bands, s);
  return km_ok() ? 0 : 9;
}

extern "C" int mdt_kmeans_update(const mdt::KmeansArgs* a, hipStream_t s) {
  using namespace mdt;
  const int rc = mdt_kmeans_check(a);
  if (rc) return rc;
  if (!a->counts) return 5;
  km_update(*a, s);
  km_fold(*a, kKmFold | kKmC2, 0, 0, s);
  return km_ok() ? 0 : 9;
}
