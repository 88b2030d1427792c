// The 128 x 128 exact-f32 Gram tile of the sample scores' pair kernels (ts_pair_k,
// prdc_radius_k, prdc_member_k, sk_cost_k) and what their neighbours share with it.
//
// acc = A B^T of two 128-row operand tiles on the MFMA 32x32x2 (a k-ordered fma chain
// per element, so inputs whose products and partial sums are exact give exact results):
// 256 threads, 2 x 2 MFMA tiles per wave (wave (wr, wc) = (wave >> 1, wave & 1) takes
// rows wr * 64 .. of A against rows wc * 64 .. of B), K in LDS chunks of kPairBK at row
// stride kPairLd with the tail of D zero-filled, the next chunk's global loads in flight
// under the current chunk's MFMAs. Accumulator register reg of lane (r, h) = (lane & 31,
// lane >> 5) in acc[m][n] is row 32 m + (reg & 3) + 8 (reg >> 2) + 4 h of the wave's 64
// rows of A against row 32 n + r of its 64 rows of B.
//
// The constants are plain C++ (the host-side layouts read kPairTile); the device part
// needs the HIP compiler.
#pragma once

namespace mdt {

constexpr int kPairTile = 128;         // rows per operand tile
constexpr int kPairBK = 32;            // k per LDS chunk
constexpr int kPairLd = kPairBK + 4;   // LDS row stride (floats): 16-lane groups of a 16-byte read hit 16 slots
constexpr int kPairThreads = 256;

}  // namespace mdt

#ifdef __HIPCC__
#include "common.h"

namespace mdt {

// Four consecutive k of one row, zero past the row's end (and for a null row: one past the operand's end)
template <bool VEC>
__device__ __forceinline__ float4 pair_load4(const float* p, int k, int D) {
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

// The squared norm of row p[0 .. D), by one whole wave: a lane's fma chain over its k, then the wave's tree
__device__ __forceinline__ float pair_row_norm(const float* p, int D) {
  float s = 0.f;
  for (int k = lane_id(); k < D; k += kWave) s = fmaf(p[k], p[k], s);
  return wave_sum(s);
}

// The squared distance of two rows from their Gram element and squared norms
__device__ __forceinline__ float pair_d2(float acc, float qi, float qj) { return fmaxf(0.f, fmaf(-2.f, acc, qi + qj)); }

// acc = A B^T of the two staged 128-row tiles. pa / pb: this thread's four rows
// of each (rows srow + 32 i, four k at sk of a chunk), null past the set's end.
// Enters through a barrier (LDS readers of the previous tile are done) and
// leaves with the last chunk's fragments read by this wave only.
template <bool VEC>
__device__ __forceinline__ void pair_gram128(const float* const (&pa)[4], const float* const (&pb)[4], int D, float* As,
                                             float* Bs, int tid, f32x16 (&acc)[2][2]) {
  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, r = lane & 31, h = lane >> 5;
  const int srow = tid >> 3, sk = (tid & 7) * 4;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[m][n][e] = 0.f;
  float4 ra[4], rb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = pair_load4<VEC>(pa[i], sk, D);
    rb[i] = pair_load4<VEC>(pb[i], sk, D);
  }
  for (int k0 = 0; k0 < D; k0 += kPairBK) {
    __syncthreads();  // the previous chunk's fragments are read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<float4*>(As + (srow + 32 * i) * kPairLd + sk) = ra[i];
      *reinterpret_cast<float4*>(Bs + (srow + 32 * i) * kPairLd + sk) = rb[i];
    }
    __syncthreads();
    if (k0 + kPairBK < D) {  // the next chunk's loads fly under this chunk's MFMAs
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = pair_load4<VEC>(pa[i], k0 + kPairBK + sk, D);
        rb[i] = pair_load4<VEC>(pb[i], k0 + kPairBK + sk, D);
      }
    }
    // lane half h takes k = 8 c + 4 h + j of the chunk in MFMA step (c, j), from both
    // operands alike: one 16-byte read feeds four steps
#pragma unroll
    for (int c = 0; c < kPairBK / 8; ++c) {
      float4 av[2], bv[2];
#pragma unroll
      for (int m = 0; m < 2; ++m)
        av[m] = *reinterpret_cast<const float4*>(As + (wr * 64 + m * 32 + r) * kPairLd + 8 * c + 4 * h);
#pragma unroll
      for (int n = 0; n < 2; ++n)
        bv[n] = *reinterpret_cast<const float4*>(Bs + (wc * 64 + n * 32 + r) * kPairLd + 8 * c + 4 * h);
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
}

}  // namespace mdt
#endif  // __HIPCC__
