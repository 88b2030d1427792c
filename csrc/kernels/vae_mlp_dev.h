// Device helpers shared by the MLP-VAE kernels (vae_mlp.hip, vae_iw.hip).
#pragma once
#include "common.h"

namespace mdt {

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;

__device__ __forceinline__ int cdiv_d(int a, int b) { return (a + b - 1) / b; }

// Slab geometry: TH = H/16 slices; [mu|lv] slabs are NTM = ceil(2Z/16) tiles
// wide (SW floats), dz slabs NTZ = ceil(Z/16) tiles (SWZ floats). F2/B2 run
// GROUPS = ceil(TH/8) blocks per row tile, one 16-column output tile per wave.
struct SlabGeo {
  int th, ntm, sw, ntz, swz, groups;
  __device__ __host__ SlabGeo(int H, int Z)
      : th((H + 15) / 16), ntm((2 * Z + 15) / 16), sw(((2 * Z + 15) / 16) * 16), ntz((Z + 15) / 16),
        swz(((Z + 15) / 16) * 16), groups(((H + 15) / 16 + kWaves - 1) / kWaves) {}
};

// Transposes a 16x16 C-layout tile (wave 0's registers: col = lane&15,
// rows 4q..4q+3) into an LDS [row][k] image readable as A fragments.
__device__ __forceinline__ void tile_to_lds(float (*t)[20], const float (&v)[4]) {
  const int lane = lane_id();
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) t[4 * (lane >> 4) + rr][lane & 15] = v[rr];
}

// 16x16 MFMA with A from the LDS tile (k = 16) and a prefetched B fragment.
__device__ __forceinline__ f32x4 lds_tile_mma(float (*t)[20], const float (&b)[4]) {
  const int lane = lane_id();
  const float4 av = *reinterpret_cast<const float4*>(&t[lane & 15][4 * (lane >> 4)]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = mfma16x16x4(av.x, b[0], acc);
  acc = mfma16x16x4(av.y, b[1], acc);
  acc = mfma16x16x4(av.z, b[2], acc);
  acc = mfma16x16x4(av.w, b[3], acc);
  return acc;
}

}  // namespace mdt
