// Reconstruction report (see recon.hip): per row of real | recon [n, S*S] the
// squared error and the SSIM of the pair with its luminance and contrast-
// structure means, on the 11x11 Gaussian window at the (S - 10)^2 valid
// positions. models/recon_report.py is the definition.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mdt {

constexpr int kReconCols = 4;          // a table row: se, ssim, l, cs
constexpr int kReconWin = 11;          // taps of the window, sigma 1.5
constexpr int kReconMinSide = kReconWin;
constexpr int kReconMaxSide = 256;
constexpr int kReconMaxRows = 1 << 20;
constexpr int kReconMaps = 5;          // x, r, x^2, r^2, x r (of the values shifted by -0.5)
constexpr int kReconRun = 6;           // output columns a lane filters in one horizontal run
constexpr int kReconWaveSide = 32;     // up to here one wavefront owns one image
constexpr int kReconWaves = 4;         // images per workgroup of the wave kernel
constexpr int kReconThreads = 256;     // workgroup of the band kernel
constexpr int kReconLds2 = 80 * 1024;  // a band's LDS with two workgroups per CU
constexpr int kReconLds1 = 160 * 1024; // ... with one, for sides whose bands would fall below kReconMinBand
constexpr int kReconMinBand = 12;

// LDS row strides (floats) of the staged inputs and of a filtered map: odd, so
// lanes that walk down a column hit distinct banks.
__host__ __device__ inline int recon_in_ld(int S) { return S | 1; }
__host__ __device__ inline int recon_map_ld(int S) { return (S - (kReconWin - 1)) | 1; }
// floats of LDS for `rows` input rows: both images and the five filtered maps
__host__ __device__ inline int recon_lds_floats(int S, int rows) {
  return rows * (2 * recon_in_ld(S) + kReconMaps * recon_map_ld(S));
}
// Output rows of one band: a function of S alone. Sides up to kReconWaveSide: all of them.
__host__ __device__ inline int recon_band_rows(int S) {
  const int H = S - (kReconWin - 1), row = recon_lds_floats(S, 1) * 4;
  int R = kReconLds2 / row - (kReconWin - 1);
  if (R < kReconMinBand) R = kReconLds1 / row - (kReconWin - 1);
  return S <= kReconWaveSide || R > H ? H : R;
}
__host__ __device__ inline int recon_bands(int S) {
  const int H = S - (kReconWin - 1), R = recon_band_rows(S);
  return (H + R - 1) / R;
}

struct ReconArgs {
  int n, side, bands;
  const float* real;   // [n, S*S]
  const float* recon;  // [n, S*S]
  float* partial;      // [n][bands][kReconCols] band sums (sides above kReconWaveSide)
  float* table;        // [n][kReconCols]
};

}  // namespace mdt

extern "C" {
// 0, or why not: 1 n outside [1, 2^20], 2 side outside [11, 256], 3 bands != recon_bands(side), 4 missing buffer
int mdt_recon_check(const mdt::ReconArgs* a);
// sides up to 32: one launch (a wavefront per image); above: the band kernel over (image, band), then the fold
int mdt_recon_rows(const mdt::ReconArgs* a, hipStream_t s);
}
