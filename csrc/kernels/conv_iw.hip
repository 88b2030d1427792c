// Conv-VAE side of the importance-weighted log-likelihood pass (vae_iw.hip has
// the definitions and the shared reduce kernel). The encoder and the decoder
// run on the existing layer kernels; these two small kernels sit around the
// decoder: the K-sample reparameterisation (+ prior term) in front of it and
// the per-row BCE behind it. Virtual row v = s*M + i (sample s of the chunk,
// batch row i); a chunk has at most B virtual rows, the decoder's batch size.
#include "common.h"
#include "vae_iw.h"

namespace mdt {

constexpr int kIwMaxZ = 256;

// One 64-thread workgroup per virtual row: eps (Philox counter (k*B + i)*Z + c,
// stream kIwStream, step = 0-based batch index), z = mu + eps*exp(lv/2) as
// bf16 (the decoder's input) and f32, and sum_c(-z^2/2 + eps^2/2 + lv/2) from
// the unrounded z, summed in latent order by one thread.
__global__ void __launch_bounds__(64) iw_reparam_k(const float* mulv, int M, int B, int Z, int k0, int S,
                                                   const IwState* ist, const HParams* hp, __bf16* z16, float* z32,
                                                   float* eps, float* prior) {
  __shared__ float term[kIwMaxZ];
  const int v = blockIdx.x;
  if (v >= S * M) return;
  const int s = v / M, i = v - s * M;
  const long long stp = ist->st.step - 1;
  const uint32_t step_lo = (uint32_t)((unsigned long long)stp & 0xffffffffu);
  const uint32_t step_hi = (uint32_t)((unsigned long long)stp >> 32);
  for (int c = threadIdx.x; c < Z; c += 64) {
    const float mu = mulv[(size_t)i * 2 * Z + c], lv = mulv[(size_t)i * 2 * Z + Z + c];
    const uint32_t ctr = ((uint32_t)(k0 + s) * (uint32_t)B + (uint32_t)i) * (uint32_t)Z + (uint32_t)c;
    const u32x4 bits = philox4x32_10(u32x4{ctr, kIwStream, step_lo, step_hi}, hp->seed_lo, hp->seed_hi);
    const float ep = normal_from_bits(bits.x, bits.y);
    const float zz = mu + ep * expf(0.5f * lv);
    const size_t o = (size_t)v * Z + c;
    eps[o] = ep;
    z32[o] = zz;
    z16[o] = (__bf16)zz;
    term[c] = -0.5f * zz * zz + 0.5f * ep * ep + 0.5f * lv;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int c = 0; c < Z; ++c) t += term[c];
    prior[v] = t;
  }
}

// One 256-thread workgroup per virtual row: the clamped logit-form BCE of
// bce_logits_k, logits row v against image row v % M, summed over the P pixels
// (per-thread strided sums, then the fixed block tree).
__global__ void __launch_bounds__(256) iw_row_bce_k(const float* logits, const float* xb, int V, int M, int P,
                                                    float* bce) {
  __shared__ float scratch[16];
  const int v = blockIdx.x;
  if (v >= V) return;
  const float* t = logits + (size_t)v * P;
  const float* x = xb + (size_t)(v % M) * P;
  float loss = 0.f;
  for (int j = threadIdx.x; j < P; j += 256) {
    const float tj = t[j], xj = x[j];
    const float sp_pos = fmaxf(tj, 0.f) + log1pf(expf(-fabsf(tj)));
    loss += xj * fminf(sp_pos - tj, 100.f) + (1.f - xj) * fminf(sp_pos, 100.f);
  }
  const float s = block_sum(loss, scratch);
  if (threadIdx.x == 0) bce[v] = s;
}

}  // namespace mdt

using namespace mdt;

extern "C" int mdt_iw_reparam(const float* mulv, int M, int B, int Z, int k0, int S, const void* ist, const void* hp,
                              void* z16, float* z32, float* eps, float* prior, hipStream_t s) {
  if (M <= 0 || M > B || S < 1 || k0 < 0 || Z <= 0 || Z > kIwMaxZ || (long long)S * M > B) return 1;
  if ((unsigned long long)(k0 + S) * (unsigned long long)B * (unsigned long long)Z > (1ull << 32)) return 2;
  hipLaunchKernelGGL(iw_reparam_k, dim3(S * M), dim3(64), 0, s, mulv, M, B, Z, k0, S,
                     reinterpret_cast<const IwState*>(ist), reinterpret_cast<const HParams*>(hp),
                     reinterpret_cast<__bf16*>(z16), z32, eps, prior);
  return (int)hipGetLastError();
}

extern "C" int mdt_iw_row_bce(const float* logits, const float* xb, int V, int M, int P, float* bce, hipStream_t s) {
  if (V <= 0 || M <= 0 || P <= 0) return 1;
  hipLaunchKernelGGL(iw_row_bce_k, dim3(V), dim3(256), 0, s, logits, xb, V, M, P, bce);
  return (int)hipGetLastError();
}
