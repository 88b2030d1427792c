// What the sample-score entry points (two_sample, prdc, swd, gmm, sinkhorn, kmeans, recon _ops.cpp) share:
// the tensor checks, the 256-byte-segment workspace layout and the refusal a kernel's return code becomes.
#pragma once
#include <torch/extension.h>

#include <stdexcept>
#include <string>

namespace mdt {

inline bool f32_dense(const at::Tensor& t, int64_t dim) {
  return t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.dim() == dim && t.is_contiguous();
}
inline bool f32_mat(const at::Tensor& t) { return f32_dense(t, 2); }

inline int64_t align64(int64_t v) { return (v + 63) / 64 * 64; }

// A workspace of 32-bit words laid out segment by segment: every segment starts on a 256-byte boundary
struct Segments {
  int64_t total = 0;
  int64_t seg(int64_t numel) {
    const int64_t at = total;
    total = align64(total + numel);
    return at;
  }
};

// rc != 0 of an mdt_* entry point: codes 1 .. last_invalid are the caller's arguments (ValueError in Python),
// every other one a RuntimeError
inline void throw_rc(int rc, const char* what, const char* reason, int last_invalid) {
  if (rc == 0) return;
  const std::string msg = std::string("mdt: ") + what + ": " + reason + " (code " + std::to_string(rc) + ")";
  if (rc >= 1 && rc <= last_invalid) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}

}  // namespace mdt
