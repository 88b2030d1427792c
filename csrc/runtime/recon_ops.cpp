// Reconstruction report row table (csrc/kernels/recon.hip): the workspace size
// and the entry point that evaluate_recon and the kernel tests use.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>

#include "../kernels/recon.h"
#include "ops_common.h"

namespace mdt {

namespace {
const char* recon_reason(int rc) {
  switch (rc) {
    case 1: return "n must be in [1, 1048576]";
    case 2: return "side must be in [11, 256]";
    case 3: return "bands must be recon_bands(side)";
    case 4: return "missing buffer";
    default: return "launch failed";
  }
}

void recon_rc(int rc, const char* what) { throw_rc(rc, what, recon_reason(rc), 3); }

// The domain, before any size is computed from the arguments -> bands.
int64_t recon_domain(int64_t n, int64_t side) {
  if (n < 1 || n > kReconMaxRows) recon_rc(1, "recon");
  if (side < kReconMinSide || side > kReconMaxSide) recon_rc(2, "recon");
  return recon_bands((int)side);
}

// float32 workspace elements: the band sums of the sides the band kernel serves
int64_t recon_ws_numel(int64_t n, int64_t side) {
  const int64_t bands = recon_domain(n, side);
  return side <= kReconWaveSide ? 0 : n * bands * kReconCols;
}
}  // namespace

// table[n, 4] = se, ssim, l, cs of every row pair of real | recon [n, side * side].
void recon_rows(const at::Tensor& real, const at::Tensor& recon, int64_t side, at::Tensor ws, at::Tensor table) {
  TORCH_CHECK(f32_mat(real) && f32_mat(recon), "recon_rows: real and recon must be contiguous CUDA float32 matrices");
  TORCH_CHECK(real.sizes() == recon.sizes(), "recon_rows: real and recon must have the same shape");
  TORCH_CHECK(real.device() == recon.device() && ws.device() == real.device() && table.device() == real.device(),
              "recon_rows: all tensors must be on one device");
  const int64_t n = real.size(0);
  const int64_t bands = recon_domain(n, side);
  TORCH_CHECK(real.size(1) == side * side, "recon_rows: rows must hold side * side = ", side * side, " pixels");
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == torch::kFloat32 && ws.is_contiguous() &&
                  ws.numel() >= recon_ws_numel(n, side),
              "recon_rows: the workspace needs recon_ws_numel(n, side) float32 elements");
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == torch::kFloat32 && table.is_contiguous() && table.dim() == 2 &&
                  table.size(0) == n && table.size(1) == kReconCols,
              "recon_rows: table must be a contiguous CUDA float32 [n, ", kReconCols, "] tensor");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(real.device());
  ReconArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int)n; a.side = (int)side; a.bands = (int)bands;
  a.real = real.data_ptr<float>();
  a.recon = recon.data_ptr<float>();
  a.partial = side <= kReconWaveSide ? nullptr : ws.data_ptr<float>();
  a.table = table.data_ptr<float>();
  recon_rc(mdt_recon_rows(&a, c10::hip::getCurrentHIPStream().stream()), "recon_rows");
}

void bind_recon(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("kReconCols") = (int64_t)kReconCols;
  m.attr("kReconWaveSide") = (int64_t)kReconWaveSide;
  m.attr("kReconWaves") = (int64_t)kReconWaves;
  m.def("recon_bands", [](int64_t side) { return recon_domain(1, side); }, py::arg("side"));
  m.def("recon_ws_numel", &recon_ws_numel, py::arg("n"), py::arg("side"));
  m.def("recon_rows", &recon_rows, py::arg("real"), py::arg("recon"), py::arg("side"), py::arg("ws"), py::arg("table"));
}

}  // namespace mdt
