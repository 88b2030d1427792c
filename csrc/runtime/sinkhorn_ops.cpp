// Sinkhorn divergence (csrc/kernels/sinkhorn.hip): the entry point that
// evaluate_samples and the kernel tests use, and the two phases alone for the tests and the bench.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cmath>
#include <cstring>
#include <stdexcept>

#include "../kernels/sinkhorn.h"
#include "ops_common.h"

namespace mdt {

namespace {
const char* sk_reason(int rc) {
  switch (rc) {
    case 1: return "na and nb must be in [2, 16384]: the cost matrices are stored";
    case 2: return "D must be in [1, 65536]";
    case 3: return "the blur must be finite and in (0, 4]";
    case 4: return "the iterations must be in [1, 10000], and an iteration's index below them";
    case 5: return "missing or misaligned buffer";
    default: return "launch failed";
  }
}

void sk_rc(int rc, const char* what) { throw_rc(rc, what, sk_reason(rc), 4); }

// The domain, before any size is computed from the arguments.
void sk_domain(int64_t na, int64_t nb, int64_t D, double E, int64_t T, const char* what) {
  if (na < 2 || na > kSkMaxRows || nb < 2 || nb > kSkMaxRows) sk_rc(1, what);
  if (D < 1 || D > kSkMaxD) sk_rc(2, what);
  if (!(std::isfinite(E) && E > 0.0 && E <= kSkMaxBlur)) sk_rc(3, what);
  if (T < 1 || T > kSkMaxIters) sk_rc(4, what);
}

void sk_check_ws(const at::Tensor& ws, int64_t na, int64_t nb, const char* what) {
  TORCH_CHECK(f32_dense(ws, 1) && (uint64_t)ws.numel() >= sk_layout((int)na, (int)nb).total, what,
              ": ws must be a contiguous CUDA float32 vector of at least sinkhorn_ws_numel(na, nb) elements");
}

void sk_check_outs(const at::Tensor& ws, const at::Tensor& pot, const at::Tensor& out, int64_t na, int64_t nb,
                   const char* what) {
  TORCH_CHECK(f32_dense(pot, 2) && pot.size(0) == na + nb && pot.size(1) == kSkCols && pot.device() == ws.device(), what,
              ": pot must be a contiguous CUDA float32 [na + nb, ", kSkCols, "] tensor on the workspace's device");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat64 && out.dim() == 1 && out.numel() == 2 &&
                  out.is_contiguous() && out.device() == ws.device(),
              what, ": out must be a contiguous CUDA float64 vector of 2 elements on the workspace's device");
}

SinkhornArgs sk_inputs(const at::Tensor& real, const at::Tensor& fake, double E, int64_t T, const at::Tensor& ws,
                       const char* what) {
  TORCH_CHECK(f32_dense(real, 2) && f32_dense(fake, 2), what, ": real and fake must be contiguous CUDA float32 matrices");
  TORCH_CHECK(real.size(1) == fake.size(1), what, ": real and fake must have the same width");
  TORCH_CHECK(real.device() == fake.device() && ws.device() == real.device(), what, ": all tensors must be on one device");
  const int64_t na = real.size(0), nb = fake.size(0), D = real.size(1);
  sk_domain(na, nb, D, E, T, what);
  sk_check_ws(ws, na, nb, what);
  SinkhornArgs a;
  std::memset(&a, 0, sizeof(a));
  a.na = (int)na; a.nb = (int)nb; a.D = (int)D; a.T = (int)T;
  a.E = E;
  a.real = real.data_ptr<float>();
  a.fake = fake.data_ptr<float>();
  a.ws = ws.data_ptr<float>();
  return a;
}
}  // namespace

int64_t sinkhorn_ws_numel(int64_t na, int64_t nb) {
  sk_domain(na, nb, 1, 1.0, 1, "sinkhorn_ws_numel");
  return (int64_t)sk_layout((int)na, (int)nb).total;
}

// Where the workspace keeps what: float offsets of the three matrices with their row strides, of m (a double)
// and the rows per band of the iteration kernel.
pybind11::dict sinkhorn_layout(int64_t na, int64_t nb) {
  sk_domain(na, nb, 1, 1.0, 1, "sinkhorn_layout");
  const SkLayout L = sk_layout((int)na, (int)nb);
  pybind11::dict d;
  d["cxy"] = (int64_t)L.cxy; d["cxx"] = (int64_t)L.cxx; d["cyy"] = (int64_t)L.cyy;
  d["lda"] = (int64_t)L.lda; d["ldb"] = (int64_t)L.ldb;
  d["scale"] = (int64_t)L.scale;
  d["band"] = (int64_t)kSkBand;
  return d;
}

// pot[na + nb, 2] = (ft | gt), (pt | qt) after T iterations at blur E; out[2] = m, marg_err.
void sinkhorn_rows(const at::Tensor& real, const at::Tensor& fake, double E, int64_t T, at::Tensor ws, at::Tensor pot,
                   at::Tensor out) {
  SinkhornArgs a = sk_inputs(real, fake, E, T, ws, "sinkhorn_rows");
  sk_check_outs(ws, pot, out, a.na, a.nb, "sinkhorn_rows");
  a.pot = pot.data_ptr<float>();
  a.out = out.data_ptr<double>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(real.device());
  sk_rc(mdt_sinkhorn_rows(&a, c10::hip::getCurrentHIPStream().stream()), "sinkhorn_rows");
}

// The cost phase alone: the three matrices and m into ws, the potentials cleared.
void sinkhorn_cost(const at::Tensor& real, const at::Tensor& fake, at::Tensor ws) {
  const SinkhornArgs a = sk_inputs(real, fake, 1.0, 1, ws, "sinkhorn_cost");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(real.device());
  sk_rc(mdt_sinkhorn_cost(&a, c10::hip::getCurrentHIPStream().stream()), "sinkhorn_cost");
}

// Iteration t of T alone, on a workspace that sinkhorn_cost has filled and iterations 0 .. t-1 have advanced.
void sinkhorn_step(int64_t na, int64_t nb, double E, int64_t T, int64_t t, at::Tensor ws, at::Tensor pot, at::Tensor out) {
  sk_domain(na, nb, 1, E, T, "sinkhorn_step");
  if (t < 0 || t >= T) sk_rc(4, "sinkhorn_step");
  sk_check_ws(ws, na, nb, "sinkhorn_step");
  sk_check_outs(ws, pot, out, na, nb, "sinkhorn_step");
  SinkhornArgs a;
  std::memset(&a, 0, sizeof(a));
  a.na = (int)na; a.nb = (int)nb; a.D = 1; a.T = (int)T;
  a.E = E;
  a.ws = ws.data_ptr<float>();
  a.pot = pot.data_ptr<float>();
  a.out = out.data_ptr<double>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(ws.device());
  sk_rc(mdt_sinkhorn_step(&a, (int)t, c10::hip::getCurrentHIPStream().stream()), "sinkhorn_step");
}

void bind_sinkhorn(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("kSkCols") = (int64_t)kSkCols;
  m.attr("kSkMaxRows") = (int64_t)kSkMaxRows;
  m.attr("kSkMaxIters") = (int64_t)kSkMaxIters;
  m.def("sinkhorn_ws_numel", &sinkhorn_ws_numel, py::arg("na"), py::arg("nb"));
  m.def("sinkhorn_layout", &sinkhorn_layout, py::arg("na"), py::arg("nb"));
  m.def("sinkhorn_rows", &sinkhorn_rows, py::arg("real"), py::arg("fake"), py::arg("E"), py::arg("T"), py::arg("ws"),
        py::arg("pot"), py::arg("out"));
  m.def("sinkhorn_cost", &sinkhorn_cost, py::arg("real"), py::arg("fake"), py::arg("ws"));
  m.def("sinkhorn_step", &sinkhorn_step, py::arg("na"), py::arg("nb"), py::arg("E"), py::arg("T"), py::arg("t"),
        py::arg("ws"), py::arg("pot"), py::arg("out"));
}

}  // namespace mdt
