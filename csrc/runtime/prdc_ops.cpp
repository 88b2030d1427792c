// PRDC row table (csrc/kernels/prdc.hip): the workspace layout and the entry
// point that evaluate_samples and the kernel tests use.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>

#include "../kernels/prdc.h"
#include "ops_common.h"

namespace mdt {

namespace {
const char* prdc_reason(int rc) {
  switch (rc) {
    case 1: return "na and nb must be in [k + 1, 32768]";
    case 2: return "D must be in [1, 65536]";
    case 3: return "strips must be prdc_strips(na, nb)";
    case 4: return "k must be in [1, 8]";
    case 5: return "missing buffer";
    default: return "launch failed";
  }
}

void prdc_rc(int rc, const char* what) { throw_rc(rc, what, prdc_reason(rc), 4); }

// The domain, before any size is computed from the arguments.
int64_t prdc_domain(int64_t na, int64_t nb, int64_t D, int64_t k) {
  if (k < 1 || k > kPrdcMaxK) prdc_rc(4, "prdc");
  if (na <= k || na > kPrdcMaxRows || nb <= k || nb > kPrdcMaxRows) prdc_rc(1, "prdc");
  if (D < 1 || D > kPrdcMaxD) prdc_rc(2, "prdc");
  return prdc_strips(na, nb);
}

// 32-bit workspace words: every segment starts on a 256-byte boundary
struct PrdcLayout : Segments {
  int64_t q, rad, cnt, dminx, lists;
  PrdcLayout(int64_t rows, int64_t strips) {
    q = seg(rows);
    rad = seg(rows);
    cnt = seg(rows);
    dminx = seg(rows);
    lists = seg(strips * rows * kPrdcMaxK);
  }
};

int64_t prdc_strips_of(int64_t na, int64_t nb) { return prdc_domain(na, nb, 1, 1); }

int64_t prdc_ws_numel(int64_t na, int64_t nb, int64_t D, int64_t k) {
  return PrdcLayout(na + nb, prdc_domain(na, nb, D, k)).total;
}
}  // namespace

// out[na + nb, 3] = rad, cnt, dminx of every row of real | fake at neighbour rank k.
void prdc_rows(const at::Tensor& real, const at::Tensor& fake, int64_t k, at::Tensor ws, at::Tensor out) {
  TORCH_CHECK(f32_mat(real) && f32_mat(fake), "prdc_rows: real and fake must be contiguous CUDA float32 matrices");
  TORCH_CHECK(real.size(1) == fake.size(1), "prdc_rows: real and fake must have the same width");
  TORCH_CHECK(real.device() == fake.device() && ws.device() == real.device() && out.device() == real.device(),
              "prdc_rows: all tensors must be on one device");
  const int64_t na = real.size(0), nb = fake.size(0), D = real.size(1);
  const int64_t S = prdc_domain(na, nb, D, k);
  const PrdcLayout L(na + nb, S);
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == torch::kFloat32 && ws.is_contiguous() && ws.numel() >= L.total,
              "prdc_rows: the workspace needs prdc_ws_numel(na, nb, D, k) float32 elements");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat32 && out.is_contiguous() && out.dim() == 2 &&
                  out.size(0) == na + nb && out.size(1) == kPrdcCols,
              "prdc_rows: out must be a contiguous CUDA float32 [na + nb, ", kPrdcCols, "] tensor");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(real.device());
  PrdcArgs a;
  std::memset(&a, 0, sizeof(a));
  a.na = (int)na; a.nb = (int)nb; a.D = (int)D; a.k = (int)k; a.strips = (int)S;
  a.real = real.data_ptr<float>();
  a.fake = fake.data_ptr<float>();
  float* f = ws.data_ptr<float>();
  a.q = f + L.q;
  a.rad = f + L.rad;
  a.cnt = reinterpret_cast<int*>(f + L.cnt);
  a.dminx = reinterpret_cast<unsigned*>(f + L.dminx);
  a.lists = f + L.lists;
  a.out = out.data_ptr<float>();
  prdc_rc(mdt_prdc_rows(&a, c10::hip::getCurrentHIPStream().stream()), "prdc_rows");
}

void bind_prdc(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("kPrdcCols") = (int64_t)kPrdcCols;
  m.def("prdc_strips", &prdc_strips_of, py::arg("na"), py::arg("nb"));
  m.def("prdc_ws_numel", &prdc_ws_numel, py::arg("na"), py::arg("nb"), py::arg("D"), py::arg("k"));
  m.def("prdc_rows", &prdc_rows, py::arg("real"), py::arg("fake"), py::arg("k"), py::arg("ws"), py::arg("out"));
}

}  // namespace mdt
