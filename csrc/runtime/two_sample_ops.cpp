// Two-sample row statistics (csrc/kernels/two_sample.hip): the workspace layout and
// the entry point that evaluate_samples and the kernel tests use.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cmath>
#include <cstring>
#include <stdexcept>

#include "../kernels/two_sample.h"

namespace mdt {

namespace {
inline int64_t align64(int64_t v) { return (v + 63) / 64 * 64; }

const char* ts_reason(int rc) {
  switch (rc) {
    case 1: return "na and nb must be in [2, 32768]";
    case 2: return "D must be in [1, 65536]";
    case 3: return "strips must be ts_strips(na + nb)";
    case 5: return "missing buffer";
    default: return "launch failed";
  }
}

void ts_rc(int rc, const char* what) {
  if (rc == 0) return;
  const std::string msg = std::string("mdt: ") + what + ": " + ts_reason(rc) + " (code " + std::to_string(rc) + ")";
  if (rc >= 1 && rc <= 3) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}

// The domain, before any size is computed from the arguments.
int64_t ts_domain(int64_t na, int64_t nb, int64_t D) {
  if (na < 2 || na > kTsMaxRows || nb < 2 || nb > kTsMaxRows) ts_rc(1, "two_sample");
  if (D < 1 || D > kTsMaxD) ts_rc(2, "two_sample");
  return ts_strips(na + nb);
}

// float32 workspace: every segment starts on a 256-byte boundary
struct TwoSampleLayout {
  int64_t q, part, tpart, total;
  TwoSampleLayout(int64_t rows, int64_t strips) {
    int64_t o = 0;
    auto seg = [&](int64_t numel) { const int64_t at = o; o = align64(o + numel); return at; };
    q = seg(rows);
    part = seg(strips * rows * kTsCols);
    tpart = seg((int64_t)ts_toffsets(rows) * rows * kTsCols);
    total = o;
  }
};

int64_t two_sample_strips(int64_t na, int64_t nb) { return ts_domain(na, nb, 1); }

int64_t two_sample_ws_numel(int64_t na, int64_t nb, int64_t D) {
  return TwoSampleLayout(na + nb, ts_domain(na, nb, D)).total;
}

bool f32_mat(const at::Tensor& t) {
  return t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.dim() == 2 && t.is_contiguous();
}
}  // namespace

// out[na + nb, 8] = dmin_r, dmin_f, ksum_r[3], ksum_f[3] of every row of real | fake under bandwidths h.
void two_sample_rows(const at::Tensor& real, const at::Tensor& fake, const std::vector<double>& h, at::Tensor ws,
                     at::Tensor out) {
  TORCH_CHECK(f32_mat(real) && f32_mat(fake), "two_sample_rows: real and fake must be contiguous CUDA float32 matrices");
  TORCH_CHECK(real.size(1) == fake.size(1), "two_sample_rows: real and fake must have the same width");
  TORCH_CHECK(real.device() == fake.device() && ws.device() == real.device() && out.device() == real.device(),
              "two_sample_rows: all tensors must be on one device");
  const int64_t na = real.size(0), nb = fake.size(0), D = real.size(1);
  const int64_t S = ts_domain(na, nb, D);
  const TwoSampleLayout L(na + nb, S);
  TORCH_CHECK((int64_t)h.size() == kTsBandwidths, "two_sample_rows: needs ", kTsBandwidths, " bandwidths");
  for (double v : h) TORCH_CHECK(v > 0.0 && std::isfinite(v), "two_sample_rows: bandwidths must be positive and finite");
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == torch::kFloat32 && ws.is_contiguous() && ws.numel() >= L.total,
              "two_sample_rows: the workspace needs two_sample_ws_numel(na, nb, D) float32 elements");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat32 && out.is_contiguous() && out.dim() == 2 &&
                  out.size(0) == na + nb && out.size(1) == kTsCols,
              "two_sample_rows: out must be a contiguous CUDA float32 [na + nb, ", kTsCols, "] tensor");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(real.device());
  TwoSampleArgs a;
  std::memset(&a, 0, sizeof(a));
  a.na = (int)na; a.nb = (int)nb; a.D = (int)D; a.strips = (int)S;
  a.real = real.data_ptr<float>();
  a.fake = fake.data_ptr<float>();
  for (int s = 0; s < kTsBandwidths; ++s) {
    const double c = -1.0 / h[s];
    a.c_hi[s] = (float)c;
    a.c_lo[s] = (float)(c - (double)a.c_hi[s]);
  }
  float* f = ws.data_ptr<float>();
  a.q = f + L.q;
  a.part = f + L.part;
  a.tpart = f + L.tpart;
  a.out = out.data_ptr<float>();
  ts_rc(mdt_two_sample_rows(&a, c10::hip::getCurrentHIPStream().stream()), "two_sample_rows");
}

void bind_two_sample(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("kTsCols") = (int64_t)kTsCols;
  m.def("two_sample_strips", &two_sample_strips, py::arg("na"), py::arg("nb"));
  m.def("two_sample_ws_numel", &two_sample_ws_numel, py::arg("na"), py::arg("nb"), py::arg("D"));
  m.def("two_sample_rows", &two_sample_rows, py::arg("real"), py::arg("fake"), py::arg("h"), py::arg("ws"),
        py::arg("out"));
}

}  // namespace mdt
