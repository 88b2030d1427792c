// Ex-post Gaussian-mixture prior (csrc/kernels/gmm.hip): the fit and the score that
// evaluate_samples uses, and one EM iteration alone for the kernel tests.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>

#include "../kernels/gmm.h"
#include "ops_common.h"

namespace mdt {

namespace {
const char* gmm_reason(int rc) {
  switch (rc) {
    case 1: return "the number of rows must be above K and at most 2^20";
    case 2: return "Z must be in [1, 64]: a component's covariance is factored in one workgroup's LDS";
    case 3: return "the number of components must be in [1, 32]";
    case 4: return "missing buffer";
    case 5: return "the number of EM iterations must be in [0, 1000]";
    default: return "launch failed";
  }
}

void gmm_rc(int rc, const char* what) { throw_rc(rc, what, gmm_reason(rc), rc == 4 ? 3 : 5); }

bool f32_on(const at::Tensor& t, const at::Tensor& like) {
  return t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.device() == like.device();
}

// The domain, before any size is computed from the arguments.
void gmm_domain(int64_t n, int64_t Z, int64_t K, int64_t iters, const char* what) {
  if (K < 1 || K > kGmmMaxK) gmm_rc(3, what);
  if (n <= K || n > kGmmMaxRows) gmm_rc(1, what);
  if (Z < 1 || Z > kGmmMaxZ) gmm_rc(2, what);
  if (iters < 0 || iters > kGmmMaxIters) gmm_rc(5, what);
}

// z and ws checked, the workspace pointers set; r and ll point into ws
GmmArgs gmm_base(const at::Tensor& z, int64_t K, const at::Tensor& ws, double reg, const char* what) {
  TORCH_CHECK(f32_mat(z), what,
              ": z must be a contiguous CUDA float32 matrix");
  const int64_t n = z.size(0), Z = z.size(1);
  gmm_domain(n, Z, K, 0, what);
  const GmmWs w = gmm_ws_layout((int)n, (int)Z, (int)K);
  TORCH_CHECK(f32_on(ws, z) && ws.dim() == 1 && (size_t)ws.numel() >= w.total, what,
              ": ws must be a contiguous CUDA float32 vector of gmm_ws_numel(n, Z, K) elements on z's device");
  TORCH_CHECK(reg >= 0.0, what, ": reg must not be negative");
  GmmArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = (int)n; a.Z = (int)Z; a.K = (int)K;
  a.reg = (float)reg;
  a.z = z.data_ptr<float>();
  float* p = ws.data_ptr<float>();
  a.W = p + w.W; a.c = p + w.c; a.status = p + w.status; a.llpart = p + w.llpart; a.mpart = p + w.mpart;
  a.r = p + w.r; a.ll = p + w.ll;
  return a;
}

void gmm_params(GmmArgs& a, const at::Tensor& z, const at::Tensor& pi, const at::Tensor& mu, const at::Tensor& cov,
                const char* what) {
  const int64_t K = a.K, Z = a.Z;
  TORCH_CHECK(f32_on(pi, z) && pi.dim() == 1 && pi.size(0) == K && f32_on(mu, z) && mu.dim() == 2 && mu.size(0) == K &&
                  mu.size(1) == Z && f32_on(cov, z) && cov.dim() == 3 && cov.size(0) == K && cov.size(1) == Z &&
                  cov.size(2) == Z,
              what, ": parameters must be contiguous CUDA float32 pi [K], mu [K, Z], cov [K, Z, Z] on z's device");
  a.pi = pi.data_ptr<float>(); a.mu = mu.data_ptr<float>(); a.cov = cov.data_ptr<float>();
}

// After the launches: a pivot that was not positive is the caller's error (this synchronises)
void gmm_status(const GmmArgs& a, const at::Tensor& ws, const char* what) {
  const at::Tensor st = ws.narrow(0, a.status - ws.data_ptr<float>(), a.K).cpu();
  for (int64_t k = 0; k < a.K; ++k)
    if (st[k].item<float>() != 0.f)
      throw std::invalid_argument(std::string("mdt: ") + what + ": the covariance of mixture component " +
                                  std::to_string(k) + " is not positive definite");
}
}  // namespace

int64_t gmm_ws_numel(int64_t n, int64_t Z, int64_t K) {
  gmm_domain(n, Z, K, 0, "gmm_ws_numel");
  return (int64_t)gmm_ws_layout((int)n, (int)Z, (int)K).total;
}

// "W" [K, Z, Z], "c" [K], "r" [n, K], "ll" [n]: views of what the last call left in ws
at::Tensor gmm_ws_view(const at::Tensor& ws, int64_t n, int64_t Z, int64_t K, const std::string& name) {
  gmm_domain(n, Z, K, 0, "gmm_ws_view");
  const GmmWs w = gmm_ws_layout((int)n, (int)Z, (int)K);
  TORCH_CHECK(ws.dim() == 1 && (size_t)ws.numel() >= w.total, "gmm_ws_view: ws is too small");
  if (name == "W") return ws.narrow(0, w.W, K * Z * Z).view({K, Z, Z});
  if (name == "c") return ws.narrow(0, w.c, K);
  if (name == "r") return ws.narrow(0, w.r, n * K).view({n, K});
  if (name == "ll") return ws.narrow(0, w.ll, n);
  throw std::invalid_argument("gmm_ws_view: no part named " + name);
}

// params_out [K (1 + Z + Z Z)] = pi | mu | cov of the fit; ll_history [iters + 1]; r and ll of the last E-step in ws
void gmm_fit(const at::Tensor& z, int64_t K, int64_t iters, at::Tensor ws, at::Tensor params_out, at::Tensor ll_history) {
  GmmArgs a = gmm_base(z, K, ws, kGmmRegCovar, "gmm_fit");
  gmm_domain(a.n, a.Z, K, iters, "gmm_fit");
  const int64_t Z = a.Z;
  TORCH_CHECK(f32_on(params_out, z) && params_out.dim() == 1 && params_out.numel() == K * (1 + Z + Z * Z),
              "gmm_fit: params_out must be a contiguous CUDA float32 vector of K (1 + Z + Z Z) elements");
  TORCH_CHECK(f32_on(ll_history, z) && ll_history.dim() == 1 && ll_history.numel() == iters + 1,
              "gmm_fit: ll_history must be a contiguous CUDA float32 vector of iters + 1 elements");
  a.pi = params_out.data_ptr<float>();
  a.mu = a.pi + K;
  a.cov = a.mu + K * Z;
  a.ll_hist = ll_history.data_ptr<float>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(z.device());
  gmm_rc(mdt_gmm_fit(&a, (int)iters, c10::hip::getCurrentHIPStream().stream()), "gmm_fit");
  gmm_status(a, ws, "gmm_fit");
}

// One EM iteration from (pi, mu, cov): r [n, K], ll [n], the next parameters; ws keeps W and c of the input ones
void gmm_em_step(const at::Tensor& z, const at::Tensor& pi, const at::Tensor& mu, const at::Tensor& cov, at::Tensor ws,
                 at::Tensor r, at::Tensor ll, at::Tensor pi_out, at::Tensor mu_out, at::Tensor cov_out, double reg) {
  GmmArgs a = gmm_base(z, pi.dim() == 1 ? pi.size(0) : 0, ws, reg, "gmm_em_step");
  gmm_params(a, z, pi, mu, cov, "gmm_em_step");
  GmmArgs o = a;
  gmm_params(o, z, pi_out, mu_out, cov_out, "gmm_em_step");
  TORCH_CHECK(f32_on(r, z) && r.dim() == 2 && r.size(0) == a.n && r.size(1) == a.K && f32_on(ll, z) && ll.dim() == 1 &&
                  ll.size(0) == a.n,
              "gmm_em_step: r must be [n, K] and ll [n], contiguous CUDA float32 on z's device");
  a.pi_out = o.pi; a.mu_out = o.mu; a.cov_out = o.cov;
  a.r = r.data_ptr<float>();
  a.ll = ll.data_ptr<float>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(z.device());
  gmm_rc(mdt_gmm_em_step(&a, c10::hip::getCurrentHIPStream().stream()), "gmm_em_step");
  gmm_status(a, ws, "gmm_em_step");
}

// ll [n] of the rows under (pi, mu, cov)
void gmm_score(const at::Tensor& z, const at::Tensor& pi, const at::Tensor& mu, const at::Tensor& cov, at::Tensor ws,
               at::Tensor ll, double reg) {
  GmmArgs a = gmm_base(z, pi.dim() == 1 ? pi.size(0) : 0, ws, reg, "gmm_score");
  gmm_params(a, z, pi, mu, cov, "gmm_score");
  TORCH_CHECK(f32_on(ll, z) && ll.dim() == 1 && ll.size(0) == a.n,
              "gmm_score: ll must be a contiguous CUDA float32 [n] vector on z's device");
  a.ll = ll.data_ptr<float>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(z.device());
  gmm_rc(mdt_gmm_score(&a, c10::hip::getCurrentHIPStream().stream()), "gmm_score");
  gmm_status(a, ws, "gmm_score");
}

void bind_gmm(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("kGmmMaxK") = (int64_t)kGmmMaxK;
  m.attr("kGmmMaxZ") = (int64_t)kGmmMaxZ;
  m.attr("kGmmMaxRows") = (int64_t)kGmmMaxRows;
  m.def("gmm_ws_numel", &gmm_ws_numel, py::arg("n"), py::arg("Z"), py::arg("K"));
  m.def("gmm_ws_view", &gmm_ws_view, py::arg("ws"), py::arg("n"), py::arg("Z"), py::arg("K"), py::arg("name"));
  m.def("gmm_fit", &gmm_fit, py::arg("z"), py::arg("K"), py::arg("iters"), py::arg("ws"), py::arg("params_out"),
        py::arg("ll_history"));
  m.def("gmm_em_step", &gmm_em_step, py::arg("z"), py::arg("pi"), py::arg("mu"), py::arg("cov"), py::arg("ws"),
        py::arg("r"), py::arg("ll"), py::arg("pi_out"), py::arg("mu_out"), py::arg("cov_out"),
        py::arg("reg") = (double)kGmmRegCovar);
  m.def("gmm_score", &gmm_score, py::arg("z"), py::arg("pi"), py::arg("mu"), py::arg("cov"), py::arg("ws"), py::arg("ll"),
        py::arg("reg") = (double)kGmmRegCovar);
}

}  // namespace mdt
