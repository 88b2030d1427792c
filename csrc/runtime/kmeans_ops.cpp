// k-means bins of the NDB / JSD score (csrc/kernels/kmeans.hip): the fit that
// evaluate_samples and the kernel tests use, and the two steps alone for the tests,
// the bench and the mixture draws' second assignment.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>
#include <tuple>

#include "../kernels/kmeans.h"
#include "ops_common.h"

namespace mdt {

namespace {
const char* km_reason(int rc) {
  switch (rc) {
    case 1: return "rows must be in [2, 65536] per set";
    case 2: return "D must be in [1, 65536]";
    case 3: return "K must be in [2, 256], and a fit's K at most the real rows";
    case 4: return "the iterations must be in [1, 1000]";
    case 5: return "missing or misaligned buffer";
    default: return "launch failed";
  }
}

void km_rc(int rc, const char* what) { throw_rc(rc, what, km_reason(rc), 4); }

// The domain, before any size is computed from the arguments. nb == 0: no second set. fit: K starts from real rows.
void km_domain(int64_t na, int64_t nb, int64_t D, int64_t K, int64_t T, bool fit, const char* what) {
  if (na < 2 || na > kKmMaxRows || nb < 0 || nb == 1 || nb > kKmMaxRows) km_rc(1, what);
  if (D < 1 || D > kKmMaxD) km_rc(2, what);
  if (K < 2 || K > kKmMaxK || (fit && K > na)) km_rc(3, what);
  if (T < 1 || T > kKmMaxIters) km_rc(4, what);
}

KmeansArgs km_inputs(const at::Tensor& real, const c10::optional<at::Tensor>& fake, int64_t K, int64_t T, bool fit,
                     const at::Tensor& ws, const char* what) {
  TORCH_CHECK(f32_mat(real), what,
              ": the rows must be a contiguous CUDA float32 matrix");
  const int64_t na = real.size(0), D = real.size(1), nb = fake ? fake->size(0) : 0;
  if (fake) {
    TORCH_CHECK(f32_dense(*fake, 2) && fake->device() == real.device(), what,
                ": the second set must be a contiguous CUDA float32 matrix on the first's device");
    TORCH_CHECK(fake->size(1) == D, what, ": both sets must have the same width");
    if (nb < 2) km_rc(1, what);
  }
  km_domain(na, nb, D, K, T, fit, what);
  TORCH_CHECK(f32_dense(ws, 1) && ws.device() == real.device() &&
                  (uint64_t)ws.numel() >= km_layout((int)na, (int)nb, (int)D, (int)K).total,
              what, ": ws must be a contiguous CUDA float32 vector of at least kmeans_ws_numel(na, nb, D, K) elements");
  KmeansArgs a;
  std::memset(&a, 0, sizeof(a));
  a.na = (int)na; a.nb = (int)nb; a.D = (int)D; a.K = (int)K; a.T = (int)T;
  a.real = real.data_ptr<float>();
  a.fake = fake ? fake->data_ptr<float>() : nullptr;
  a.ws = ws.data_ptr<float>();
  return a;
}

at::Tensor km_new(const at::Tensor& like, at::IntArrayRef shape, at::ScalarType t) {
  return torch::empty(shape, like.options().dtype(t));
}
}  // namespace

// Raises ValueError outside the domain of a fit; nothing is launched.
void kmeans_check(int64_t na, int64_t nb, int64_t D, int64_t K, int64_t T) {
  if (nb < 2) km_rc(1, "kmeans_check");
  km_domain(na, nb, D, K, T, true, "kmeans_check");
}

int64_t kmeans_ws_numel(int64_t na, int64_t nb, int64_t D, int64_t K) {
  km_domain(na, nb, D, K, 1, false, "kmeans_ws_numel");
  return (int64_t)km_layout((int)na, (int)nb, (int)D, (int)K).total;
}

// How the launches split the work: rows per band of an assign launch over n rows, rows per split of the update.
pybind11::dict kmeans_layout(int64_t n) {
  pybind11::dict d;
  d["band"] = (int64_t)km_band((int)n);
  d["split_rows"] = (int64_t)kKmSplitRows;
  d["chunk"] = (int64_t)kKmBK;
  return d;
}

// (labels [na + nb] int32, mind [na + nb], centroids [K, D], moved [T] int32, inertia [1] float64)
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> kmeans_rows(
    const at::Tensor& real, const at::Tensor& fake, int64_t K, int64_t T, const at::Tensor& init_idx, at::Tensor ws) {
  KmeansArgs a = km_inputs(real, fake, K, T, true, ws, "kmeans_rows");
  TORCH_CHECK(init_idx.is_cuda() && init_idx.scalar_type() == torch::kInt64 && init_idx.dim() == 1 &&
                  init_idx.numel() == K && init_idx.is_contiguous() && init_idx.device() == real.device(),
              "kmeans_rows: init_idx must be a contiguous CUDA int64 vector of K row indices on the rows' device");
  const at::Tensor host = init_idx.cpu();
  for (int64_t k = 0; k < K; ++k) {
    const int64_t v = host.data_ptr<int64_t>()[k];
    TORCH_CHECK(v >= 0 && v < a.na, "kmeans_rows: init_idx[", k, "] = ", v, " is no real row");
  }
  at::Tensor labels = km_new(real, {a.na + a.nb}, torch::kInt32), mind = km_new(real, {a.na + a.nb}, torch::kFloat32);
  at::Tensor cent = km_new(real, {K, a.D}, torch::kFloat32), moved = km_new(real, {T}, torch::kInt32);
  at::Tensor inertia = km_new(real, {1}, torch::kFloat64);
  a.init = reinterpret_cast<const long long*>(init_idx.data_ptr<int64_t>());
  a.cent = cent.data_ptr<float>();
  a.labels = labels.data_ptr<int>();
  a.mind = mind.data_ptr<float>();
  a.moved = moved.data_ptr<int>();
  a.inertia = inertia.data_ptr<double>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(real.device());
  km_rc(mdt_kmeans_rows(&a, c10::hip::getCurrentHIPStream().stream()), "kmeans_rows");
  return {labels, mind, cent, moved, inertia};
}

// One assignment of x | y (y optional) to given centroids: (labels int32, mind, moved [1] int32). With `prev`
// (int32 labels of the same rows) moved counts the rows whose label differs from it, else every row.
std::tuple<at::Tensor, at::Tensor, at::Tensor> kmeans_assign(const at::Tensor& x, const c10::optional<at::Tensor>& y,
                                                             const at::Tensor& cent, at::Tensor ws,
                                                             const c10::optional<at::Tensor>& prev) {
  TORCH_CHECK(f32_dense(cent, 2), "kmeans_assign: the centroids must be a contiguous CUDA float32 matrix");
  KmeansArgs a = km_inputs(x, y, cent.size(0), 1, false, ws, "kmeans_assign");
  TORCH_CHECK(cent.size(1) == a.D && cent.device() == x.device(), "kmeans_assign: the centroids must have the rows' width and device");
  const int64_t n = a.na + a.nb;
  at::Tensor labels = km_new(x, {n}, torch::kInt32);
  if (prev) {
    TORCH_CHECK(prev->is_cuda() && prev->scalar_type() == torch::kInt32 && prev->dim() == 1 && prev->numel() == n &&
                    prev->is_contiguous() && prev->device() == x.device(),
                "kmeans_assign: prev must be a contiguous CUDA int32 vector of one label per row");
    labels.copy_(*prev);
  }
  at::Tensor mind = km_new(x, {n}, torch::kFloat32), moved = km_new(x, {1}, torch::kInt32);
  a.cent = cent.data_ptr<float>();
  a.labels = labels.data_ptr<int>();
  a.mind = mind.data_ptr<float>();
  a.moved = moved.data_ptr<int>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  km_rc(mdt_kmeans_assign(&a, prev ? 1 : 0, c10::hip::getCurrentHIPStream().stream()), "kmeans_assign");
  return {labels, mind, moved};
}

// One update from given labels: (centroids [K, D], counts [K] int32); a cell without rows keeps its row of `cent`.
std::tuple<at::Tensor, at::Tensor> kmeans_update(const at::Tensor& x, const at::Tensor& labels, const at::Tensor& cent,
                                                 at::Tensor ws) {
  TORCH_CHECK(f32_dense(cent, 2), "kmeans_update: the centroids must be a contiguous CUDA float32 matrix");
  KmeansArgs a = km_inputs(x, c10::nullopt, cent.size(0), 1, false, ws, "kmeans_update");
  TORCH_CHECK(cent.size(1) == a.D && cent.device() == x.device(), "kmeans_update: the centroids must have the rows' width and device");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == torch::kInt32 && labels.dim() == 1 && labels.numel() == a.na &&
                  labels.is_contiguous() && labels.device() == x.device(),
              "kmeans_update: labels must be a contiguous CUDA int32 vector of one label per row");
  at::Tensor out = cent.clone(), counts = km_new(x, {a.K}, torch::kInt32);
  a.cent = out.data_ptr<float>();
  a.labels = labels.data_ptr<int>();
  a.counts = counts.data_ptr<int>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  km_rc(mdt_kmeans_update(&a, c10::hip::getCurrentHIPStream().stream()), "kmeans_update");
  return {out, counts};
}

void bind_kmeans(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("kKmMaxK") = (int64_t)kKmMaxK;
  m.attr("kKmMaxRows") = (int64_t)kKmMaxRows;
  m.def("kmeans_check", &kmeans_check, py::arg("na"), py::arg("nb"), py::arg("D"), py::arg("K"), py::arg("T"));
  m.def("kmeans_ws_numel", &kmeans_ws_numel, py::arg("na"), py::arg("nb"), py::arg("D"), py::arg("K"));
  m.def("kmeans_layout", &kmeans_layout, py::arg("n"));
  m.def("kmeans_rows", &kmeans_rows, py::arg("real"), py::arg("fake"), py::arg("K"), py::arg("T"), py::arg("init_idx"),
        py::arg("ws"));
  m.def("kmeans_assign", &kmeans_assign, py::arg("x"), py::arg("y"), py::arg("centroids"), py::arg("ws"),
        py::arg("prev") = py::none());
  m.def("kmeans_update", &kmeans_update, py::arg("x"), py::arg("labels"), py::arg("centroids"), py::arg("ws"));
}

}  // namespace mdt
