// Sliced Wasserstein distance (csrc/kernels/swd.hip): the entry point that
// evaluate_samples and the kernel tests use, and the two launches alone for the bench.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>

#include "../kernels/swd.h"
#include "ops_common.h"

namespace mdt {

namespace {
const char* swd_reason(int rc) {
  switch (rc) {
    case 1: return "na and nb must be in [2, 16384]: both sorted sets of a projection are held in one workgroup's LDS";
    case 2: return "D must be in [1, 65536]";
    case 3: return "the number of directions must be in [1, 4096]";
    case 4: return "missing buffer";
    default: return "launch failed";
  }
}

void swd_rc(int rc, const char* what) { throw_rc(rc, what, swd_reason(rc), 3); }

// The domain, before any size is computed from the arguments.
void swd_domain(int64_t na, int64_t nb, int64_t D, int64_t P, const char* what) {
  if (na < 2 || na > kSwdMaxRows || nb < 2 || nb > kSwdMaxRows) swd_rc(1, what);
  if (D < 1 || D > kSwdMaxD) swd_rc(2, what);
  if (P < 1 || P > kSwdMaxDirs) swd_rc(3, what);
}

SwdArgs swd_inputs(const at::Tensor& real, const at::Tensor& fake, const at::Tensor& dirs, const at::Tensor& proj,
                   const char* what) {
  TORCH_CHECK(f32_mat(real) && f32_mat(fake) && f32_mat(dirs), what,
              ": real, fake and dirs must be contiguous CUDA float32 matrices");
  TORCH_CHECK(real.size(1) == fake.size(1) && real.size(1) == dirs.size(1), what,
              ": real, fake and dirs must have the same width");
  TORCH_CHECK(real.device() == fake.device() && dirs.device() == real.device() && proj.device() == real.device(), what,
              ": all tensors must be on one device");
  const int64_t na = real.size(0), nb = fake.size(0), D = real.size(1), P = dirs.size(0);
  swd_domain(na, nb, D, P, what);
  TORCH_CHECK(f32_mat(proj) && proj.size(0) == P && proj.size(1) == na + nb, what,
              ": proj must be a contiguous CUDA float32 [P, na + nb] tensor");
  SwdArgs a;
  std::memset(&a, 0, sizeof(a));
  a.na = (int)na; a.nb = (int)nb; a.D = (int)D; a.P = (int)P;
  a.real = real.data_ptr<float>();
  a.fake = fake.data_ptr<float>();
  a.dirs = dirs.data_ptr<float>();
  a.proj = proj.data_ptr<float>();
  return a;
}

void swd_check_out(const at::Tensor& proj, const at::Tensor& out, const char* what) {
  TORCH_CHECK(f32_mat(out) && out.device() == proj.device() && out.size(0) == proj.size(0) && out.size(1) == kSwdCols,
              what, ": out must be a contiguous CUDA float32 [P, ", kSwdCols, "] tensor on proj's device");
}
}  // namespace

// proj[P, na + nb] = per direction the sorted real | the sorted fake projections; out[P, 2] = w1, w2sq.
void swd_rows(const at::Tensor& real, const at::Tensor& fake, const at::Tensor& dirs, at::Tensor proj, at::Tensor out) {
  SwdArgs a = swd_inputs(real, fake, dirs, proj, "swd_rows");
  swd_check_out(proj, out, "swd_rows");
  a.out = out.data_ptr<float>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(real.device());
  swd_rc(mdt_swd_rows(&a, c10::hip::getCurrentHIPStream().stream()), "swd_rows");
}

// The first launch alone: proj[P, na + nb] = the projections, unsorted.
void swd_project(const at::Tensor& real, const at::Tensor& fake, const at::Tensor& dirs, at::Tensor proj) {
  const SwdArgs a = swd_inputs(real, fake, dirs, proj, "swd_project");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(real.device());
  swd_rc(mdt_swd_project(&a, c10::hip::getCurrentHIPStream().stream()), "swd_project");
}

// The second launch alone, on a proj [P, na + nb] of projections: sorts it in place, out[P, 2] = w1, w2sq.
void swd_sort(int64_t na, int64_t nb, at::Tensor proj, at::Tensor out) {
  TORCH_CHECK(f32_mat(proj), "swd_sort: proj must be a contiguous CUDA float32 matrix");
  swd_domain(na, nb, 1, proj.size(0), "swd_sort");
  TORCH_CHECK(proj.size(1) == na + nb, "swd_sort: proj must be [P, na + nb]");
  swd_check_out(proj, out, "swd_sort");
  SwdArgs a;
  std::memset(&a, 0, sizeof(a));
  a.na = (int)na; a.nb = (int)nb; a.D = 1; a.P = (int)proj.size(0);
  a.proj = proj.data_ptr<float>();
  a.out = out.data_ptr<float>();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(proj.device());
  swd_rc(mdt_swd_sort(&a, c10::hip::getCurrentHIPStream().stream()), "swd_sort");
}

void bind_swd(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("kSwdCols") = (int64_t)kSwdCols;
  m.attr("kSwdMaxRows") = (int64_t)kSwdMaxRows;
  m.attr("kSwdMaxDirs") = (int64_t)kSwdMaxDirs;
  m.def("swd_rows", &swd_rows, py::arg("real"), py::arg("fake"), py::arg("dirs"), py::arg("proj"), py::arg("out"));
  m.def("swd_project", &swd_project, py::arg("real"), py::arg("fake"), py::arg("dirs"), py::arg("proj"));
  m.def("swd_sort", &swd_sort, py::arg("na"), py::arg("nb"), py::arg("proj"), py::arg("out"));
}

}  // namespace mdt
