// Data-set ops on device-resident splits. binarize_rows (csrc/kernels/binarize.hip):
// rewrite a compact [n, D] buffer of {0, 1} from the grey-level rows X[idx] in
// place, once per epoch, so the trainers' bound pointers and captured step
// graphs stay valid.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>
#include <string>

#include "../kernels/binarize.h"

namespace mdt {

static const char* binarize_reason(int rc) {
  switch (rc) {
    case 1: return "mode must be threshold | static | dynamic and split 0 | 1";
    case 2: return "needs n >= 0, D >= 1 and a data set of at least one row";
    case 3: return "ceil(D/4) exceeds the 2^32 range of the pixel-group counter word";
    case 4: return "the data set exceeds the 2^31 rows an int32 row index (and the 32-bit row counter word) can name";
    case 5: return "n*D exceeds the limit of 2^62 elements";
    case 6: return "missing buffer";
    default: return "launch failed";
  }
}

static void binarize_rc(int rc) {
  if (rc == 0) return;
  const std::string msg = std::string("mdt: binarize_rows: ") + binarize_reason(rc) + " (code " + std::to_string(rc) + ")";
  if (rc >= 1 && rc <= 5) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}

static int binarize_mode(const std::string& mode) {
  if (mode == "threshold") return kBinThreshold;
  if (mode == "static" || mode == "dynamic") return kBinBernoulli;
  throw std::invalid_argument("mdt: binarize_rows: unknown mode '" + mode + "' (threshold | static | dynamic)");
}

// The shape domain alone (no tensors): raises what binarize_rows would.
static void binarize_check(int64_t n, int64_t D, int64_t N, const std::string& mode, int64_t split) {
  binarize_rc(mdt_binarize_check(n, D, N, binarize_mode(mode), split == 0 ? 0 : split == 1 ? 1 : -1));
}

// out[i, :] = b(X[idx[i], :]) on the current stream, no host sync (graph-capturable).
// static and dynamic differ only in the epoch the caller passes (static: 0).
static void binarize_rows(const at::Tensor& X, const at::Tensor& idx, at::Tensor out, int64_t seed, int64_t epoch,
                          int64_t split, const std::string& mode) {
  const int m = binarize_mode(mode);
  TORCH_CHECK(X.is_cuda() && X.scalar_type() == torch::kFloat32 && X.dim() == 2 && X.is_contiguous(),
              "binarize_rows: X must be a contiguous CUDA float32 [N, D] tensor");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt32 && idx.dim() == 1 && idx.is_contiguous() &&
                  idx.device() == X.device(),
              "binarize_rows: idx must be a contiguous CUDA int32 vector on X's device");
  const int64_t n = idx.numel(), N = X.size(0), D = X.size(1);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kFloat32 && out.is_contiguous() && out.dim() == 2 &&
                  out.size(0) == n && out.size(1) == D && out.device() == X.device(),
              "binarize_rows: out must be a contiguous CUDA float32 [len(idx), D] tensor on X's device");
  TORCH_CHECK(epoch >= 0 && epoch <= 0xffffffffll, "binarize_rows: epoch must fit the 32-bit epoch counter word");
  binarize_rc(mdt_binarize_check(n, D, N, m, split == 0 ? 0 : split == 1 ? 1 : -1));
  // dynamic needs the probabilities again next epoch: out may not overwrite any of X
  const char* xb = static_cast<const char*>(X.data_ptr());
  const char* ob = static_cast<const char*>(out.data_ptr());
  const bool overlap = n > 0 && ob < xb + (size_t)N * D * 4 && xb < ob + (size_t)n * D * 4;
  if (overlap) throw std::invalid_argument("mdt: binarize_rows: out aliases X (the grey levels are needed again next epoch)");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  BinarizeArgs a;
  std::memset(&a, 0, sizeof(a));
  a.X = X.data_ptr<float>();
  a.idx = idx.data_ptr<int32_t>();
  a.out = out.data_ptr<float>();
  a.n = n; a.D = D; a.N = N;
  a.seed_lo = (uint32_t)((uint64_t)seed & 0xffffffffu);
  a.seed_hi = (uint32_t)((uint64_t)seed >> 32);
  a.epoch = (uint32_t)epoch;
  a.split = (uint32_t)split;
  a.mode = m;
  binarize_rc(mdt_binarize_rows(&a, c10::hip::getCurrentHIPStream().stream()));
}

void bind_data(pybind11::module& m) {
  namespace py = pybind11;
  m.attr("BINARIZE_TAG") = (int64_t)kBinTag;
  m.def("binarize_check", &binarize_check, py::arg("n"), py::arg("D"), py::arg("N"), py::arg("mode"), py::arg("split"));
  m.def("binarize_rows", &binarize_rows, py::arg("X"), py::arg("idx"), py::arg("out"), py::arg("seed"),
        py::arg("epoch"), py::arg("split"), py::arg("mode"));
}

}  // namespace mdt
