// Total-correlation penalty of a training batch (csrc/kernels/vae_tc.hip): the
// workspace layout and the entry points both trainers and the kernel tests use.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>

#include "../kernels/vae_tc.h"

namespace mdt {

namespace {
inline int64_t align64(int64_t v) { return (v + 63) / 64 * 64; }

const char* tc_reason(int rc) {
  switch (rc) {
    case 1: return "Z must be in [1, 64]";
    case 2: return "M must be in [1, 4096]";
    case 4: return "splits must be in [1, min(64, ceil(M/16))]";
    case 5: return "missing buffer";
    default: return "launch failed";
  }
}

void tc_rc(int rc, const char* what) {
  if (rc == 0) return;
  const std::string msg = std::string("mdt: ") + what + ": " + tc_reason(rc) + " (code " + std::to_string(rc) + ")";
  if (rc >= 1 && rc <= 4) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}

// The domain, before any size is computed from the arguments.
int64_t tc_domain(int64_t M, int64_t Z, c10::optional<int64_t> splits) {
  if (Z < 1 || Z > kLatMaxZ) tc_rc(1, "tc penalty");
  if (M < 1 || M > kMaxBatch) tc_rc(2, "tc penalty");
  const int64_t S = splits.has_value() ? *splits : tc_splits((int)M, (int)Z);
  if (S < 1 || S > kLatMaxSplits || S > lat_cdiv(M, kLatJTile)) tc_rc(4, "tc penalty");
  return S;
}

// float32 workspace: every segment starts on a 256-byte boundary
struct TcLayout {
  int64_t z, pk, acc_m, acc_s, lse_d, lse_j, gz, gmu, glv, csum, total;
  TcLayout(int64_t M, int64_t Z, int64_t S) {
    const int64_t zt = lat_zt((int)Z);
    int64_t o = 0;
    auto seg = [&](int64_t numel) { const int64_t at = o; o = align64(o + numel); return at; };
    z = seg(M * Z); pk = seg(M * zt * 4);
    acc_m = seg(S * (zt + 1) * M); acc_s = seg(S * (zt + 1) * M);
    lse_d = seg(M * zt); lse_j = seg(M);
    gz = seg(S * M * zt); gmu = seg(S * M * zt); glv = seg(S * M * zt);
    csum = seg(S * M * (zt + 1));
    total = o;
  }
};

int64_t tc_default_splits(int64_t M, int64_t Z) { return tc_domain(M, Z, c10::nullopt); }

int64_t tc_ws_numel(int64_t M, int64_t Z, c10::optional<int64_t> splits) {
  return TcLayout(M, Z, tc_domain(M, Z, splits)).total;
}

bool f32_buf(const at::Tensor& t, int64_t need) {
  return t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() >= need;
}
}  // namespace

// Value and gradient of the step's penalty over rows mulv[:M], eps[:M].
// `stage`: 0 everything, 1 forward + backward (what needs only mulv and eps),
// 2 the fold alone (after d[mu|lv] exists when it is added in place).
// The weight is TrainState.tc_t of `state` (which also accumulates epoch_tc), or
// the one-element `weight` tensor.
void tc_penalty(const at::Tensor& mulv, const at::Tensor& eps, int64_t M, int64_t Z, at::Tensor ws, at::Tensor value,
                const c10::optional<at::Tensor>& state, const c10::optional<at::Tensor>& weight,
                const c10::optional<at::Tensor>& add_out, const c10::optional<at::Tensor>& dmulv,
                const c10::optional<at::Tensor>& dmulv16, c10::optional<int64_t> splits, int64_t stage) {
  const int64_t S = tc_domain(M, Z, splits);
  const TcLayout L(M, Z, S);
  TORCH_CHECK(f32_buf(mulv, M * 2 * Z), "tc_penalty: mulv must be a contiguous CUDA float32 tensor of >= M*2Z elements");
  TORCH_CHECK(f32_buf(eps, M * Z), "tc_penalty: eps must be a contiguous CUDA float32 tensor of >= M*Z elements");
  TORCH_CHECK(f32_buf(ws, L.total), "tc_penalty: the workspace needs tc_ws_numel(M, Z, splits) float32 elements");
  TORCH_CHECK(value.is_cuda() && value.scalar_type() == torch::kFloat64 && value.numel() >= 1,
              "tc_penalty: value must be a CUDA float64 tensor");
  TORCH_CHECK(stage >= 0 && stage <= 2, "tc_penalty: stage must be 0, 1 or 2");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(mulv.device());
  TcArgs a;
  std::memset(&a, 0, sizeof(a));
  a.M = (int)M; a.Z = (int)Z; a.splits = (int)S;
  a.mulv = mulv.data_ptr<float>();
  a.eps = eps.data_ptr<float>();
  float* f = ws.data_ptr<float>();
  a.z = f + L.z; a.pk = reinterpret_cast<float4*>(f + L.pk);
  a.acc_m = f + L.acc_m; a.acc_s = f + L.acc_s; a.lse_d = f + L.lse_d; a.lse_j = f + L.lse_j;
  a.gz = f + L.gz; a.gmu = f + L.gmu; a.glv = f + L.glv; a.csum = f + L.csum;
  a.value = value.data_ptr<double>();
  if (state.has_value() && state->defined()) {
    TORCH_CHECK(state->is_cuda() && state->numel() * state->element_size() >= (int64_t)sizeof(TrainState),
                "tc_penalty: state buffer too small");
    a.st = reinterpret_cast<TrainState*>(state->data_ptr());
    a.tcw = &a.st->tc_t;
  } else {
    TORCH_CHECK(weight.has_value() && f32_buf(*weight, 1), "tc_penalty: needs a state or a CUDA float32 weight");
    a.tcw = weight->data_ptr<float>();
  }
  if (add_out.has_value() && add_out->defined()) {
    TORCH_CHECK(f32_buf(*add_out, M * 2 * Z), "tc_penalty: add_out must hold M*2Z float32 elements");
    a.add_out = add_out->data_ptr<float>();
  }
  if (dmulv.has_value() && dmulv->defined()) {
    TORCH_CHECK(f32_buf(*dmulv, M * 2 * Z), "tc_penalty: dmulv must hold M*2Z float32 elements");
    a.dmulv = dmulv->data_ptr<float>();
    if (dmulv16.has_value() && dmulv16->defined()) {
      TORCH_CHECK(dmulv16->is_cuda() && dmulv16->scalar_type() == torch::kBFloat16 && dmulv16->is_contiguous() &&
                      dmulv16->numel() >= M * 2 * Z,
                  "tc_penalty: dmulv16 must hold M*2Z bfloat16 elements");
      a.dmulv16 = dmulv16->data_ptr();
    }
  }
  TORCH_CHECK(stage == 1 || a.add_out || a.dmulv, "tc_penalty: the fold needs add_out or dmulv");
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  if (stage != 2) {
    tc_rc(mdt_tc_forward(&a, stream), "tc forward");
    tc_rc(mdt_tc_backward(&a, stream), "tc backward");
  }
  if (stage != 1) tc_rc(mdt_tc_fold(&a, stream), "tc fold");
}

void bind_tc(pybind11::module& m) {
  namespace py = pybind11;
  m.def("tc_default_splits", &tc_default_splits, py::arg("M"), py::arg("Z"));
  m.def("tc_ws_numel", &tc_ws_numel, py::arg("M"), py::arg("Z"), py::arg("splits") = py::none());
  m.def("tc_penalty", &tc_penalty, py::arg("mulv"), py::arg("eps"), py::arg("M"), py::arg("Z"), py::arg("ws"),
        py::arg("value"), py::arg("state") = py::none(), py::arg("weight") = py::none(),
        py::arg("add_out") = py::none(), py::arg("dmulv") = py::none(), py::arg("dmulv16") = py::none(),
        py::arg("splits") = py::none(), py::arg("stage") = 0);
}

}  // namespace mdt
