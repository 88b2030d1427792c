// Weight averaging (csrc/kernels/ema.hip): the entry points both trainers and
// the kernel tests use. Both launch on the current stream without a host sync
// (graph-capturable).
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../kernels/ema.h"

namespace mdt {

namespace {
const char* ema_reason(int rc) {
  switch (rc) {
    case 1: return "n must be >= 1";
    case 2: return "missing buffer";
    case 3: return "decay must be in [0, 1) and t >= 1";
    case 5: return "the two buffers overlap";
    default: return "launch failed";
  }
}

void ema_rc(int rc, const char* what) {
  if (rc == 0) return;
  const std::string msg = std::string("mdt: ") + what + ": " + ema_reason(rc) + " (code " + std::to_string(rc) + ")";
  if (rc == 1 || rc == 3 || rc == 5) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}

bool f32_vec(const at::Tensor& t, int64_t need) {
  return t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() >= need;
}
}  // namespace

// e[:n] <- e + (1 - d_t) (p - e), d_t = min(decay, (1 + t) / (10 + t)). The step t and the decay
// come from the trial's device buffers (`state`: TrainState.step, `hparams`: HParams.ema_decay) or,
// for kernel-level tests, from the explicit pair (`decay`, `t`).
void ema_update(at::Tensor e, const at::Tensor& p, int64_t n, const c10::optional<at::Tensor>& state,
                const c10::optional<at::Tensor>& hparams, c10::optional<double> decay, c10::optional<int64_t> t) {
  TORCH_CHECK_VALUE(n >= 1, "ema_update: n must be >= 1, got ", n);
  TORCH_CHECK(f32_vec(e, n) && f32_vec(p, n) && e.device() == p.device(),
              "ema_update: e and p must be contiguous CUDA float32 tensors of >= n elements on one device");
  EmaArgs a;
  std::memset(&a, 0, sizeof(a));
  a.e = e.data_ptr<float>();
  a.p = p.data_ptr<float>();
  a.n = n;
  const bool dev = state.has_value() && state->defined();
  if (dev) {
    TORCH_CHECK(!decay.has_value() && !t.has_value(), "ema_update: give (state, hparams) or (decay, t), not both");
    TORCH_CHECK(hparams.has_value() && hparams->defined(), "ema_update: state needs hparams");
    TORCH_CHECK(state->is_cuda() && state->device() == e.device() &&
                    state->numel() * state->element_size() >= (int64_t)sizeof(TrainState),
                "ema_update: state buffer too small or on another device");
    TORCH_CHECK(hparams->is_cuda() && hparams->device() == e.device() &&
                    hparams->numel() * hparams->element_size() >= (int64_t)sizeof(HParams),
                "ema_update: hparams buffer too small or on another device");
    a.st = reinterpret_cast<const TrainState*>(state->data_ptr());
    a.hp = reinterpret_cast<const HParams*>(hparams->data_ptr());
  } else {
    TORCH_CHECK(decay.has_value() && t.has_value(), "ema_update: needs (state, hparams) or (decay, t)");
    TORCH_CHECK_VALUE(std::isfinite(*decay) && *decay >= 0.0 && *decay < 1.0, "ema_update: decay must be in [0, 1), got ",
                      *decay);
    TORCH_CHECK_VALUE(*t >= 1, "ema_update: t is the 1-based optimizer step, got ", *t);
    a.decay = *decay;
    a.t = *t;
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(e.device());
  ema_rc(mdt_ema_update(&a, c10::hip::getCurrentHIPStream().stream()), "ema_update");
}

// a[:n] <-> b[:n] in place
void arena_swap(at::Tensor a, at::Tensor b, int64_t n) {
  TORCH_CHECK_VALUE(n >= 1, "arena_swap: n must be >= 1, got ", n);
  TORCH_CHECK(f32_vec(a, n) && f32_vec(b, n) && a.device() == b.device(),
              "arena_swap: a and b must be contiguous CUDA float32 tensors of >= n elements on one device");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(a.device());
  ema_rc(mdt_arena_swap(a.data_ptr<float>(), b.data_ptr<float>(), n, c10::hip::getCurrentHIPStream().stream()),
         "arena_swap");
}

void bind_ema(pybind11::module& m) {
  namespace py = pybind11;
  m.def("ema_update", &ema_update, py::arg("e"), py::arg("p"), py::arg("n"), py::arg("state") = py::none(),
        py::arg("hparams") = py::none(), py::arg("decay") = py::none(), py::arg("t") = py::none());
  m.def("arena_swap", &arena_swap, py::arg("a"), py::arg("b"), py::arg("n"));
  // 1 - d_t as the kernel forms it (a float): the CPU step and the tests' oracles share the ramp
  m.def("ema_omd", [](double decay, int64_t t) { return (double)ema_omd(decay, (long long)t); }, py::arg("decay"),
        py::arg("t"));
}

}  // namespace mdt
