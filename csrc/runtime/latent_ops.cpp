// Latent report pass (csrc/kernels/vae_latent.hip): device state, workspaces
// and the model-agnostic entry points shared by both trainers. The MLP-VAE's
// per-batch encoder call lives in MlpVaeEngine (vae_engine.cpp).
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cstring>
#include <stdexcept>

#include "../kernels/vae_latent.h"
#include "vae_engine.h"

namespace mdt {

static inline int64_t align64(int64_t v) { return (v + 63) / 64 * 64; }

static const char* latent_reason(int rc) {
  switch (rc) {
    case 1: return "Z must be in [1, 64]";
    case 2: return "n must be >= 1";
    case 3: return "n*Z exceeds the 2^32 Philox counter range of one pass";
    case 4: return "splits must be in [1, min(64, ceil(n/16))]";
    case 5: return "missing buffer";
    default: return "launch failed";
  }
}

static void latent_rc(int rc, const char* what) {
  if (rc == 0) return;
  const std::string msg = std::string("mdt: ") + what + ": " + latent_reason(rc) + " (code " + std::to_string(rc) + ")";
  if (rc >= 1 && rc <= 4) throw std::invalid_argument(msg);
  throw std::runtime_error(msg);
}

// The domain of the pass, before any size is computed from the arguments.
static void latent_domain(int64_t n, int64_t Z, int64_t splits) {
  LatentArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = n;
  a.Z = (int)std::max<int64_t>(std::min<int64_t>(Z, 1 << 20), -1);
  a.splits = (int)std::max<int64_t>(std::min<int64_t>(splits, 1 << 20), -1);
  int rc = mdt_latent_check(&a);
  if (n > (1ll << 32)) rc = 3;  // before the product can wrap
  if (rc >= 1 && rc <= 4) latent_rc(rc, "latent report");
}

at::Tensor latent_state_new(int64_t device_index) {
  auto bopt = torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA, device_index);
  return torch::zeros({align64((int64_t)sizeof(LatentState))}, bopt);
}

void latent_state_begin(at::Tensor state, int64_t nbatches) {
  TORCH_CHECK(nbatches > 0, "latent pass: nbatches must be positive");
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == torch::kUInt8 && state.numel() >= (int64_t)sizeof(LatentState),
              "latent pass: state must come from latent_state_new");
  state.zero_();
  TrainState h;
  std::memset(&h, 0, sizeof(h));
  h.nbatches = (int32_t)nbatches;
  h.b1pow = h.b2pow = 1.0;
  h.sched_off = 1;  // no schedule enters the pass (the encoder's first kernel still advances the step there)
  auto cpu = torch::empty({(int64_t)offsetof(TrainState, loss_hist)}, torch::kUInt8);
  std::memcpy(cpu.data_ptr(), &h, offsetof(TrainState, loss_hist));
  state.narrow(0, 0, offsetof(TrainState, loss_hist)).copy_(cpu);
}

// {kl, mi, tc, dwkl, sampled_kl, step (batches begun), cursor}
std::vector<double> latent_state_read(const at::Tensor& state) {
  auto cpu = state.to(torch::kCPU);
  const uint8_t* p = cpu.data_ptr<uint8_t>();
  TrainState h;
  std::memcpy(&h, p, offsetof(TrainState, loss_hist));
  double t[5];
  std::memcpy(t, p + offsetof(LatentState, kl), sizeof(t));
  return {t[0], t[1], t[2], t[3], t[4], (double)h.step, (double)h.cursor};
}

// An HParams image that carries only the Philox key (kernel tests without a trainer).
static at::Tensor latent_hparams(int64_t seed, int64_t device_index) {
  HParams h;
  std::memset(&h, 0, sizeof(h));
  h.seed_lo = (uint32_t)((uint64_t)seed & 0xffffffffu);
  h.seed_hi = (uint32_t)((uint64_t)seed >> 32);
  auto cpu = torch::zeros({align64((int64_t)sizeof(HParams))}, torch::kUInt8);
  std::memcpy(cpu.data_ptr(), &h, sizeof(h));
  return cpu.to(torch::Device(torch::kCUDA, device_index));
}

static int64_t latent_default_splits(int64_t n) {
  TORCH_CHECK(n >= 1, "latent report: n must be >= 1");
  return lat_splits(n);
}

namespace {
// float32 workspace: every segment starts on a 256-byte boundary
struct WsLayout {
  int64_t eps, z, pk, lq_cond, lp, lq_joint, lq_marg, acc_m, acc_s, kl_per_dim, mu_var, post_var, total;
  int64_t stat, part, total_d;
  WsLayout(int64_t n, int64_t Z, int64_t splits) {
    const int64_t zt = lat_zt((int)Z);
    int64_t o = 0;
    auto seg = [&](int64_t numel) { const int64_t at = o; o = align64(o + numel); return at; };
    eps = seg(n * Z); z = seg(n * Z); pk = seg(n * zt * 4);
    lq_cond = seg(n); lp = seg(n); lq_joint = seg(n); lq_marg = seg(n);
    acc_m = seg(splits * (zt + 1) * n); acc_s = seg(splits * (zt + 1) * n);
    kl_per_dim = seg(Z); mu_var = seg(Z); post_var = seg(Z);
    total = o;
    stat = 0;
    part = lat_cdiv(n, kLatPrepRows) * 4 * Z;
    total_d = part + lat_cdiv(n, kLatFinRows) * 4;
  }
};
}  // namespace

// (float32 elements, float64 elements) of the two workspace tensors of a pass
static std::vector<int64_t> latent_ws_numel(int64_t n, int64_t Z, c10::optional<int64_t> splits) {
  const int64_t S = splits.has_value() ? *splits : (n >= 1 ? lat_splits(n) : 1);
  latent_domain(n, Z, S);
  const WsLayout L(n, Z, S);
  return {L.total, L.total_d};
}

// A view of one result buffer of the float32 workspace.
static at::Tensor latent_ws_view(const at::Tensor& wsf, int64_t n, int64_t Z, c10::optional<int64_t> splits,
                                 const std::string& name) {
  const int64_t S = splits.has_value() ? *splits : (n >= 1 ? lat_splits(n) : 1);
  latent_domain(n, Z, S);
  const WsLayout L(n, Z, S);
  TORCH_CHECK(wsf.scalar_type() == torch::kFloat32 && wsf.numel() >= L.total, "latent_ws_view: workspace too small");
  if (name == "eps") return wsf.narrow(0, L.eps, n * Z).view({n, Z});
  if (name == "z") return wsf.narrow(0, L.z, n * Z).view({n, Z});
  if (name == "lq_cond") return wsf.narrow(0, L.lq_cond, n);
  if (name == "lp") return wsf.narrow(0, L.lp, n);
  if (name == "lq_joint") return wsf.narrow(0, L.lq_joint, n);
  if (name == "lq_marg") return wsf.narrow(0, L.lq_marg, n);
  if (name == "kl_per_dim") return wsf.narrow(0, L.kl_per_dim, Z);
  if (name == "mu_var") return wsf.narrow(0, L.mu_var, Z);
  if (name == "post_var") return wsf.narrow(0, L.post_var, Z);
  TORCH_CHECK(false, "latent_ws_view: unknown buffer ", name);
}

static void latent_run(const at::Tensor& mulv_rows, int64_t n, int64_t Z, at::Tensor state, const at::Tensor& hparams,
                       const std::vector<at::Tensor>& ws, c10::optional<int64_t> splits, bool pair_only) {
  const int64_t S = splits.has_value() ? *splits : (n >= 1 ? lat_splits(n) : 1);
  latent_domain(n, Z, S);
  TORCH_CHECK(mulv_rows.is_cuda() && mulv_rows.scalar_type() == torch::kFloat32 && mulv_rows.is_contiguous() &&
                  mulv_rows.numel() >= n * 2 * Z,
              "latent_report: mulv_rows must be a contiguous CUDA float32 tensor of >= n*2Z elements");
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == torch::kUInt8 && state.numel() >= (int64_t)sizeof(LatentState),
              "latent_report: state must come from latent_state_new");
  TORCH_CHECK(hparams.is_cuda() && hparams.numel() * hparams.element_size() >= (int64_t)sizeof(HParams),
              "latent_report: hparams buffer too small");
  const WsLayout L(n, Z, S);
  TORCH_CHECK(ws.size() == 2 && ws[0].is_cuda() && ws[0].scalar_type() == torch::kFloat32 && ws[0].is_contiguous() &&
                  ws[0].numel() >= L.total && ws[1].is_cuda() && ws[1].scalar_type() == torch::kFloat64 &&
                  ws[1].is_contiguous() && ws[1].numel() >= L.total_d,
              "latent_report: workspaces must be [float32, float64] CUDA tensors of latent_ws_numel(n, Z, splits) elements");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(mulv_rows.device());
  LatentArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = n; a.Z = (int)Z; a.splits = (int)S;
  a.mulv = mulv_rows.data_ptr<float>();
  float* f = ws[0].data_ptr<float>();
  a.eps = f + L.eps; a.z = f + L.z; a.pk = reinterpret_cast<float4*>(f + L.pk);
  a.lq_cond = f + L.lq_cond; a.lp = f + L.lp; a.lq_joint = f + L.lq_joint; a.lq_marg = f + L.lq_marg;
  a.acc_m = f + L.acc_m; a.acc_s = f + L.acc_s;
  a.kl_per_dim = f + L.kl_per_dim; a.mu_var = f + L.mu_var; a.post_var = f + L.post_var;
  double* d = ws[1].data_ptr<double>();
  a.stat = d + L.stat; a.part = d + L.part;
  a.lst = reinterpret_cast<LatentState*>(state.data_ptr<uint8_t>());
  a.hp = reinterpret_cast<const HParams*>(hparams.data_ptr());
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  latent_rc(pair_only ? mdt_latent_pair(&a, stream) : mdt_latent_report(&a, stream), "latent report");
}

// The once-per-pass launches over rows mulv_rows[:n]: prep, pair, finish, fold.
// Results: latent_state_read(state) and the workspace views.
static void latent_report(const at::Tensor& mulv_rows, int64_t n, int64_t Z, at::Tensor state, const at::Tensor& hparams,
                          const std::vector<at::Tensor>& workspaces, c10::optional<int64_t> splits) {
  latent_run(mulv_rows, n, Z, state, hparams, workspaces, splits, false);
}

// latent_pair_k alone on the operands a latent_report left in the workspaces (timing).
static void latent_pair(const at::Tensor& mulv_rows, int64_t n, int64_t Z, at::Tensor state, const at::Tensor& hparams,
                        const std::vector<at::Tensor>& workspaces, c10::optional<int64_t> splits) {
  latent_run(mulv_rows, n, Z, state, hparams, workspaces, splits, true);
}

void latent_collect(const at::Tensor& mulv, int64_t M, int64_t B, int64_t Z, at::Tensor rows, at::Tensor state) {
  TORCH_CHECK(mulv.is_cuda() && mulv.scalar_type() == torch::kFloat32 && mulv.is_contiguous() &&
                  mulv.numel() >= M * 2 * Z,
              "latent_collect: mulv must be a contiguous CUDA float32 tensor of >= M*2Z elements");
  TORCH_CHECK(rows.is_cuda() && rows.scalar_type() == torch::kFloat32 && rows.is_contiguous() && Z >= 1 &&
                  rows.numel() % (2 * Z) == 0,
              "latent_collect: rows must be a contiguous CUDA float32 [rows, 2Z] tensor");
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == torch::kUInt8 && state.numel() >= (int64_t)sizeof(LatentState),
              "latent_collect: state must come from latent_state_new");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(mulv.device());
  latent_rc(mdt_latent_collect(mulv.data_ptr<float>(), (int)M, (int)B, (int)Z, rows.data_ptr<float>(),
                               rows.numel() / (2 * Z), state.data_ptr(), c10::hip::getCurrentHIPStream().stream()),
            "latent collect");
}

void bind_latent(pybind11::module& m) {
  namespace py = pybind11;
  m.def("latent_state_new", &latent_state_new, py::arg("device_index"));
  m.def("latent_state_begin", &latent_state_begin, py::arg("state"), py::arg("nbatches"));
  m.def("latent_state_read", &latent_state_read, py::arg("state"));
  m.def("latent_hparams", &latent_hparams, py::arg("seed"), py::arg("device_index"));
  m.def("latent_default_splits", &latent_default_splits, py::arg("n"));
  m.def("latent_ws_numel", &latent_ws_numel, py::arg("n"), py::arg("Z"), py::arg("splits") = py::none());
  m.def("latent_ws_view", &latent_ws_view, py::arg("wsf"), py::arg("n"), py::arg("Z"), py::arg("splits"),
        py::arg("name"));
  m.def("latent_report", &latent_report, py::arg("mulv_rows"), py::arg("n"), py::arg("Z"), py::arg("state"),
        py::arg("hparams"), py::arg("workspaces"), py::arg("splits") = py::none());
  m.def("latent_pair", &latent_pair, py::arg("mulv_rows"), py::arg("n"), py::arg("Z"), py::arg("state"),
        py::arg("hparams"), py::arg("workspaces"), py::arg("splits") = py::none());
  m.def("latent_collect", &latent_collect, py::arg("mulv"), py::arg("M"), py::arg("B"), py::arg("Z"), py::arg("rows"),
        py::arg("state"));
}

}  // namespace mdt
