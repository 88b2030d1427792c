// Torch bindings of the conv-VAE kernels (csrc/kernels/conv_bf16.hip) and a
// device-resident trial state (same TrainState / HParams structs as the MLP
// engine) for generic trainers.
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <array>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <unordered_map>
#include <variant>
#include <vector>

#include "../kernels/conv28_slots.h"
#include "../kernels/conv_launch.h"

namespace mdt {

// A recorded launch for the horizontally fused job kernels (conv_jobs.hip):
// the op bindings below take an optional Job; when given, they validate and
// RECORD the launch into it instead of issuing it. `post` is the dependent
// follow-up (split-K combine) to launch after the job's own kernel.
struct Job {
  JobBlob main{}, post{};
  int kind() const { return main.kind; }
  bool has_post() const { return post.kind != 0; }
};

static hipStream_t cur() { return c10::hip::getCurrentHIPStream().stream(); }
static void rc(int r, const char* w) { TORCH_CHECK(r == 0, "mdt: ", w, " failed (", r, ")"); }
static const void* opt_ptr(const c10::optional<at::Tensor>& t) {
  return (t.has_value() && t->defined()) ? t->data_ptr() : nullptr;
}

static ConvDesc desc(const std::vector<int64_t>& v) {
  TORCH_CHECK(v.size() == 11, "conv desc needs 11 ints (N,H,W,C,OH,OW,CO,KH,KW,S,P)");
  for (auto x : v) TORCH_CHECK(x >= 0 && x < (1 << 30), "conv desc value out of range");
  return ConvDesc{(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5],
                  (int)v[6], (int)v[7], (int)v[8], (int)v[9], (int)v[10]};
}

static void check_bf16(const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 && t.is_contiguous(), n,
              " must be a contiguous CUDA bfloat16 tensor");
}
static void check_f32(const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous(), n,
              " must be a contiguous CUDA float32 tensor");
}
static void check_min(const c10::optional<at::Tensor>& t, int64_t n, const char* w) {
  if (t.has_value() && t->defined()) TORCH_CHECK(t->numel() >= n, w, " too small: ", t->numel(), " < ", n);
}

// Argument checks of the small step kernels (conv_bf16.hip), which take raw
// pointers: `t` is a contiguous tensor of dtype `ty` with >= n elements on the
// device of `ref` (the op's first tensor). A bad call stops here, on the host.
static void check_buf(const at::Tensor& t, c10::ScalarType ty, int64_t n, const at::Tensor& ref, const char* op,
                      const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.scalar_type() == ty && t.is_contiguous(), op, ": ", name,
              " must be a contiguous CUDA tensor of dtype ", ty);
  TORCH_CHECK(t.get_device() == ref.get_device(), op, ": ", name, " is on another device than the op's first tensor");
  TORCH_CHECK(t.numel() >= n, op, ": ", name, " too small: ", t.numel(), " < ", n);
}
static void check_buf(const c10::optional<at::Tensor>& t, c10::ScalarType ty, int64_t n, const at::Tensor& ref,
                      const char* op, const char* name) {
  if (t.has_value() && t->defined()) check_buf(*t, ty, n, ref, op, name);
}
// a TrialState device buffer (train_state / eval_state / hparams) of >= `bytes` bytes
static void check_blob(const at::Tensor& t, size_t bytes, const at::Tensor& ref, const char* op, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.is_contiguous() && t.get_device() == ref.get_device() &&
                  t.numel() * t.element_size() >= (int64_t)bytes,
              op, ": ", name, " must be a TrialState buffer (>= ", bytes, " bytes) on the op's device");
}
// B x Z latent extents: positive, and the element index fits the 32-bit Philox counter word / int arithmetic
static void check_bz(int64_t B, int64_t Z, const char* op) {
  const int64_t lim = int64_t(1) << 30;
  TORCH_CHECK(B >= 1 && Z >= 1 && B < lim && Z < lim && B * 2 * Z < 2 * lim, op,
              ": need B >= 1, Z >= 1 and 2 B Z < 2^31, got B = ", B, ", Z = ", Z);
}
static int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// fwd: the forward-pass call of this geometry (may select the direct kernel
// where the backward-data call of the same geometry keeps the fusable one)
// A plan goes to Python as a struct sequence (a C-level named tuple) made from
// ONE field list: read by name (ops/conv_plans.py), and still a sequence in the
// order of the list.
template <class P>
struct PlanField {
  const char* name;
  int P::*member;
};
static const PlanField<FwdPlan> kFwdPlanFields[] = {
    {"cfg", &FwdPlan::cfg},         {"bm", &FwdPlan::BM},         {"bn", &FwdPlan::BN},
    {"classes", &FwdPlan::classes}, {"m", &FwdPlan::M},           {"ncols", &FwdPlan::Ncols},
    {"k", &FwdPlan::K},             {"mtiles", &FwdPlan::mtiles}, {"ntiles", &FwdPlan::ntiles},
    {"ktiles", &FwdPlan::ktiles},   {"ksplit", &FwdPlan::ksplit}, {"colsum_rows", &FwdPlan::colsum_rows}};
static const PlanField<WgradPlan> kWgradPlanFields[] = {
    {"cfg", &WgradPlan::cfg},         {"bm", &WgradPlan::BM},         {"bn", &WgradPlan::BN},
    {"cotiles", &WgradPlan::cotiles}, {"ktiles", &WgradPlan::ktiles}, {"mtiles", &WgradPlan::mtiles},
    {"nsplit", &WgradPlan::nsplit},   {"mt_per_split", &WgradPlan::mt_per_split}};

template <class P, size_t N>
static pybind11::object plan_tuple(const char* type, const PlanField<P> (&fields)[N], const P& q) {
  static PyTypeObject* cls = [&] {  // made once per plan type, kept for the life of the process
    static PyStructSequence_Field f[N + 1] = {};
    for (size_t i = 0; i < N; ++i) f[i] = PyStructSequence_Field{fields[i].name, nullptr};
    static PyStructSequence_Desc d{type, nullptr, f, (int)N};
    return PyStructSequence_NewType(&d);
  }();
  TORCH_CHECK(cls != nullptr, "mdt: could not create the plan type ", type);
  PyObject* t = PyStructSequence_New(cls);
  for (size_t i = 0; i < N; ++i) PyStructSequence_SetItem(t, i, PyLong_FromLong(q.*fields[i].member));
  return pybind11::reinterpret_steal<pybind11::object>(t);
}

pybind11::object igemm_plan(int64_t mode, const std::vector<int64_t>& dv, bool allow_split, bool fwd) {
  FwdPlan q;
  rc(mdt_igemm_plan((int)mode, desc(dv), allow_split ? 1 : 0, fwd ? 1 : 0, &q), "igemm_plan (unsupported geometry)");
  return plan_tuple("_C.FwdPlan", kFwdPlanFields, q);
}

pybind11::object wgrad_plan(const std::vector<int64_t>& dv) {
  WgradPlan q;
  rc(mdt_wgrad_plan(desc(dv), &q), "wgrad_plan (unsupported geometry)");
  return plan_tuple("_C.WgradPlan", kWgradPlanFields, q);
}

// A job's blob, or null for a launch: the first argument of every op builder.
static JobBlob* blob(Job* job) { return job ? &job->main : nullptr; }

// mode 0: conv (fwd / convT bwd-data), mode 1: parity-class transposed conv
// (conv bwd-data / convT fwd; B16 = parity-ordered transposed weights).
void igemm(int64_t mode, const at::Tensor& A, const at::Tensor& B16, const std::vector<int64_t>& dv,
           const c10::optional<at::Tensor>& bias, bool relu, const c10::optional<at::Tensor>& y16,
           const c10::optional<at::Tensor>& y32, const c10::optional<at::Tensor>& omask,
           const c10::optional<at::Tensor>& colsum, const c10::optional<at::Tensor>& ws, Job* job, bool combine,
           const c10::optional<at::Tensor>& a_slab, int64_t a_ks, const c10::optional<at::Tensor>& a_bias,
           bool a_relu, const c10::optional<at::Tensor>& a_out16, bool fwd) {
  const ConvDesc d = desc(dv);
  TORCH_CHECK(A.is_cuda() && A.is_contiguous(), "A must be contiguous CUDA");
  const bool f32 = A.scalar_type() == torch::kFloat32;
  TORCH_CHECK(f32 || A.scalar_type() == torch::kBFloat16, "A must be f32 or bf16");
  check_bf16(B16, "B16");
  FwdPlan q;
  rc(mdt_igemm_plan((int)mode, d, ws.has_value() && ws->defined() ? 1 : 0, fwd ? 1 : 0, &q), "igemm_plan");
  TORCH_CHECK(!(fwd && job), "igemm: fwd calls have no job form");
  const int64_t classes = q.classes, M = q.M, Ncols = q.Ncols, K = q.K, ksplit = q.ksplit;
  const int64_t rows_total = classes * M;
  const int64_t a_need = mode == kModeConv ? (int64_t)d.N * d.H * d.W * d.C : (int64_t)d.N * d.OH * d.OW * d.CO;
  TORCH_CHECK(A.numel() >= a_need, "A too small: ", A.numel(), " < ", a_need);
  TORCH_CHECK(B16.numel() >= classes * Ncols * K, "B16 too small");
  check_min(y16, rows_total * Ncols, "y16");
  check_min(y32, rows_total * Ncols, "y32");
  check_min(omask, rows_total * Ncols, "omask");
  check_min(bias, Ncols, "bias");
  check_min(colsum, (int64_t)q.colsum_rows * Ncols, "colsum");
  if (ksplit > 1) check_min(ws, ksplit * M * Ncols, "ws");
  APro pro{};
  if (a_slab.has_value() && a_slab->defined()) {
    // A is formed from the producing layer's split-K partial slabs (see APro)
    TORCH_CHECK(!job, "igemm: the A prologue has no job form");
    TORCH_CHECK(a_bias.has_value() && a_bias->defined() && a_out16.has_value() && a_out16->defined(),
                "igemm: a_slab needs a_bias and a_out16");
    check_f32(*a_slab, "a_slab");
    check_bf16(*a_out16, "a_out16");
    TORCH_CHECK(a_ks >= 1 && a_slab->numel() >= a_ks * a_need, "a_slab too small");
    TORCH_CHECK(a_out16->numel() >= a_need, "a_out16 too small");
    const int64_t cin = a_bias->numel();
    TORCH_CHECK(cin % 8 == 0 && a_need % cin == 0, "a_bias length must divide the A row layout");
    pro = APro{(const float*)a_slab->data_ptr(), (const float*)a_bias->data_ptr(),
               a_out16->data_ptr(), (int)a_ks, a_relu ? 1 : 0, (int)cin, (long long)a_need};
  }
  rc(mdt_igemm(blob(job), job ? &job->post : nullptr, (int)mode, A.data_ptr(), f32, B16.data_ptr(), d,
               (const float*)opt_ptr(bias), relu, const_cast<void*>(opt_ptr(y16)), (float*)opt_ptr(y32),
               opt_ptr(omask), (float*)opt_ptr(colsum), (float*)opt_ptr(ws), combine ? 0 : 1, cur(),
               pro.slab ? &pro : nullptr, fwd ? 1 : 0),
     job ? "job_igemm" : "igemm");
}

// The 64-byte device buffer that hands one AdamC from the step kernel to the
// Adam epilogues of the next launch.
static float* adamc_ptr(const at::Tensor& t, int dev, const char* who) {
  TORCH_CHECK(t.is_cuda() && t.get_device() == dev && t.is_contiguous() && t.scalar_type() == torch::kFloat32 &&
                  t.numel() >= 16 && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              who, ": adamc must be a contiguous 16-B aligned f32 tensor of >= 16 elements on the launch's device");
  return t.data_ptr<float>();
}

// `adam` (jobs only) = [P, m, v, w16] arenas with `adam_off` the weight's arena
// offset and `adamc` the constants buffer: the job applies Adam to the weight
// in its epilogue instead of writing `out` (single m-split plans only).
void wgrad(const at::Tensor& G16, const at::Tensor& X, const std::vector<int64_t>& dv, at::Tensor out, Job* job,
           const std::vector<at::Tensor>& adam, int64_t adam_off, const c10::optional<at::Tensor>& adamc) {
  const ConvDesc d = desc(dv);
  check_bf16(G16, "G16");
  check_f32(out, "out");
  const bool f32 = X.scalar_type() == torch::kFloat32;
  TORCH_CHECK(X.is_cuda() && X.is_contiguous() && (f32 || X.scalar_type() == torch::kBFloat16), "X dtype/layout");
  WgradPlan q;
  rc(mdt_wgrad_plan(d, &q), "wgrad_plan");
  TORCH_CHECK(G16.numel() >= (int64_t)d.N * d.OH * d.OW * d.CO, "G16 too small");
  TORCH_CHECK(X.numel() >= (int64_t)d.N * d.H * d.W * d.C, "X too small");
  TORCH_CHECK(out.numel() >= (int64_t)q.nsplit * d.CO * d.KH * d.KW * d.C, "wgrad out too small for ", q.nsplit,
              " partial slabs");
  if (!adam.empty()) {
    const int64_t numel = (int64_t)d.CO * d.KH * d.KW * d.C;
    TORCH_CHECK(job != nullptr && !f32, "wgrad: the Adam epilogue exists for bf16 weight-gradient jobs only");
    TORCH_CHECK(adam.size() == 4 && adamc.has_value() && adamc->defined(), "wgrad: adam = [P, m, v, w16] and adamc");
    TORCH_CHECK(q.nsplit == 1, "wgrad: the Adam epilogue needs a single m-split plan, got ", q.nsplit);
    TORCH_CHECK(adam_off >= 0 && adam_off % 4 == 0 && numel % 4 == 0, "wgrad: adam_off and the weight size must be multiples of 4");
    const int dev = G16.get_device();
    for (int i = 0; i < 4; ++i) {
      TORCH_CHECK(adam[i].is_cuda() && adam[i].get_device() == dev && adam[i].is_contiguous() &&
                      adam[i].scalar_type() == (i < 3 ? torch::kFloat32 : torch::kBFloat16) &&
                      adam[i].numel() >= adam_off + numel && reinterpret_cast<uintptr_t>(adam[i].data_ptr()) % 16 == 0,
                  "wgrad: adam[", i, "] must be a contiguous 16-B aligned arena holding the weight at adam_off");
    }
    rc(mdt_job_wgrad_adam(&job->main, G16.data_ptr(), X.data_ptr(), f32, d, adam[0].data_ptr<float>() + adam_off,
                          adam[1].data_ptr<float>() + adam_off, adam[2].data_ptr<float>() + adam_off,
                          static_cast<char*>(adam[3].data_ptr()) + 2 * adam_off, adamc_ptr(*adamc, dev, "wgrad")),
       "job_wgrad_adam");
    return;
  }
  rc(mdt_wgrad(blob(job), G16.data_ptr(), X.data_ptr(), f32, d, out.data_ptr<float>(), cur()),
     job ? "job_wgrad" : "wgrad");
}

// Single-channel edge layers (conv_thin.hip): Wf is the f32 master weight
// [CO][KH][KW][1] (read with wave-uniform scalar loads).
void thin_conv(const at::Tensor& X, const at::Tensor& Wf, const std::vector<int64_t>& dv,
               const c10::optional<at::Tensor>& bias, bool relu, at::Tensor y16,
               const c10::optional<at::Tensor>& omask, const c10::optional<at::Tensor>& colsum, Job* job,
               const c10::optional<at::Tensor>& idx, const c10::optional<at::Tensor>& state,
               const c10::optional<at::Tensor>& hparams, int64_t B, const c10::optional<at::Tensor>& xb) {
  const ConvDesc d = desc(dv);
  const bool f32 = X.scalar_type() == torch::kFloat32;
  TORCH_CHECK(X.is_cuda() && X.is_contiguous() && (f32 || X.scalar_type() == torch::kBFloat16), "X dtype/layout");
  check_f32(Wf, "Wf");
  check_bf16(y16, "y16");
  const int64_t M = (int64_t)d.N * d.OH * d.OW;
  TORCH_CHECK(X.numel() >= (int64_t)d.N * d.H * d.W, "X too small");
  TORCH_CHECK(Wf.numel() >= (int64_t)d.CO * d.KH * d.KW, "Wf too small");
  TORCH_CHECK(y16.numel() >= M * d.CO, "y16 too small");
  check_min(omask, M * d.CO, "omask");
  check_min(colsum, (int64_t)mdt_thin_blocks(0, d) * d.CO, "colsum");
  check_min(bias, d.CO, "bias");
  const bool gather = idx.has_value() && idx->defined();
  if (gather) {
    TORCH_CHECK(idx->scalar_type() == torch::kInt32 && state.has_value() && B >= d.N, "thin_conv gather arguments");
    TORCH_CHECK(X.dim() == 2 && X.size(1) == (int64_t)d.H * d.W, "thin_conv gather: X must be [rows, H*W]");
  }
  check_min(xb, (int64_t)d.N * d.H * d.W, "xb");
  rc(mdt_thin_conv(blob(job), X.data_ptr(), f32, Wf.data_ptr<float>(), d, (const float*)opt_ptr(bias), relu,
                   y16.data_ptr(), opt_ptr(omask), (float*)opt_ptr(colsum), (const int*)opt_ptr(idx),
                   const_cast<void*>(opt_ptr(state)), opt_ptr(hparams), (int)B, (float*)opt_ptr(xb), cur()),
     job ? "job_thin_conv" : "thin_conv");
}

int64_t thin_blocks(bool tconv, const std::vector<int64_t>& dv) { return mdt_thin_blocks(tconv ? 1 : 0, desc(dv)); }

void thin_tconv(const at::Tensor& G16, const at::Tensor& Wf, const std::vector<int64_t>& dv,
                const c10::optional<at::Tensor>& bias, const c10::optional<at::Tensor>& y32,
                const c10::optional<at::Tensor>& X, const c10::optional<at::Tensor>& dlog16,
                const c10::optional<at::Tensor>& recon, const c10::optional<at::Tensor>& part,
                const c10::optional<at::Tensor>& gpart) {
  const ConvDesc d = desc(dv);
  check_bf16(G16, "G16");
  check_f32(Wf, "Wf");
  const int64_t npix = (int64_t)d.N * d.H * d.W;
  const int64_t nb = mdt_thin_blocks(1, d);
  TORCH_CHECK(G16.numel() >= (int64_t)d.N * d.OH * d.OW * d.CO, "G16 too small");
  TORCH_CHECK(Wf.numel() >= (int64_t)d.CO * d.KH * d.KW, "Wf too small");
  check_min(y32, npix, "y32");
  check_min(X, npix, "X");
  check_min(dlog16, npix, "dlog16");
  check_min(recon, npix, "recon");
  check_min(part, nb, "part");
  check_min(gpart, nb, "gpart");
  rc(mdt_thin_tconv(G16.data_ptr(), Wf.data_ptr<float>(), d, (const float*)opt_ptr(bias), (float*)opt_ptr(y32),
                    (const float*)opt_ptr(X), const_cast<void*>(opt_ptr(dlog16)), (float*)opt_ptr(recon),
                    (float*)opt_ptr(part), (float*)opt_ptr(gpart), cur()),
     "thin_tconv");
}

void colsum(const at::Tensor& G16, int64_t M, int64_t N, int64_t rows_per, at::Tensor slab, Job* job) {
  check_bf16(G16, "G16");
  check_f32(slab, "slab");
  // 8 bf16 columns (16 B) per thread; rows_per divides below
  const int64_t lim = int64_t(1) << 30;
  TORCH_CHECK(M >= 1 && M < lim && N >= 8 && N < lim && N % 8 == 0 && rows_per >= 1 && rows_per < lim &&
                  M * N < 2 * lim,
              "colsum: need M >= 1, N a positive multiple of 8 and rows_per >= 1, got M = ", M, ", N = ", N,
              ", rows_per = ", rows_per);
  TORCH_CHECK(slab.get_device() == G16.get_device(), "colsum: slab is on another device than G16");
  TORCH_CHECK(G16.numel() >= M * N, "G16 too small");
  TORCH_CHECK(slab.numel() >= ((M + rows_per - 1) / rows_per) * N, "colsum slab too small");
  rc(mdt_colsum(blob(job), G16.data_ptr(), (int)M, (int)N, (int)rows_per, slab.data_ptr<float>(), cur()),
     job ? "job_colsum" : "colsum");
}

void reparam(const at::Tensor& mulv, at::Tensor eps, at::Tensor z16, const c10::optional<at::Tensor>& z32, int64_t B,
             int64_t Z, const at::Tensor& state, const at::Tensor& hparams, int64_t stream, at::Tensor kld_part) {
  check_bz(B, Z, "reparam");
  check_buf(mulv, torch::kFloat32, B * 2 * Z, mulv, "reparam", "mulv");
  check_buf(eps, torch::kFloat32, B * Z, mulv, "reparam", "eps");
  check_buf(z16, torch::kBFloat16, B * Z, mulv, "reparam", "z16");
  check_buf(z32, torch::kFloat32, B * Z, mulv, "reparam", "z32");
  check_blob(state, sizeof(TrainState), mulv, "reparam", "state");
  check_blob(hparams, sizeof(HParams), mulv, "reparam", "hparams");
  check_buf(kld_part, torch::kFloat32, cdiv64(B * Z, 256), mulv, "reparam", "kld_part");  // one partial per block
  rc(mdt_reparam(mulv.data_ptr<float>(), eps.data_ptr<float>(), z16.data_ptr(), (float*)opt_ptr(z32), (int)B, (int)Z,
                 state.data_ptr(), hparams.data_ptr(), (unsigned)stream, kld_part.data_ptr<float>(), cur()),
     "reparam");
}

// Device address of the KL weight a backward kernel of the running step uses:
// TrainState.kl_t of `state` (written when the step was begun, an earlier
// launch; follows the trial's schedule) or, with no state, HParams.kl_beta.
const float* kl_weight_ptr(const at::Tensor& hparams, const c10::optional<at::Tensor>& state) {
  if (state.has_value() && state->defined()) {
    TORCH_CHECK(state->is_cuda() && state->is_contiguous() &&
                    state->numel() * state->element_size() >= (int64_t)sizeof(TrainState),
                "state: a TrialState device buffer");
    return reinterpret_cast<const float*>(static_cast<const char*>(state->data_ptr()) + offsetof(TrainState, kl_t));
  }
  TORCH_CHECK(hparams.defined() && hparams.is_cuda() && hparams.is_contiguous() &&
                  hparams.numel() * hparams.element_size() >= (int64_t)sizeof(HParams),
              "hparams: a TrialState device buffer");
  return reinterpret_cast<const float*>(static_cast<const char*>(hparams.data_ptr()) + offsetof(HParams, kl_beta));
}

// ... and of its free-bits floor: TrainState.fb_t (0 in an eval state) or, with
// no state, HParams.free_bits. Only address arithmetic: kl_weight_ptr, called
// for the same launch, validates both buffers before anything runs.
const float* free_bits_ptr(const at::Tensor& hparams, const c10::optional<at::Tensor>& state) {
  if (state.has_value() && state->defined())
    return reinterpret_cast<const float*>(static_cast<const char*>(state->data_ptr()) + offsetof(TrainState, fb_t));
  return reinterpret_cast<const float*>(static_cast<const char*>(hparams.data_ptr()) + offsetof(HParams, free_bits));
}

void reparam_bwd(const at::Tensor& dz, const at::Tensor& mulv, const at::Tensor& eps, at::Tensor dmulv,
                 const c10::optional<at::Tensor>& dmulv16, int64_t B, int64_t Z, const at::Tensor& hparams,
                 const c10::optional<at::Tensor>& state) {
  check_bz(B, Z, "reparam_bwd");
  check_buf(dz, torch::kFloat32, B * Z, dz, "reparam_bwd", "dz");
  check_buf(mulv, torch::kFloat32, B * 2 * Z, dz, "reparam_bwd", "mulv");
  check_buf(eps, torch::kFloat32, B * Z, dz, "reparam_bwd", "eps");
  check_buf(dmulv, torch::kFloat32, B * 2 * Z, dz, "reparam_bwd", "dmulv");
  check_buf(dmulv16, torch::kBFloat16, B * 2 * Z, dz, "reparam_bwd", "dmulv16");
  rc(mdt_reparam_bwd(dz.data_ptr<float>(), mulv.data_ptr<float>(), eps.data_ptr<float>(), dmulv.data_ptr<float>(),
                     const_cast<void*>(opt_ptr(dmulv16)), (int)B, (int)Z, kl_weight_ptr(hparams, state),
                     free_bits_ptr(hparams, state), cur()),
     "reparam_bwd");
}

void gather_rows(const at::Tensor& X, const at::Tensor& idx, const at::Tensor& state, int64_t B, int64_t M,
                 at::Tensor xb) {
  TORCH_CHECK(X.scalar_type() == torch::kFloat32 && idx.scalar_type() == torch::kInt32, "gather_rows dtypes");
  // Not checkable here: the rows idx[cursor * B + i] depend on device state (the
  // cursor) and on the index values; the trainer guarantees them (see f28 below)
  TORCH_CHECK(X.dim() == 2 && X.size(0) >= 1 && X.size(1) >= 4 && X.size(1) % 4 == 0 && X.size(1) < (int64_t(1) << 30),
              "gather_rows: X must be [rows][P] with P a positive multiple of 4 (16-B row pieces)");
  const int64_t P = X.size(1);
  TORCH_CHECK(B >= 1 && M >= 1 && M <= B && B < (int64_t(1) << 30), "gather_rows: need 1 <= M <= B, got M = ", M,
              ", B = ", B);
  check_buf(X, torch::kFloat32, P, X, "gather_rows", "X");
  check_buf(idx, torch::kInt32, B, X, "gather_rows", "idx");  // at least the batch at cursor 0
  check_blob(state, sizeof(TrainState), X, "gather_rows", "state");
  check_buf(xb, torch::kFloat32, M * P, X, "gather_rows", "xb");
  rc(mdt_gather_rows(X.data_ptr<float>(), idx.data_ptr<int32_t>(), state.data_ptr(), (int)B, (int)M,
                     (int)X.size(1), xb.data_ptr<float>(), cur()),
     "gather_rows");
}

void bce_logits(const at::Tensor& logits, const at::Tensor& X, const c10::optional<at::Tensor>& rows, int64_t B,
                int64_t P, const c10::optional<at::Tensor>& dlog16, const c10::optional<at::Tensor>& recon,
                at::Tensor part, const c10::optional<at::Tensor>& gpart) {
  const int64_t lim = int64_t(1) << 30;
  TORCH_CHECK(B >= 1 && P >= 1 && B < lim && P < lim, "bce_logits: need B >= 1 and P >= 1, got B = ", B, ", P = ", P);
  const int64_t n = B * P, nblk = cdiv64(n, 256);
  TORCH_CHECK(nblk < 2 * lim, "bce_logits: B * P too large");
  check_buf(logits, torch::kFloat32, n, logits, "bce_logits", "logits");
  if (rows.has_value() && rows->defined()) {
    // target row i = X[rows[i]]: the index VALUES are the caller's to keep inside X
    check_buf(rows, torch::kInt32, B, logits, "bce_logits", "rows");
    check_buf(X, torch::kFloat32, P, logits, "bce_logits", "X");
    TORCH_CHECK(X.numel() % P == 0, "bce_logits: X must hold whole rows of P = ", P, " elements");
  } else {
    check_buf(X, torch::kFloat32, n, logits, "bce_logits", "X");
  }
  check_buf(dlog16, torch::kBFloat16, n, logits, "bce_logits", "dlog16");
  check_buf(recon, torch::kFloat32, n, logits, "bce_logits", "recon");
  check_buf(part, torch::kFloat32, nblk, logits, "bce_logits", "part");  // one partial per 256-element block
  check_buf(gpart, torch::kFloat32, nblk, logits, "bce_logits", "gpart");
  rc(mdt_bce_logits(logits.data_ptr<float>(), X.data_ptr<float>(), (const int*)opt_ptr(rows), (int)B, (int)P,
                    const_cast<void*>(opt_ptr(dlog16)), (float*)opt_ptr(recon), part.data_ptr<float>(),
                    (float*)opt_ptr(gpart), cur()),
     "bce_logits");
}

void loss_finalize2(const at::Tensor& bce_part, int64_t nb, const at::Tensor& kld_part, int64_t nk, at::Tensor state,
                    const at::Tensor& hparams, bool advance_cursor, Job* job, bool advance_step) {
  TORCH_CHECK(nb >= 0 && nk >= 0 && nb < (int64_t(1) << 31) && nk < (int64_t(1) << 31),
              "loss_finalize2: partial counts out of range");
  TORCH_CHECK(bce_part.numel() >= nb && kld_part.numel() >= nk, "loss partials too small");
  check_buf(bce_part, torch::kFloat32, nb, bce_part, "loss_finalize2", "bce_part");
  check_buf(kld_part, torch::kFloat32, nk, bce_part, "loss_finalize2", "kld_part");
  check_blob(state, sizeof(TrainState), bce_part, "loss_finalize2", "state");
  check_blob(hparams, sizeof(HParams), bce_part, "loss_finalize2", "hparams");
  rc(mdt_conv_loss_finalize(blob(job), bce_part.data_ptr<float>(), (int)nb, kld_part.data_ptr<float>(), (int)nk,
                            state.data_ptr(), hparams.data_ptr(), (advance_cursor ? 1 : 0) | (advance_step ? 2 : 0),
                            cur()),
     job ? "job_loss" : "loss_finalize");
}

// Launch recorded jobs as ONE fused kernel when an instantiation exists for
// their kinds (returns true), else launch nothing and return false (the caller
// then issues the ops' own kernels). Follow-up combines run right after.
bool launch_jobs(const std::vector<Job*>& jobs) {
  TORCH_CHECK(jobs.size() >= 2 && jobs.size() <= 3, "launch_jobs takes 2 or 3 jobs");
  JobBlob v[3];
  for (size_t i = 0; i < jobs.size(); ++i) {
    TORCH_CHECK(jobs[i] != nullptr, "null job");
    v[i] = jobs[i]->main;
  }
  const int r = mdt_launch_jobs(v, (int)jobs.size(), cur());
  TORCH_CHECK(r >= 0 && r != 2, "mdt: launch_jobs failed (", r, ")");
  if (r != 0) return false;
  for (auto* j : jobs)
    if (j->has_post()) rc(mdt_launch_job1(&j->post, cur()), "job follow-up");
  return true;
}

// Pack recorded jobs (any supported kinds, up to kMaxMultiJobs = 8) into a job
// table for ONE jobs_multi_k launch: returns (uint8 CPU tensor image, grid). The caller keeps
// the table in device memory for the lifetime of the plan (graph replays).
std::tuple<at::Tensor, int64_t> pack_jobs_multi(const std::vector<Job*>& jobs,
                                                const c10::optional<at::Tensor>& stamps) {
  TORCH_CHECK(!jobs.empty() && jobs.size() <= (size_t)mdt::kMaxMultiJobs, "pack_jobs_multi takes 1..",
              mdt::kMaxMultiJobs, " jobs");
  std::vector<JobBlob> v;
  for (auto* j : jobs) {
    TORCH_CHECK(j != nullptr && !j->has_post(), "pack_jobs_multi: null job or job with a follow-up pass");
    TORCH_CHECK(j->main.kind > 0, "pack_jobs_multi: job has no fused form (kind 0)");
    v.push_back(j->main);
  }
  auto img = torch::zeros({(int64_t)mdt_jobs_multi_bytes()}, torch::kUInt8);
  const int grid = mdt_pack_jobs_multi(v.data(), (int)v.size(), img.data_ptr());
  TORCH_CHECK(grid > 0, "pack_jobs_multi: unsupported job kind or bad job (", grid, ")");
  if (stamps.has_value() && stamps->defined()) {  // profiling: [grid][2] int64 per-workgroup start / end stamps
    TORCH_CHECK(stamps->is_cuda() && stamps->scalar_type() == torch::kInt64 && stamps->numel() >= 2 * grid,
                "pack_jobs_multi: stamps must be an int64 CUDA tensor of >= 2 * grid elements");
    mdt_pack_jobs_multi_stamps(img.data_ptr(), stamps->data_ptr());
  }
  return {img, (int64_t)grid};
}

void launch_jobs_multi(const at::Tensor& dev_pack, int64_t grid) {
  TORCH_CHECK(dev_pack.is_cuda() && dev_pack.scalar_type() == torch::kUInt8 &&
                  dev_pack.numel() >= mdt_jobs_multi_bytes(), "launch_jobs_multi: device job table");
  const int r = mdt_launch_jobs_multi(dev_pack.data_ptr(), (int)grid, cur());
  TORCH_CHECK(r == 0, "mdt: launch_jobs_multi failed (", r, ")");
}

// Fused 28x28 step launches (conv28_fused.hip). A launch takes its tensors by
// slot name (csrc/kernels/conv28_slots.h; None or absent -> nullptr where
// optional); every tensor is checked for device, contiguity, dtype and minimum
// size BEFORE the launch, so a wrong buffer is a Python error rather than an
// out-of-bounds access. Not checkable here: the gathered rows
// X[idx[cursor * B + n]] depend on device state (the cursor) and on the index
// VALUES; the trainer guarantees them (bind_train_data pads idx to whole
// batches of in-range rows, set_cursor keeps cursor < nbatches), and the
// checks below pin the shapes they assume.
//
// f28_table resolves the names once: a trainer makes its tables when it plans a
// batch size and launches with them; a launch given a dict makes its table on
// the spot (as the eval pass does, whose data tensors change with the set).
using F28Tensors = std::unordered_map<std::string, c10::optional<at::Tensor>>;

// One validated table of a launch over M samples of batches of B: the device
// addresses in slot order, and the tensors they point into, kept alive.
struct F28Table {
  std::string kind;  // "forward", "backward" or "pair"
  int64_t B, M;      // B: the forward's (idx holds whole batches of B); M elsewhere
  bool train;        // forward: validated for a launch that stores the activations
  int dev;
  std::array<long long, f28::kNumFwdSlots> p;
  F28Tensors keep;
};
static_assert(f28::kNumFwdSlots >= f28::kNumBwdSlots && f28::kNumFwdSlots >= f28::kNumPairSlots, "F28Table::p");
using F28Arg = std::variant<std::shared_ptr<F28Table>, F28Tensors>;

namespace {
const at::Tensor* f28_find(const F28Tensors& t, const char* name) {
  const auto it = t.find(name);
  return it != t.end() && it->second.has_value() && it->second->defined() ? &*it->second : nullptr;
}

// r.p of `slots` from the tensors r.keep holds under their names, on the device of the first slot's.
template <size_t N>
void f28_resolve(F28Table& r, const f28::Slot (&slots)[N]) {
  const F28Tensors& t = r.keep;
  const at::Tensor* first = f28_find(t, slots[0].name);
  TORCH_CHECK(first, "f28: tensor ", slots[0].name, " is required");
  r.dev = (int)first->device().index();
  size_t known = 0;
  for (size_t i = 0; i < N; ++i) {
    const f28::Slot& s = slots[i];
    known += t.count(s.name);
    const at::Tensor* x = f28_find(t, s.name);
    if (!x) {
      TORCH_CHECK(s.need == f28::kOptional || (s.need == f28::kTrainOnly && !r.train), "f28: tensor ", s.name,
                  " is required");
      continue;
    }
    TORCH_CHECK(x->is_cuda() && x->device().index() == r.dev && x->is_contiguous(), "f28: ", s.name,
                " must be a contiguous tensor on cuda:", r.dev);
    const auto st = x->scalar_type();
    const bool ok = (s.dtype == 'f' && st == torch::kFloat32) || (s.dtype == 'b' && st == torch::kBFloat16) ||
                    (s.dtype == 'i' && st == torch::kInt32) || (s.dtype == 'u' && st == torch::kUInt8) ||
                    (s.dtype == 'l' && st == torch::kInt64);
    TORCH_CHECK(ok, "f28: ", s.name, " has dtype ", st);
    int64_t unit = 1;
    switch (s.unit) {
      case f28::kFixed: break;
      case f28::kPerSample: unit = r.M; break;
      case f28::kPerBatchRow: unit = r.B; break;
      case f28::kTrainState: unit = (int64_t)sizeof(TrainState); break;
      case f28::kHParams: unit = (int64_t)sizeof(HParams); break;
      case f28::kPairGranules: unit = r.M * mdt_f28_pair_words(); break;
    }
    TORCH_CHECK(x->numel() >= s.count * unit, "f28: ", s.name, " has ", x->numel(), " elements, needs ",
                s.count * unit);
    r.p[i] = (long long)(intptr_t)x->data_ptr();
  }
  if (known != t.size())  // a key that is no slot of this table
    for (const auto& kv : t) {
      bool is_slot = false;
      for (const f28::Slot& s : slots) is_slot |= kv.first == s.name;
      TORCH_CHECK(is_slot, "f28: unknown tensor name ", kv.first);
    }
}
}  // namespace

std::shared_ptr<F28Table> f28_table(const std::string& kind, const F28Tensors& t, int64_t B, int64_t M, bool train) {
  TORCH_CHECK(M > 0 && M <= B, "f28: bad M ", M, " for B ", B);
  const bool fwd = kind == "forward";
  auto r = std::make_shared<F28Table>(F28Table{kind, fwd ? B : M, M, train || !fwd, 0, {}, t});
  if (fwd) {
    f28_resolve(*r, f28::kFwdSlots);
    // X is [rows][784] and idx whole batches of B (cursor * B + n indexes it)
    const int64_t nx = f28_find(t, "X")->numel(), ni = f28_find(t, "idx")->numel();
    TORCH_CHECK(nx % 784 == 0, "f28: X must be [rows][784], has ", nx, " elements");
    TORCH_CHECK(ni % B == 0, "f28: idx must hold whole batches of ", B, ", has ", ni);
  } else if (kind == "backward") {
    f28_resolve(*r, f28::kBwdSlots);
  } else {
    TORCH_CHECK(kind == "pair", "f28_table: kind is forward, backward or pair, got ", kind);
    f28_resolve(*r, f28::kPairSlots);
  }
  return r;
}

namespace {
// The launch's table of `kind`: the one given, if it was made for this launch, or one made from the dict given.
std::shared_ptr<F28Table> f28_get(const F28Arg& a, const char* kind, int64_t B, int64_t M, bool train, int dev = -1) {
  auto r = a.index() == 0 ? std::get<0>(a) : f28_table(kind, std::get<1>(a), B, M, train);
  const int64_t b = std::strcmp(kind, "forward") == 0 ? B : M;
  TORCH_CHECK(r && r->kind == kind && r->B == b && r->M == M && r->train == train, "f28: not a ", kind,
              " table made for this launch's B, M and train");
  TORCH_CHECK(dev < 0 || r->dev == dev, "f28: the ", kind, " table's tensors are on another device than the forward's");
  return r;
}
bool f28_empty(const F28Arg& a) { return a.index() == 1 && std::get<1>(a).empty(); }
}  // namespace

// The names of the four tables, in table order (the launch tables begin with the weights).
std::map<std::string, std::vector<std::string>> f28_slot_names() {
  const auto names = [](const auto& slots) {
    std::vector<std::string> v;
    for (const f28::Slot& s : slots) v.push_back(s.name);
    return v;
  };
  return {{"weights", names(f28::kWeightSlots)}, {"forward", names(f28::kFwdSlots)},
          {"backward", names(f28::kBwdSlots)}, {"pair", names(f28::kPairSlots)}};
}

// `pair` (eval only, train = false): the same three tensors as f28_step's;
// the forward then runs two workgroups per sample (mdt_f28_forward_pair).
void f28_forward(const F28Arg& t, int64_t B, int64_t M, int64_t stream, bool train, const F28Arg& pair) {
  TORCH_CHECK(M > 0 && M <= B, "f28_forward: bad M ", M, " for B ", B);
  TORCH_CHECK(f28_empty(pair) || !train, "f28_forward: the paired forward is eval-only");
  const auto f = f28_get(t, "forward", B, M, train);
  if (!f28_empty(pair)) {
    const auto pp = f28_get(pair, "pair", B, M, true, f->dev);
    rc(mdt_f28_forward_pair(f->p.data(), pp->p.data(), (int)B, (int)M, (unsigned)stream, cur()), "f28_forward(pair)");
    return;
  }
  rc(mdt_f28_forward(f->p.data(), (int)B, (int)M, (unsigned)stream, train ? 1 : 0, cur()), "f28_forward");
}

// `state` (optional): the training state whose step is advanced AFTER this
// launch (the fused step's loss job): the backward then uses the KL weight of
// step + 1 recorded there; without it, HParams.kl_beta.
void f28_backward(const F28Arg& t, int64_t M, const c10::optional<at::Tensor>& state) {
  TORCH_CHECK(M > 0, "f28_backward: bad M");
  const auto b = f28_get(t, "backward", M, M, true);
  const void* st = nullptr;
  if (state.has_value() && state->defined()) {
    TORCH_CHECK(state->is_cuda() && state->numel() * state->element_size() >= (int64_t)sizeof(TrainState),
                "f28_backward: state must be a TrialState device buffer");
    st = state->data_ptr();
  }
  rc(mdt_f28_backward(b->p.data(), (int)M, st, cur()), "f28_backward");
}

// Forward + backward of one training step in ONE launch (f28_step_k). With
// `pair` (exchange granules `xg` int64 [B][2][f28_pair_words()], pairing words
// `pairw` int32 [B], error word `err` int32 [1], all zero-initialised) the
// launch runs two workgroups per sample. `adamc` (optional, f32 [16]): receives
// the Adam constants of the step that the following launch advances to, for
// weight-gradient jobs that apply Adam in it (wgrad's `adam`).
void f28_step(const F28Arg& tf, const F28Arg& tb, int64_t B, int64_t M, int64_t stream, const F28Arg& pair,
              int64_t pair_delay_us, const c10::optional<at::Tensor>& adamc) {
  TORCH_CHECK(M > 0 && M <= B, "f28_step: bad M ", M, " for B ", B);
  const auto f = f28_get(tf, "forward", B, M, true);
  const auto b = f28_get(tb, "backward", B, M, true, f->dev);
  const auto pp = f28_empty(pair) ? nullptr : f28_get(pair, "pair", B, M, true, f->dev);
  float* ac = nullptr;
  if (adamc.has_value() && adamc->defined()) ac = adamc_ptr(*adamc, f->dev, "f28_step");
  rc(mdt_f28_step(f->p.data(), b->p.data(), pp ? pp->p.data() : nullptr, (int)B, (int)M, (unsigned)stream,
                  pp ? 1 : 0, (int)pair_delay_us, ac, cur()),
     "f28_step");
}

void step_begin(at::Tensor state, const at::Tensor& hparams) {
  check_blob(state, sizeof(TrainState), state, "step_begin", "state");
  check_blob(hparams, sizeof(HParams), state, "step_begin", "hparams");
  rc(mdt_step_begin(state.data_ptr(), hparams.data_ptr(), cur()), "step_begin");
}

// segment = (off, numel, slab_ptr, nsplit, co, k, s, ci, toff); slab_ptr is a
// device address (tensor.data_ptr()) or 0. The caller keeps the slabs alive.
at::Tensor make_grad_segs(const std::vector<std::vector<int64_t>>& segs, int64_t device_index) {
  std::vector<GradSeg> v;
  for (auto& s : segs) {
    TORCH_CHECK(s.size() == 9, "segment = (off, numel, slab_ptr, nsplit, co, k, s, ci, toff)");
    GradSeg g;
    g.off = s[0]; g.numel = s[1];
    g.slab = reinterpret_cast<const float*>((uintptr_t)s[2]);
    g.nsplit = (int)s[3]; g.co = (int)s[4]; g.k = (int)s[5]; g.s = (int)s[6]; g.ci = (int)s[7]; g.toff = s[8];
    TORCH_CHECK(g.toff < 0 || (g.s > 0 && g.k % g.s == 0), "transposed copy needs k % s == 0");
    v.push_back(g);
  }
  auto cpu = torch::empty({(int64_t)(v.size() * sizeof(GradSeg))}, torch::kUInt8);
  std::memcpy(cpu.data_ptr(), v.data(), v.size() * sizeof(GradSeg));
  return cpu.to(torch::Device(torch::kCUDA, device_index));
}

at::Tensor make_grad_units(const std::vector<std::vector<int64_t>>& units, int64_t device_index) {
  std::vector<GradUnit> v;
  for (auto& u : units) {
    // count <= 256: one element (column) per thread group; 256 < count <= 1024: 4 elements per thread
    TORCH_CHECK(u.size() == 3 && u[2] >= 1 && u[2] <= 1024, "unit = (seg, start, count<=1024)");
    v.push_back(GradUnit{(int)u[0], (int)u[1], (int)u[2]});
  }
  auto cpu = torch::empty({(int64_t)std::max<size_t>(1, v.size() * sizeof(GradUnit))}, torch::kUInt8);
  if (!v.empty()) std::memcpy(cpu.data_ptr(), v.data(), v.size() * sizeof(GradUnit));
  return cpu.to(torch::Device(torch::kCUDA, device_index));
}

at::Tensor make_tr_units(const std::vector<std::vector<int64_t>>& units, int64_t device_index) {
  std::vector<TrUnit> v;
  for (auto& u : units) {
    TORCH_CHECK(u.size() == 4, "unit = (seg, tap, co0, ci0)");
    v.push_back(TrUnit{(int)u[0], (int)u[1], (int)u[2], (int)u[3]});
  }
  auto cpu = torch::empty({(int64_t)std::max<size_t>(1, v.size() * sizeof(TrUnit))}, torch::kUInt8);
  if (!v.empty()) std::memcpy(cpu.data_ptr(), v.data(), v.size() * sizeof(TrUnit));
  return cpu.to(torch::Device(torch::kCUDA, device_index));
}

void adam_cast(at::Tensor P, const at::Tensor& G, at::Tensor M, at::Tensor V, at::Tensor w16, const at::Tensor& segs,
               int64_t nseg, const at::Tensor& state, const at::Tensor& hparams, bool do_adam) {
  TORCH_CHECK(G.numel() == P.numel() && M.numel() == P.numel() && V.numel() == P.numel() && w16.numel() == P.numel(),
              "adam_cast: P, G, m, v and w16 must be arenas of one size");
  const int64_t total = P.numel();
  TORCH_CHECK(total >= 4 && total % 4 == 0, "adam_cast: the arena length must be a positive multiple of 4, got ",
              total);
  check_buf(P, torch::kFloat32, total, P, "adam_cast", "P");
  check_buf(G, torch::kFloat32, total, P, "adam_cast", "G");
  check_buf(M, torch::kFloat32, total, P, "adam_cast", "m");
  check_buf(V, torch::kFloat32, total, P, "adam_cast", "v");
  check_buf(w16, torch::kBFloat16, total, P, "adam_cast", "w16");
  check_blob(state, sizeof(TrainState), P, "adam_cast", "state");
  check_blob(hparams, sizeof(HParams), P, "adam_cast", "hparams");
  rc(mdt_adam_cast(P.data_ptr<float>(), G.data_ptr<float>(), M.data_ptr<float>(), V.data_ptr<float>(),
                   w16.data_ptr(), segs.data_ptr(), (int)nseg, P.numel(), state.data_ptr(), hparams.data_ptr(),
                   do_adam ? 1 : 0, cur()),
     "adam_cast");
}

void grad_finalize(at::Tensor P, at::Tensor G, at::Tensor M, at::Tensor V, at::Tensor w16, const at::Tensor& segs,
                   const at::Tensor& units, int64_t nunits, const at::Tensor& state, const at::Tensor& hparams,
                   bool do_adam, Job* job, const std::vector<at::Tensor>& gather, int64_t gather_B) {
  TORCH_CHECK(units.numel() >= nunits * (int64_t)sizeof(GradUnit), "grad_finalize: unit table too small");
  TORCH_CHECK(!job || gather.empty(), "grad_finalize: a finalize job takes no gather");
  // optional next-batch gather (the fused 28x28 step): [X, idx, xn, xtag] and the batch size
  const float* gX = nullptr;
  const int* gidx = nullptr;
  float* xn = nullptr;
  unsigned* xtag = nullptr;
  if (!gather.empty()) {
    TORCH_CHECK(gather.size() == 4 && gather_B > 0, "grad_finalize: gather = [X, idx, xn, xtag] with gather_B > 0");
    const int dev = P.get_device();
    const char* nm[4] = {"X", "idx", "xn", "xtag"};
    for (int i = 0; i < 4; ++i)
      TORCH_CHECK(gather[i].is_cuda() && gather[i].get_device() == dev && gather[i].is_contiguous(),
                  "grad_finalize: gather ", nm[i], " must be a contiguous tensor on the arena's device");
    TORCH_CHECK(gather[0].scalar_type() == torch::kFloat32 && gather[0].numel() % 784 == 0, "grad_finalize: X [rows][784] f32");
    TORCH_CHECK(gather[1].scalar_type() == torch::kInt32 && gather[1].numel() % gather_B == 0,
                "grad_finalize: idx int32 in whole batches");
    TORCH_CHECK(gather[2].scalar_type() == torch::kFloat32 && gather[2].numel() >= gather_B * 784, "grad_finalize: xn");
    TORCH_CHECK(gather[3].scalar_type() == torch::kInt32 && gather[3].numel() >= gather_B, "grad_finalize: xtag");
    gX = gather[0].data_ptr<float>();
    gidx = gather[1].data_ptr<int>();
    xn = gather[2].data_ptr<float>();
    xtag = reinterpret_cast<unsigned*>(gather[3].data_ptr<int>());
  }
  rc(mdt_grad_finalize(blob(job), P.data_ptr<float>(), G.data_ptr<float>(), M.data_ptr<float>(), V.data_ptr<float>(),
                       w16.data_ptr(), segs.data_ptr(), units.data_ptr(), (int)nunits, state.data_ptr(),
                       hparams.data_ptr(), do_adam ? 1 : 0, gX, gidx, xn, xtag, (int)gather_B, cur()),
     job ? "job_finalize" : "grad_finalize");
}

// Record a fused all-reduce job (csrc/kernels/comm_jobs.h) over `nunits`
// finalize units: mode 1 push, 2 reduce(+Adam), 3 both. `ctx` is the device
// address from XgmiP2PReducer.comm_ctx(). Jobs only: they run inside a
// jobs_multi_k launch next to other work of the step.
void comm_job(at::Tensor P, at::Tensor G, at::Tensor M, at::Tensor V, at::Tensor w16, const at::Tensor& segs,
              const at::Tensor& units, int64_t nunits, const at::Tensor& state, const at::Tensor& hparams,
              bool do_adam, int64_t ctx, int64_t mode, Job* job) {
  TORCH_CHECK(job != nullptr, "comm_job: records into a Job (no stand-alone launch)");
  TORCH_CHECK(units.numel() >= nunits * (int64_t)sizeof(GradUnit), "comm_job: unit table too small");
  TORCH_CHECK(P.numel() == G.numel() && M.numel() == G.numel() && V.numel() == G.numel() && w16.numel() == G.numel(),
              "comm_job: arenas differ in size");
  rc(mdt_job_comm(&job->main, P.data_ptr<float>(), G.data_ptr<float>(), M.data_ptr<float>(), V.data_ptr<float>(),
                  w16.data_ptr(), segs.data_ptr(), units.data_ptr(), (int)nunits, state.data_ptr(),
                  hparams.data_ptr(), do_adam ? 1 : 0, reinterpret_cast<const void*>((intptr_t)ctx), (int)mode),
     "job_comm");
}

void wtrans(const at::Tensor& w16, at::Tensor w16t, const at::Tensor& segs, const at::Tensor& units, int64_t nunits,
            Job* job) {
  check_bf16(w16, "w16");
  check_bf16(w16t, "w16t");
  TORCH_CHECK(units.numel() >= nunits * (int64_t)sizeof(TrUnit), "wtrans: unit table too small");
  rc(mdt_wtrans(blob(job), w16.data_ptr(), w16t.data_ptr(), segs.data_ptr(), units.data_ptr(), (int)nunits, cur()),
     job ? "job_wtrans" : "wtrans");
}

// Split-K combine of the encoder head fused with the reparameterisation, and
// of the decoder Linear's backward-data fused with its backward.
void combine_reparam(const at::Tensor& ws, int64_t ks, const c10::optional<at::Tensor>& bias, at::Tensor mulv,
                     at::Tensor eps, at::Tensor z16, const c10::optional<at::Tensor>& z32, int64_t B, int64_t Z,
                     const at::Tensor& state, const at::Tensor& hparams, int64_t stream, at::Tensor kld_part) {
  check_f32(ws, "ws");
  check_bz(B, Z, "combine_reparam");
  TORCH_CHECK(ks >= 1 && ks < (int64_t(1) << 20), "combine_reparam: need 1 <= ks < 2^20 k-slices, got ", ks);
  // the row form reads the slab as float4s
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ws.data_ptr()) % 16 == 0, "combine_reparam: ws must be 16-B aligned");
  check_buf(ws, torch::kFloat32, ks * B * 2 * Z, ws, "combine_reparam", "ws");
  check_buf(bias, torch::kFloat32, 2 * Z, ws, "combine_reparam", "bias");
  check_buf(mulv, torch::kFloat32, B * 2 * Z, ws, "combine_reparam", "mulv");
  check_buf(eps, torch::kFloat32, B * Z, ws, "combine_reparam", "eps");
  check_buf(z16, torch::kBFloat16, B * Z, ws, "combine_reparam", "z16");
  check_buf(z32, torch::kFloat32, B * Z, ws, "combine_reparam", "z32");
  check_blob(state, sizeof(TrainState), ws, "combine_reparam", "state");
  check_blob(hparams, sizeof(HParams), ws, "combine_reparam", "hparams");
  check_buf(kld_part, torch::kFloat32, mdt_combine_reparam_blocks((int)ks, (int)B, (int)Z), ws, "combine_reparam",
            "kld_part");  // one partial per block
  rc(mdt_combine_reparam(ws.data_ptr<float>(), (int)ks, (const float*)opt_ptr(bias), mulv.data_ptr<float>(),
                         eps.data_ptr<float>(), z16.data_ptr(), (float*)opt_ptr(z32), (int)B, (int)Z, state.data_ptr(),
                         hparams.data_ptr(), (unsigned)stream, kld_part.data_ptr<float>(), cur()),
     "combine_reparam");
}

void combine_reparam_bwd(const at::Tensor& ws, int64_t ks, const at::Tensor& mulv, const at::Tensor& eps,
                         at::Tensor dmulv, const c10::optional<at::Tensor>& dmulv16,
                         const c10::optional<at::Tensor>& dz, int64_t B, int64_t Z, const at::Tensor& hparams,
                         const c10::optional<at::Tensor>& state) {
  check_f32(ws, "ws");
  check_bz(B, Z, "combine_reparam_bwd");
  TORCH_CHECK(ks >= 1 && ks < (int64_t(1) << 20), "combine_reparam_bwd: need 1 <= ks < 2^20 k-slices, got ", ks);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(ws.data_ptr()) % 16 == 0, "combine_reparam_bwd: ws must be 16-B aligned");
  check_buf(ws, torch::kFloat32, ks * B * Z, ws, "combine_reparam_bwd", "ws");
  check_buf(mulv, torch::kFloat32, B * 2 * Z, ws, "combine_reparam_bwd", "mulv");
  check_buf(eps, torch::kFloat32, B * Z, ws, "combine_reparam_bwd", "eps");
  check_buf(dmulv, torch::kFloat32, B * 2 * Z, ws, "combine_reparam_bwd", "dmulv");
  check_buf(dmulv16, torch::kBFloat16, B * 2 * Z, ws, "combine_reparam_bwd", "dmulv16");
  check_buf(dz, torch::kFloat32, B * Z, ws, "combine_reparam_bwd", "dz");
  rc(mdt_combine_reparam_bwd(ws.data_ptr<float>(), (int)ks, mulv.data_ptr<float>(), eps.data_ptr<float>(),
                             dmulv.data_ptr<float>(), const_cast<void*>(opt_ptr(dmulv16)), (float*)opt_ptr(dz), (int)B,
                             (int)Z, kl_weight_ptr(hparams, state), free_bits_ptr(hparams, state), cur()),
     "combine_reparam_bwd");
}

void bind_conv(pybind11::module& m) {
  namespace py = pybind11;
  // the plan numbers that are no tile index (ops/conv_plans.py)
  m.attr("FWD_DIRECT_BASE") = kFwdDirectBase;
  m.attr("WG_DIRECT_BASE") = kWgDirectBase;
  m.attr("WG_THIN_MFMA") = kWgThinMfma;
  m.def("igemm_plan", &igemm_plan, py::arg("mode"), py::arg("desc"), py::arg("allow_split"), py::arg("fwd") = false);
  m.def("dconv_stamps", [](const c10::optional<at::Tensor>& t) {
    // profiling: per-workgroup s_memrealtime stamps of the direct conv kernels ([grid][8] int64), None = off
    if (t.has_value() && t->defined()) {
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kInt64, "dconv_stamps: int64 CUDA tensor");
      mdt_dconv_stamps(reinterpret_cast<unsigned long long*>(t->data_ptr()));
    } else {
      mdt_dconv_stamps(nullptr);
    }
  });
  m.def("wgrad_plan", &wgrad_plan);
  py::class_<Job>(m, "Job")
      .def(py::init<>())
      .def_property_readonly("kind", &Job::kind)
      .def_property_readonly("nblk", [](const Job& j) { return j.main.nblk; })
      .def_property_readonly("has_post", &Job::has_post);
  m.def("launch_jobs", &launch_jobs);
  m.def("pack_jobs_multi", &pack_jobs_multi, py::arg("jobs"), py::arg("stamps") = py::none());
  m.def("launch_jobs_multi", &launch_jobs_multi, py::arg("dev_pack"), py::arg("grid"));
  m.def("f28_forward", &f28_forward, py::arg("tensors"), py::arg("B"), py::arg("M"), py::arg("stream"),
        py::arg("train"), py::arg("pair") = F28Arg{F28Tensors{}});
  m.def("f28_backward", &f28_backward, py::arg("tensors"), py::arg("M"), py::arg("state") = py::none());
  m.def("f28_pair_words", &mdt_f28_pair_words);
  m.def("f28_slot_names", &f28_slot_names);
  py::class_<F28Table, std::shared_ptr<F28Table>>(m, "F28Table");
  m.def("f28_table", &f28_table, py::arg("kind"), py::arg("tensors"), py::arg("B"), py::arg("M"),
        py::arg("train") = true);
  m.def("f28_step", &f28_step, py::arg("fwd_tensors"), py::arg("bwd_tensors"), py::arg("B"), py::arg("M"),
        py::arg("stream"), py::arg("pair") = F28Arg{F28Tensors{}},
        py::arg("pair_delay_us") = 0, py::arg("adamc") = py::none());
  m.def("igemm", &igemm, py::arg("mode"), py::arg("A"), py::arg("B16"), py::arg("desc"), py::arg("bias"),
        py::arg("relu"), py::arg("y16"), py::arg("y32"), py::arg("omask") = py::none(),
        py::arg("colsum") = py::none(), py::arg("ws") = py::none(), py::arg("job") = py::none(),
        py::arg("combine") = true, py::arg("a_slab") = py::none(), py::arg("a_ks") = 0,
        py::arg("a_bias") = py::none(), py::arg("a_relu") = false, py::arg("a_out16") = py::none(),
        py::arg("fwd") = false);
  m.def("wgrad", &wgrad, py::arg("G16"), py::arg("X"), py::arg("desc"), py::arg("out"), py::arg("job") = py::none(),
        py::arg("adam") = std::vector<at::Tensor>{}, py::arg("adam_off") = 0, py::arg("adamc") = py::none());
  m.def("colsum", &colsum, py::arg("G16"), py::arg("M"), py::arg("N"), py::arg("rows_per"), py::arg("slab"),
        py::arg("job") = py::none());
  m.def("thin_conv", &thin_conv, py::arg("X"), py::arg("Wf"), py::arg("desc"), py::arg("bias"), py::arg("relu"),
        py::arg("y16"), py::arg("omask") = py::none(), py::arg("colsum") = py::none(), py::arg("job") = py::none(),
        py::arg("idx") = py::none(), py::arg("state") = py::none(), py::arg("hparams") = py::none(),
        py::arg("B") = 0, py::arg("xb") = py::none());
  m.def("thin_blocks", &thin_blocks);
  m.def("thin_tconv", &thin_tconv, py::arg("G16"), py::arg("Wf"), py::arg("desc"), py::arg("bias"),
        py::arg("y32") = py::none(), py::arg("X") = py::none(), py::arg("dlog16") = py::none(),
        py::arg("recon") = py::none(), py::arg("part") = py::none(), py::arg("gpart") = py::none());
  m.def("gather_rows", &gather_rows);
  m.def("reparam", &reparam);
  m.def("reparam_bwd", &reparam_bwd, py::arg("dz"), py::arg("mulv"), py::arg("eps"), py::arg("dmulv"),
        py::arg("dmulv16"), py::arg("B"), py::arg("Z"), py::arg("hparams"), py::arg("state") = py::none());
  m.def("bce_logits", &bce_logits, py::arg("logits"), py::arg("X"), py::arg("rows"), py::arg("B"), py::arg("P"),
        py::arg("dlog16"), py::arg("recon"), py::arg("part"), py::arg("gpart") = py::none());
  m.def("loss_finalize2", &loss_finalize2, py::arg("bce_part"), py::arg("nb"), py::arg("kld_part"), py::arg("nk"),
        py::arg("state"), py::arg("hparams"), py::arg("advance_cursor"), py::arg("job") = py::none(),
        py::arg("advance_step") = false);
  m.def("step_begin", &step_begin);
  m.def("make_grad_segs", &make_grad_segs);
  m.def("make_grad_units", &make_grad_units);
  m.def("make_tr_units", &make_tr_units);
  m.def("adam_cast", &adam_cast);
  m.def("graph_upload", [](int64_t exec) {
    // Upload an instantiated step graph to the device ahead of its first
    // replay, so that launch's one-time cost stays out of a timed region.
    TORCH_CHECK(exec != 0, "graph_upload: null graph exec");
    rc((int)hipGraphUpload(reinterpret_cast<hipGraphExec_t>((intptr_t)exec), cur()), "hipGraphUpload");
  });
  m.def("grad_finalize", &grad_finalize, py::arg("P"), py::arg("G"), py::arg("M"), py::arg("V"), py::arg("w16"),
        py::arg("segs"), py::arg("units"), py::arg("nunits"), py::arg("state"), py::arg("hparams"),
        py::arg("do_adam"), py::arg("job") = py::none(), py::arg("gather") = std::vector<at::Tensor>{},
        py::arg("gather_B") = 0);
  m.def("comm_job", &comm_job, py::arg("P"), py::arg("G"), py::arg("M"), py::arg("V"), py::arg("w16"),
        py::arg("segs"), py::arg("units"), py::arg("nunits"), py::arg("state"), py::arg("hparams"),
        py::arg("do_adam"), py::arg("ctx"), py::arg("mode"), py::arg("job"));
  m.def("wtrans", &wtrans, py::arg("w16"), py::arg("w16t"), py::arg("segs"), py::arg("units"), py::arg("nunits"),
        py::arg("job") = py::none());
  m.def("combine_reparam", &combine_reparam);
  m.def("combine_reparam_bwd", &combine_reparam_bwd, py::arg("ws"), py::arg("ks"), py::arg("mulv"), py::arg("eps"),
        py::arg("dmulv"), py::arg("dmulv16"), py::arg("dz"), py::arg("B"), py::arg("Z"), py::arg("hparams"),
        py::arg("state") = py::none());
  m.def("combine_reparam_blocks", &mdt_combine_reparam_blocks);
}

}  // namespace mdt
