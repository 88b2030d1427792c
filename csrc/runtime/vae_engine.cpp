#include "vae_engine.h"

#include <c10/hip/HIPStream.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <cmath>
#include <cstring>
#include <stdexcept>

#include "../kernels/vae_iw.h"
#include "../kernels/vae_latent.h"
#include "../kernels/vae_mlp.h"

namespace mdt {

static inline int64_t align64(int64_t v) { return (v + 63) / 64 * 64; }

static void check_rc(int rc, const char* what) {
  if (rc != 0) {
    throw std::runtime_error(std::string("mdt: ") + what + " failed with code " +
                             std::to_string(rc));
  }
}

// Every shape-only condition of mdt_vae_check at M = B (docs/KERNELS.md, "MLP-VAE
// shape domain"): an unsupported shape fails here, by name, not as a return
// code of the first step. The kernel-side checks stay (they also see M).
static void check_shapes(int64_t batch, int64_t D, int64_t H, int64_t Z) {
  TORCH_CHECK(batch > 0 && batch <= kMaxBatch, "MlpVaeEngine: batch size ", batch, " must be in [1, ", kMaxBatch,
              "]");
  TORCH_CHECK(Z >= 4 && Z <= 32 && Z % 4 == 0, "MlpVaeEngine: latent size Z = ", Z,
              " must be a multiple of 4 in [4, 32]");
  TORCH_CHECK(D >= 4 && D % 4 == 0, "MlpVaeEngine: input size D = ", D, " must be a positive multiple of 4");
  TORCH_CHECK(H >= 4 && H % 4 == 0, "MlpVaeEngine: hidden size H = ", H, " must be a positive multiple of 4");
  TORCH_CHECK(H <= 16 * 32, "MlpVaeEngine: hidden size H = ", H, " exceeds the limit of 512 (32 slab slices of 16)");
  const int64_t row_tiles = (batch + 15) / 16;
  const int64_t kld_slots = row_tiles * 8, kld_cap = kBcePartial - kKldPartial;
  TORCH_CHECK(kld_slots <= kld_cap, "MlpVaeEngine: batch size ", batch, " needs ", kld_slots,
              " KLD partial slots (ceil(B/16)*8), limit ", kld_cap);
  const int64_t bce_slots = (row_tiles * ((D + 15) / 16) + 1) / 2 * 8, bce_cap = kPartials - kBcePartial;
  TORCH_CHECK(bce_slots <= bce_cap, "MlpVaeEngine: batch size ", batch, " with D = ", D, " needs ", bce_slots,
              " BCE partial slots (ceil(ceil(B/16)*ceil(D/16)/2)*8), limit ", bce_cap);
}

// The checks run before the first allocation (the `state` member's).
MlpVaeEngine::MlpVaeEngine(int64_t batch, int64_t D, int64_t H, int64_t Z, int64_t device_index)
    : state((check_shapes(batch, D, H, Z), device_index)), B_(batch), D_(D), H_(H), Z_(Z) {
  int64_t off = 0;
  auto add = [&](const std::string& n, std::vector<int64_t> shape, int64_t numel) {
    layout_.push_back({n, off, shape});
    off = align64(off + numel);
  };
  // head: everything whose gradient becomes final at the END of backward
  add("fc1.weight", {H, D}, H * D);
  add("fc1.bias", {H}, H);
  const int64_t w2 = off;
  off = align64(off + 2 * Z * H);
  const int64_t b2 = off;
  off = align64(off + 2 * Z);
  layout_.push_back({"fc21.weight", w2, {Z, H}});
  layout_.push_back({"fc22.weight", w2 + Z * H, {Z, H}});
  layout_.push_back({"fc21.bias", b2, {Z}});
  layout_.push_back({"fc22.bias", b2 + Z, {Z}});
  add("fc3.weight", {H, Z}, H * Z);
  add("fc3.bias", {H}, H);
  split_ = off;  // tail bucket: fc4 (ready first in backward)
  add("fc4.weight", {D, H}, D * H);
  add("fc4.bias", {D}, D);
  total_ = off;

  auto fopt = torch::TensorOptions().dtype(torch::kFloat32).device(torch::kCUDA, device_index);
  params = torch::zeros({total_}, fopt);
  grads = torch::zeros({total_}, fopt);
  exp_avg = torch::zeros({total_}, fopt);
  exp_avg_sq = torch::zeros({total_}, fopt);

  int64_t a = 0;
  auto act_add = [&](const char* n, int64_t per_row) {
    act_off_.push_back({n, a});
    a = align64(a + B_ * per_row);
  };
  act_add("h1", H); act_add("mulv", 2 * Z); act_add("eps", Z); act_add("z", Z);
  act_add("h3", H); act_add("dlog", D); act_add("dh3", H); act_add("dmulv", 2 * Z);
  act_add("dh1", H); act_add("recon", D); act_add("xb", D);
  const int64_t th = (H + 15) / 16, sw = (2 * Z + 15) / 16 * 16, swz = (Z + 15) / 16 * 16;
  const int64_t Bpad = (B_ + 15) / 16 * 16;
  act_off_.push_back({"slab_mv", a});
  a = align64(a + Bpad * th * sw);
  act_off_.push_back({"slab_dz", a});
  a = align64(a + Bpad * th * swz);
  acts = torch::zeros({a}, fopt);
  partials = torch::zeros({kPartials}, fopt);
  iw_state = iw_state_new(device_index);
}

std::vector<std::tuple<std::string, int64_t, std::vector<int64_t>>> MlpVaeEngine::layout() const {
  std::vector<std::tuple<std::string, int64_t, std::vector<int64_t>>> out;
  for (auto& e : layout_) out.emplace_back(e.name, e.offset, e.shape);
  return out;
}

static int64_t off_of(const std::vector<LayoutEntry>& l, const char* n) {
  for (auto& e : l)
    if (e.name == n) return e.offset;
  throw std::runtime_error(std::string("mdt: no layout entry ") + n);
}

at::Tensor MlpVaeEngine::act(const std::string& name, int64_t M) {
  for (auto& p : act_off_) {
    if (p.first == name) {
      int64_t per = 0;
      if (name == "h1" || name == "h3" || name == "dh3" || name == "dh1") per = H_;
      else if (name == "mulv" || name == "dmulv") per = 2 * Z_;
      else if (name == "eps" || name == "z") per = Z_;  // recon, xb, dlog: D
      else per = D_;
      return acts.narrow(0, p.second, M * per).view({M, per});
    }
  }
  throw std::runtime_error("mdt: unknown activation " + name);
}

void MlpVaeEngine::fill_args(void* out, const at::Tensor& X, const at::Tensor& idx, int64_t M,
                             bool train, bool eval, int64_t rng_stream, bool want_recon) {
  TORCH_CHECK(X.is_cuda() && X.scalar_type() == torch::kFloat32 && X.is_contiguous() &&
                  X.dim() == 2 && X.size(1) == D_,
              "X must be a contiguous CUDA float32 [N, D] tensor");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt32 && idx.is_contiguous(),
              "idx must be a contiguous CUDA int32 tensor");
  TORCH_CHECK(M > 0 && M <= B_, "M must be in [1, B]");
  VaeArgs& a = *reinterpret_cast<VaeArgs*>(out);
  std::memset(&a, 0, sizeof(a));
  a.M = (int)M; a.B = (int)B_; a.D = (int)D_; a.H = (int)H_; a.Z = (int)Z_;
  a.rng_stream = (uint32_t)rng_stream;
  a.train = train ? 1 : 0;
  a.X = X.data_ptr<float>();
  a.idx = idx.data_ptr<int32_t>();
  float* P = params.data_ptr<float>();
  float* G = grads.data_ptr<float>();
  const int64_t oW1 = off_of(layout_, "fc1.weight"), ob1 = off_of(layout_, "fc1.bias");
  const int64_t oW2 = off_of(layout_, "fc21.weight"), ob2 = off_of(layout_, "fc21.bias");
  const int64_t oW3 = off_of(layout_, "fc3.weight"), ob3 = off_of(layout_, "fc3.bias");
  const int64_t oW4 = off_of(layout_, "fc4.weight"), ob4 = off_of(layout_, "fc4.bias");
  a.W1 = P + oW1; a.b1 = P + ob1; a.W2 = P + oW2; a.b2 = P + ob2;
  a.W3 = P + oW3; a.b3 = P + ob3; a.W4 = P + oW4; a.b4 = P + ob4;
  a.gW1 = G + oW1; a.gb1 = G + ob1; a.gW2 = G + oW2; a.gb2 = G + ob2;
  a.gW3 = G + oW3; a.gb3 = G + ob3; a.gW4 = G + oW4; a.gb4 = G + ob4;
  float* A = acts.data_ptr<float>();
  auto ap = [&](const char* n) {
    for (auto& p : act_off_)
      if (p.first == n) return A + p.second;
    throw std::runtime_error("mdt: act");
  };
  a.h1 = ap("h1"); a.mulv = ap("mulv"); a.eps = ap("eps"); a.z = ap("z"); a.h3 = ap("h3");
  a.dlog = ap("dlog"); a.dh3 = ap("dh3"); a.dmulv = ap("dmulv"); a.dh1 = ap("dh1");
  a.recon = want_recon ? ap("recon") : nullptr;
  a.xb = ap("xb");
  a.slab_mv = ap("slab_mv");
  a.slab_dz = ap("slab_dz");
  a.P = P; a.G = G;
  a.Mo = exp_avg.data_ptr<float>(); a.Vo = exp_avg_sq.data_ptr<float>();
  a.oW1 = oW1; a.ob1 = ob1; a.oW2 = oW2; a.ob2 = ob2;
  a.s_beg = oW3; a.s_end = total_;
  a.stamps = stamps_.defined() && stamps_.numel() > 0
                 ? reinterpret_cast<unsigned long long*>(stamps_.data_ptr<int64_t>())
                 : nullptr;
  a.partials = partials.data_ptr<float>();
  a.st = reinterpret_cast<TrainState*>((eval ? state.eval_state : state.train_state).data_ptr<uint8_t>());
  a.hp = reinterpret_cast<const HParams*>(state.hparams.data_ptr<uint8_t>());
}

void MlpVaeEngine::forward(const at::Tensor& X, const at::Tensor& idx, int64_t M, bool train,
                           bool eval, int64_t rng_stream, bool want_recon) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
  VaeArgs a;
  fill_args(&a, X, idx, M, train, eval, rng_stream, want_recon);
  const VaeGrid g = vae_grid(a);
  // KLD partial slots: F2 blocks of group 0 write 8 per batch row tile (NOT
  // g.f2 * 8: the other groups write none, and with a tail batch those slots
  // still hold the previous batch's partials -- round 4's eval loss summed them)
  last_f2_blocks_ = (int)((M + 15) / 16) * 8;
  last_f3_blocks_ = g.f3 * 8;
  check_rc(mdt_vae_forward(&a, c10::hip::getCurrentHIPStream().stream()), "vae forward");
}

void MlpVaeEngine::backward(const at::Tensor& X, const at::Tensor& idx, int64_t M, int64_t part,
                            bool fuse_adam) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
  VaeArgs a;
  fill_args(&a, X, idx, M, true, false, 0, false);
  a.fuse_adam = fuse_adam ? 1 : 0;
  a.dmulv_add = dmulv_add_.defined() ? dmulv_add_.data_ptr<float>() : nullptr;
  check_rc(mdt_vae_backward(&a, c10::hip::getCurrentHIPStream().stream(), (int)part),
           "vae backward");
}

void MlpVaeEngine::set_dmulv_add(c10::optional<at::Tensor> t) {
  if (!t.has_value() || !t->defined()) {
    dmulv_add_ = at::Tensor();
    return;
  }
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->numel() >= B_ * 2 * Z_,
              "set_dmulv_add: needs a contiguous CUDA float32 tensor of >= B*2Z elements");
  dmulv_add_ = *t;
}

void MlpVaeEngine::adam() {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
  check_rc(mdt_adam_step(params.data_ptr<float>(), grads.data_ptr<float>(),
                         exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(), total_,
                         reinterpret_cast<const HParams*>(state.hparams.data_ptr<uint8_t>()),
                         reinterpret_cast<TrainState*>(state.train_state.data_ptr<uint8_t>()),
                         c10::hip::getCurrentHIPStream().stream()),
           "adam");
}

void MlpVaeEngine::loss_finalize(bool eval) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
  check_rc(mdt_loss_finalize(reinterpret_cast<const HParams*>(state.hparams.data_ptr<uint8_t>()),
                             reinterpret_cast<TrainState*>(
                                 (eval ? state.eval_state : state.train_state).data_ptr<uint8_t>()),
                             partials.data_ptr<float>(), last_f2_blocks_, last_f3_blocks_,
                             c10::hip::getCurrentHIPStream().stream()),
           "loss finalize");
}

at::Tensor MlpVaeEngine::decode(const at::Tensor& z) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
  TORCH_CHECK(z.is_cuda() && z.scalar_type() == torch::kFloat32 && z.is_contiguous() &&
                  z.dim() == 2 && z.size(1) == Z_ && z.size(0) <= B_,
              "z must be a contiguous CUDA float32 [M<=B, Z] tensor");
  VaeArgs a;
  // X/idx are unused by the decode kernels; pass the parameter arena as a dummy
  // dataset view of the right width is not possible, so fill by hand.
  std::memset(&a, 0, sizeof(a));
  a.M = (int)z.size(0); a.B = (int)B_; a.D = (int)D_; a.H = (int)H_; a.Z = (int)Z_;
  float* P = params.data_ptr<float>();
  a.W3 = P + off_of(layout_, "fc3.weight"); a.b3 = P + off_of(layout_, "fc3.bias");
  a.W4 = P + off_of(layout_, "fc4.weight"); a.b4 = P + off_of(layout_, "fc4.bias");
  float* A = acts.data_ptr<float>();
  for (auto& p : act_off_) {
    if (p.first == "h3") a.h3 = A + p.second;
    if (p.first == "recon") a.recon = A + p.second;
  }
  check_rc(mdt_vae_decode(&a, z.data_ptr<float>(), c10::hip::getCurrentHIPStream().stream()),
           "vae decode");
  return act("recon", a.M).clone();
}

// ------------------------------------------------- importance-weighted pass ----
at::Tensor iw_state_new(int64_t device_index) {
  auto bopt = torch::TensorOptions().dtype(torch::kUInt8).device(torch::kCUDA, device_index);
  return torch::zeros({align64((int64_t)sizeof(IwState))}, bopt);
}

void iw_state_begin(at::Tensor state, int64_t nbatches) {
  TORCH_CHECK(nbatches > 0, "iw pass: nbatches must be positive");
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == torch::kUInt8 && state.numel() >= (int64_t)sizeof(IwState),
              "iw pass: state must come from iw_state_new");
  state.zero_();
  TrainState h;
  std::memset(&h, 0, sizeof(h));
  h.nbatches = (int32_t)nbatches;
  h.b1pow = h.b2pow = 1.0;
  h.sched_off = 1;  // no schedule enters the pass (its first kernel still advances the step there)
  auto cpu = torch::empty({(int64_t)offsetof(TrainState, loss_hist)}, torch::kUInt8);
  std::memcpy(cpu.data_ptr(), &h, offsetof(TrainState, loss_hist));
  state.narrow(0, 0, offsetof(TrainState, loss_hist)).copy_(cpu);
}

std::vector<double> iw_state_read(const at::Tensor& state) {
  auto cpu = state.to(torch::kCPU);
  const uint8_t* p = cpu.data_ptr<uint8_t>();
  TrainState h;
  std::memcpy(&h, p, offsetof(TrainState, loss_hist));
  double t[2];
  std::memcpy(t, p + offsetof(IwState, nll), sizeof(t));
  return {t[0], t[1], (double)h.step, (double)h.cursor};
}

void MlpVaeEngine::iw_begin(int64_t nbatches) {
  iw_state_begin(iw_state, nbatches);
  iw_nbatches_ = nbatches;
}

void MlpVaeEngine::iw_batch(const at::Tensor& X, const at::Tensor& idx, int64_t M, int64_t K, int64_t chunk,
                            at::Tensor row_nll, at::Tensor row_neg_elbo) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
  TORCH_CHECK(K >= 1 && chunk >= 1, "iw_batch: K and chunk must be >= 1");
  TORCH_CHECK((uint64_t)K * (uint64_t)B_ * (uint64_t)Z_ <= (1ull << 32), "iw_batch: K*B*Z exceeds 2^32");
  // mdt_iw_check's shape condition, before the encoder is launched
  TORCH_CHECK(kIwRowTile * ((H_ + 15) / 16 * 16 + 4) * (int64_t)sizeof(float) <= kIwMaxLds, "iw_batch: hidden size H = ",
              H_, " exceeds the importance-weighted pass's limit of 496 (64 KiB LDS decoder tile)");
  TORCH_CHECK(iw_nbatches_ > 0, "iw_batch: call iw_begin first");
  TORCH_CHECK(idx.numel() >= iw_nbatches_ * B_, "iw_batch: idx shorter than nbatches * B");
  for (const at::Tensor* t : {&row_nll, &row_neg_elbo})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous() &&
                    t->numel() >= iw_nbatches_ * B_,
                "iw_batch: row buffers must be contiguous CUDA float32 of >= nbatches * B elements");
  const int64_t S = std::min(chunk, K);
  if (S * B_ > iw_cap_ || !iw_ws_.defined()) {
    iw_cap_ = S * B_;
    const int64_t n = align64(iw_cap_ * H_) + 2 * align64(iw_cap_ * Z_) + 2 * align64(iw_cap_);
    iw_ws_ = torch::zeros({n}, params.options());
    iw_rowbuf_ = torch::zeros({3 * align64(B_)}, params.options());
  }
  VaeArgs a;
  fill_args(&a, X, idx, M, false, true, 0, false);
  a.st = reinterpret_cast<TrainState*>(iw_state.data_ptr<uint8_t>());  // IwState begins with its TrainState
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  check_rc(mdt_vae_encode(&a, stream), "iw encoder");
  IwArgs w;
  std::memset(&w, 0, sizeof(w));
  w.M = a.M; w.B = a.B; w.D = a.D; w.H = a.H; w.Z = a.Z;
  w.K = (int)K;
  w.cap_rows = (int)iw_cap_;
  w.rows_cap = (long long)std::min(row_nll.numel(), row_neg_elbo.numel());
  w.b2 = a.b2; w.W3 = a.W3; w.b3 = a.b3; w.W4 = a.W4; w.b4 = a.b4;
  w.slab_mv = a.slab_mv; w.xb = a.xb; w.mulv = a.mulv;
  float* ws = iw_ws_.data_ptr<float>();
  w.h3 = ws; ws += align64(iw_cap_ * H_);
  w.eps = ws; ws += align64(iw_cap_ * Z_);
  w.z = ws; ws += align64(iw_cap_ * Z_);
  w.prior = ws; ws += align64(iw_cap_);
  w.bce = ws;
  float* rb = iw_rowbuf_.data_ptr<float>();
  w.lse_m = rb; w.lse_s = rb + align64(B_); w.lw_sum = rb + 2 * align64(B_);
  w.row_nll = row_nll.data_ptr<float>();
  w.row_neg_elbo = row_neg_elbo.data_ptr<float>();
  w.ist = reinterpret_cast<IwState*>(iw_state.data_ptr<uint8_t>());
  w.hp = a.hp;
  for (int64_t k0 = 0; k0 < K; k0 += S) {
    w.k0 = (int)k0;
    w.S = (int)std::min(S, K - k0);
    w.first = k0 == 0 ? 1 : 0;
    w.last = k0 + S >= K ? 1 : 0;
    check_rc(mdt_iw_chunk(&w, stream), "iw chunk");
  }
}

std::vector<double> MlpVaeEngine::iw_read() { return iw_state_read(iw_state); }

at::Tensor MlpVaeEngine::iw_act(const std::string& name, int64_t S, int64_t M) {
  TORCH_CHECK(iw_ws_.defined() && S >= 1 && M >= 1 && S * M <= iw_cap_, "iw_act: no pass has run at this size");
  if (name == "h3") return iw_ws_.narrow(0, 0, S * M * H_).view({S * M, H_});
  int64_t off = align64(iw_cap_ * H_);  // the workspace layout of iw_batch: h3 | eps | z | prior | bce
  if (name == "eps" || name == "z") {
    if (name == "z") off += align64(iw_cap_ * Z_);
    return iw_ws_.narrow(0, off, S * M * Z_).view({S, M, Z_});
  }
  off += 2 * align64(iw_cap_ * Z_);
  if (name == "bce") off += align64(iw_cap_);
  else TORCH_CHECK(name == "prior", "iw_act: unknown buffer ", name);
  return iw_ws_.narrow(0, off, S * M).view({S, M});
}

// ------------------------------------------------------ latent report pass ----
void MlpVaeEngine::latent_begin(int64_t nbatches) {
  if (!latent_state.defined()) latent_state = latent_state_new(params.device().index());
  latent_state_begin(latent_state, nbatches);
  latent_nbatches_ = nbatches;
}

void MlpVaeEngine::latent_batch(const at::Tensor& X, const at::Tensor& idx, int64_t M, at::Tensor rows) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
  TORCH_CHECK(latent_nbatches_ > 0, "latent_batch: call latent_begin first");
  TORCH_CHECK(idx.numel() >= latent_nbatches_ * B_, "latent_batch: idx shorter than nbatches * B");
  TORCH_CHECK(rows.is_cuda() && rows.scalar_type() == torch::kFloat32 && rows.is_contiguous() &&
                  rows.numel() >= latent_nbatches_ * B_ * 2 * Z_,
              "latent_batch: rows must be contiguous CUDA float32 of >= nbatches * B * 2Z elements");
  VaeArgs a;
  fill_args(&a, X, idx, M, false, true, 0, false);
  a.st = reinterpret_cast<TrainState*>(latent_state.data_ptr<uint8_t>());  // LatentState begins with its TrainState
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  check_rc(mdt_vae_encode(&a, stream), "latent encoder");
  check_rc(mdt_latent_mulv(&a, stream), "latent mulv");
  latent_collect(act("mulv", M), M, B_, Z_, rows, latent_state);
}

std::vector<double> MlpVaeEngine::latent_read() {
  TORCH_CHECK(latent_state.defined(), "latent_read: no pass has run");
  return latent_state_read(latent_state);
}

// ----------------------------------------------- conv-VAE pass: small ops ----
static float* fptr(const at::Tensor& t, int64_t need, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() >= need, "iw: ",
              what, " must be a contiguous CUDA float32 tensor of >= ", need, " elements");
  return t.data_ptr<float>();
}

static void iw_reparam(const at::Tensor& mulv, int64_t M, int64_t B, int64_t Z, int64_t k0, int64_t S,
                       const at::Tensor& state, const at::Tensor& hparams, at::Tensor z16, at::Tensor z32,
                       at::Tensor eps, at::Tensor prior) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(mulv.device());
  TORCH_CHECK(M >= 1 && S >= 1 && S * M <= B, "iw_reparam: a chunk holds at most B virtual rows");
  TORCH_CHECK(state.numel() >= (int64_t)sizeof(IwState) && hparams.numel() >= (int64_t)sizeof(HParams),
              "iw_reparam: state / hparams buffers too small");
  TORCH_CHECK(z16.is_cuda() && z16.scalar_type() == torch::kBFloat16 && z16.is_contiguous() &&
                  z16.numel() >= S * M * Z,
              "iw_reparam: z16 must be contiguous CUDA bfloat16 of >= S*M*Z elements");
  check_rc(mdt_iw_reparam(fptr(mulv, M * 2 * Z, "mulv"), (int)M, (int)B, (int)Z, (int)k0, (int)S, state.data_ptr(),
                          hparams.data_ptr(), z16.data_ptr(), fptr(z32, S * M * Z, "z32"),
                          fptr(eps, S * M * Z, "eps"), fptr(prior, S * M, "prior"),
                          c10::hip::getCurrentHIPStream().stream()),
           "iw reparam");
}

static void iw_row_bce(const at::Tensor& logits, const at::Tensor& xb, int64_t V, int64_t M, int64_t P,
                       at::Tensor bce) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
  TORCH_CHECK(V >= 1 && M >= 1, "iw_row_bce: empty chunk");
  check_rc(mdt_iw_row_bce(fptr(logits, V * P, "logits"), fptr(xb, M * P, "xb"), (int)V, (int)M, (int)P,
                          fptr(bce, V, "bce"), c10::hip::getCurrentHIPStream().stream()),
           "iw row bce");
}

// rowbuf: [3][B] running max / scaled sum / sum of logw per batch row.
static void iw_reduce(const at::Tensor& prior, const at::Tensor& bce, at::Tensor rowbuf, at::Tensor row_nll,
                      at::Tensor row_neg_elbo, at::Tensor state, int64_t M, int64_t B, int64_t K, int64_t S,
                      bool first, bool last) {
  c10::hip::HIPGuardMasqueradingAsCUDA guard(prior.device());
  TORCH_CHECK(M >= 1 && M <= B && S >= 1 && S <= K, "iw_reduce: bad sizes");
  TORCH_CHECK(state.is_cuda() && state.numel() >= (int64_t)sizeof(IwState), "iw_reduce: state too small");
  IwArgs w;
  std::memset(&w, 0, sizeof(w));
  w.M = (int)M; w.B = (int)B; w.K = (int)K; w.S = (int)S;
  w.first = first ? 1 : 0; w.last = last ? 1 : 0;
  w.prior = fptr(prior, S * M, "prior");
  w.bce = fptr(bce, S * M, "bce");
  float* rb = fptr(rowbuf, 3 * B, "rowbuf");
  w.lse_m = rb; w.lse_s = rb + B; w.lw_sum = rb + 2 * B;
  w.rows_cap = (long long)std::min(row_nll.numel(), row_neg_elbo.numel());
  w.row_nll = fptr(row_nll, B, "row_nll");
  w.row_neg_elbo = fptr(row_neg_elbo, B, "row_neg_elbo");
  w.ist = reinterpret_cast<IwState*>(state.data_ptr());
  check_rc(mdt_iw_reduce(&w, c10::hip::getCurrentHIPStream().stream()), "iw reduce");
}

void bind_iw(pybind11::module& m) {
  namespace py = pybind11;
  m.def("iw_state_new", &iw_state_new, py::arg("device_index"));
  m.def("iw_state_begin", &iw_state_begin, py::arg("state"), py::arg("nbatches"));
  m.def("iw_state_read", &iw_state_read, py::arg("state"));
  m.def("iw_reparam", &iw_reparam, py::arg("mulv"), py::arg("M"), py::arg("B"), py::arg("Z"), py::arg("k0"),
        py::arg("S"), py::arg("state"), py::arg("hparams"), py::arg("z16"), py::arg("z32"), py::arg("eps"),
        py::arg("prior"));
  m.def("iw_row_bce", &iw_row_bce, py::arg("logits"), py::arg("xb"), py::arg("V"), py::arg("M"), py::arg("P"),
        py::arg("bce"));
  m.def("iw_reduce", &iw_reduce, py::arg("prior"), py::arg("bce"), py::arg("rowbuf"), py::arg("row_nll"),
        py::arg("row_neg_elbo"), py::arg("state"), py::arg("M"), py::arg("B"), py::arg("K"), py::arg("S"),
        py::arg("first"), py::arg("last"));
}

}  // namespace mdt
