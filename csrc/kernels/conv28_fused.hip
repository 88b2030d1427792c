// Fused 28x28 conv-VAE step kernels (gfx950) and their launchers.
//
//   f28_fwd_k   one workgroup per sample: forward (train or eval)
//   f28_bwd_k   one workgroup per sample: backward-data (two-launch form)
//   f28_step_k  forward + backward in one launch: grid 2M with two workgroups
//               per sample (conv28_pair.h; a leader whose partner is not
//               resident in time runs the solo body), or grid M solo
//
// Bodies: conv28_fused.h (solo), conv28_pair.h (pairs).
#include <stddef.h>
#include <stdlib.h>

#include <type_traits>

#include "conv28_pair.h"
#include "conv28_slots.h"
#include "conv_launch.h"

namespace mdt {
namespace f28 {

__global__ void __launch_bounds__(kThreads) f28_fwd_k(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[FwdLayout::LDS];
  fwd_body<FwdLayout>(a, lds, blockIdx.x);
}

__global__ void __launch_bounds__(kThreads) f28_bwd_k(BwdArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[BwdLayout::LDS];
  bwd_body<BwdLayout, false>(a, lds, blockIdx.x);
}

// Hand-off of the step's Adam constants to the next launch (PairCtl.adamc,
// null in eval launches): one thread of the workgroup that owns sample 0's
// backward -- the solo body, or role 0 of its pair; exactly one per training
// launch -- at its very end, where nothing else is live. Nothing writes
// TrainState during this launch (the next one advances it), and the kernel
// boundary publishes the buffer. The three pointers come from the
// kernel-argument segment (kptr, conv28_pair.h): taken from fa / pc they
// stayed in SGPRs across the whole kernel (98 -> 124 SGPR spills).
__device__ __forceinline__ void adamc_handoff(int n) {
  if (n != 0 || threadIdx.x != 0) return;
  AdamC* out = kptr<AdamC>(offsetof(StepKargs, pc.adamc));
  if (!out) return;
  *out = adam_consts_next(kptr<const TrainState>(offsetof(StepKargs, fa.st)),
                          kptr<const HParams>(offsetof(StepKargs, fa.hp)));
}

static_assert(StepLayout::LDS == 161216, "probe.hip probe_ramp launches with the step kernel's LDS bytes");

// The formal arguments serve the kernel's entry (pairing, P0, P1) only.
// Everything after P1 -- the paired body and the one solo body -- reads the
// argument segment where it needs a value, so no argument is live across the
// kernel.
__global__ void __launch_bounds__(kThreads) f28_step_k(FwdArgs fa, BwdArgs ba, PairCtl pc) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[StepLayout::LDS];
  if (pc.acquire) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  // pairing (see conv28_pair.h): ticket at entry, the leader's solo claim
  // after P0 (its result is needed only after P1, which both forms share).
  // A launch without pairs (grid M) enters the solo body the same way.
  const bool pair = pc.pair != 0;
  const int n = pair ? (int)blockIdx.x % pc.M : (int)blockIdx.x;
  g32i* word = (g32i*)(pc.pairw + n);
  int ticket = 0, seen = 1;
  if (pair) {
    if (pc.delay_us > 0 && (int)blockIdx.x >= pc.M && threadIdx.x == 0) {  // tests: a partner that comes late
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      while (__builtin_amdgcn_s_memrealtime() - t0 < 100ull * (unsigned)pc.delay_us) __builtin_amdgcn_s_sleep(8);
    }
    if (threadIdx.x == 0) ticket = __hip_atomic_fetch_add(word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  fwd_p01<StepLayout>(fa, lds, n, [&] {
    if (pair && threadIdx.x == 0 && ticket == 0)
      __hip_atomic_compare_exchange_strong(word, &seen, 3, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
  });
  int* mode_w = reinterpret_cast<int*>(lds + StepLayout::Scr + 124);  // Scr[31]: unused before P4
  if (pair && threadIdx.x == 0) {
    int mode;
    if (ticket == 0) {
      mode = seen == 1 ? kModeSolo : kModeRole0;  // CAS 1 -> 3 won: solo; saw 2: the partner is in
      if (mode == kModeRole0) __hip_atomic_store(word, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (ticket == 1) {
      mode = kModeRole1;
    } else {  // the leader went solo before this workgroup arrived: last to touch the word
      mode = kModeExit;
      __hip_atomic_store(word, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    *mode_w = mode;
    if (fa.stamps) fa.stamps[blockIdx.x * 16 + 15] = (unsigned long long)mode;
  }
  lds_barrier();
  const int mode = pair ? __builtin_amdgcn_readfirstlane(*mode_w) : (int)kModeSolo;
  if (mode == kModeExit) return;
  if (__builtin_expect(mode != kModeSolo, 1)) {
    if (kval<int>(offsetof(StepKargs, pc.delay_us)) < 0 && mode == kModeRole1 && n == 0) {
      // tests: a paired half that stalls (sweep timeout)
      if (threadIdx.x == 0) {
        const unsigned delay = (unsigned)-kval<int>(offsetof(StepKargs, pc.delay_us));
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < 100ull * delay) __builtin_amdgcn_s_sleep(64);
      }
      lds_barrier();
    }
    pair_rest<StepLayout>(lds, n, mode == kModeRole1 ? 1 : 0);
    if (mode == kModeRole0) adamc_handoff(n);
    return;
  }
  // The solo body (a launch without pairs, or a leader whose partner was not
  // resident in time), after the paired path in the code. Its arguments are
  // read through the segment too.
  const StepKargs& ka = *(const StepKargs*)(const void*)kargs();
  fwd_rest<StepLayout>(ka.fa, lds, n);
  if (!ka.fa.train) return;  // eval: forward only
  lds_barrier();
  bwd_body<StepLayout, true>(ka.ba, lds, n);
  adamc_handoff(n);
}

}  // namespace f28
}  // namespace mdt

using namespace mdt;

namespace {

// One slot of a table (conv28_slots.h) into the argument member of its name.
// The slot's dtype tag, which the bindings check the tensor against, must be
// the member's element type.
template <char Tag, class T>
void put(T*& member, const long long* p, int slot) {
  using E = std::remove_const_t<T>;
  static_assert(Tag == 'f'   ? std::is_same_v<E, float>
                : Tag == 'b' ? std::is_same_v<E, __bf16>
                : Tag == 'i' ? std::is_same_v<E, int> || std::is_same_v<E, unsigned>
                : Tag == 'l' ? std::is_same_v<E, unsigned long long>
                : Tag == 'u' ? std::is_same_v<E, TrainState> || std::is_same_v<E, HParams>
                             : false,
                "conv28_slots.h: the slot's dtype tag is not the argument member's element type");
  member = reinterpret_cast<T*>((intptr_t)p[slot]);
}

void fill_weights(f28::Weights& w, const long long* p) {
#define MDT_PUT(name, tag, ...) put<tag>(w.name, p, f28::kW_##name);
  MDT_F28_WEIGHT_SLOTS(MDT_PUT)
#undef MDT_PUT
}

void fill_fwd(f28::FwdArgs& a, const long long* p, int B, unsigned stream, int train) {
  fill_weights(a.w, p);
  put<f28::kFwdSlots[f28::kFwd_state].dtype>(a.st, p, f28::kFwd_state);
  put<f28::kFwdSlots[f28::kFwd_hparams].dtype>(a.hp, p, f28::kFwd_hparams);
#define MDT_PUT(name, tag, ...) put<tag>(a.name, p, f28::kFwd_##name);
  MDT_F28_FWD_BUFFER_SLOTS(MDT_PUT)
#undef MDT_PUT
  a.B = B;
  a.stream = stream;
  a.train = train;
  a.pf_slices = 16;
}

void fill_bwd(f28::BwdArgs& a, const long long* p, int M, const TrainState* st) {
  fill_weights(a.w, p);
  const HParams* hp;
  put<f28::kBwdSlots[f28::kBwd_hparams].dtype>(hp, p, f28::kBwd_hparams);
  a.klw = st ? &st->kl_next : &hp->kl_beta;  // device addresses, not dereferenced here
  a.fbw = st ? &st->fb_t : &hp->free_bits;
#define MDT_PUT(name, tag, ...) put<tag>(a.name, p, f28::kBwd_##name);
  MDT_F28_BWD_BUFFER_SLOTS(MDT_PUT)
#undef MDT_PUT
  a.db2_m2 = M;  // db2_part is always [2][M][64] (second row: the paired step's role-1 half)
}

// false: no pair table, or one with a null slot
bool fill_pair(f28::PairCtl& pc, const long long* pp) {
  if (!pp) return false;
#define MDT_PUT(name, tag, ...) put<tag>(pc.name, pp, f28::kPair_##name);
  MDT_F28_PAIR_SLOTS(MDT_PUT)
#undef MDT_PUT
  return pc.xg && pc.pairw && pc.err;
}

}  // namespace

extern "C" {

int mdt_f28_forward(const long long* p, int B, int M, unsigned stream, int train, hipStream_t s) {
  if (M <= 0 || M > B) return 1;
  f28::FwdArgs a{};
  fill_fwd(a, p, B, stream, train);
  hipLaunchKernelGGL(f28::f28_fwd_k, dim3(M), dim3(f28::kThreads), 0, s, a);
  return (int)hipGetLastError();
}

int mdt_f28_pair_words() { return f28::kXW; }

// Forward only (eval: train = 0) through the step kernel's paired form: two
// workgroups per sample, so an eval batch of M samples fills 2M CUs instead of
// the solo f28_fwd_k's M. Same arithmetic as the solo forward (the paired and
// solo forms are bitwise equal); the backward half of the kernel is skipped.
int mdt_f28_forward_pair(const long long* p, const long long* pp, int B, int M, unsigned stream, hipStream_t s) {
  if (M <= 0 || M > B) return 1;
  f28::FwdArgs fa{};
  fill_fwd(fa, p, B, stream, 0);
  fa.pf_slices = 0;
  f28::BwdArgs ba{};
  f28::PairCtl pc{};
  if (!fill_pair(pc, pp)) return 2;
  pc.M = M;
  pc.pair = 1;
  hipLaunchKernelGGL(f28::f28_step_k, dim3(2 * M), dim3(f28::kThreads), 0, s, fa, ba, pc);
  return (int)hipGetLastError();
}

// One launch per training step: forward then backward, two workgroups per
// sample when `pair` (pp = pair table), else one.
int mdt_f28_step(const long long* pf, const long long* pb, const long long* pp, int B, int M, unsigned stream,
                 int pair, int delay_us, float* adamc, hipStream_t s) {
  if (M <= 0 || M > B) return 1;
  f28::FwdArgs fa{};
  fill_fwd(fa, pf, B, stream, 1);
  f28::BwdArgs ba{};
  fill_bwd(ba, pb, M, fa.st);
  f28::PairCtl pc{};
  pc.M = M;
  pc.pair = pair ? 1 : 0;
  pc.delay_us = delay_us;
  pc.adamc = reinterpret_cast<AdamC*>(adamc);  // 64 B, 16-B aligned (checked by the caller)
  static const int acq = [] {
    const char* e = getenv("MDT_F28_ACQ");
    return e && e[0] == '1' ? 1 : 0;
  }();
  pc.acquire = acq;
  if (pair) {
    if (!fill_pair(pc, pp)) return 2;
    // no P0 L2 prefetch in the paired form: measured 0.0636-0.0639 vs
    // 0.0638-0.0644 ms/step on the driver command with 32 slices, 200/20
    // 0.0608-0.0613 vs 0.0616-0.0622 (profiles/r4_end, gpurun_out r4af/r4ag)
    fa.pf_slices = 0;
  }
  static const int pf_env = [] {  // A/B: MDT_F28_PF = L2-prefetch slices per XCD (0 = no prefetch)
    const char* e = getenv("MDT_F28_PF");
    return e ? atoi(e) : -1;
  }();
  if (pf_env >= 0) fa.pf_slices = pf_env;
  hipLaunchKernelGGL(f28::f28_step_k, dim3(pair ? 2 * M : M), dim3(f28::kThreads), 0, s, fa, ba, pc);
  return (int)hipGetLastError();
}

// `st` (optional): the training state whose step the NEXT launch advances
int mdt_f28_backward(const long long* p, int M, const void* st, hipStream_t s) {
  if (M <= 0) return 1;
  f28::BwdArgs a{};
  fill_bwd(a, p, M, reinterpret_cast<const TrainState*>(st));
  hipLaunchKernelGGL(f28::f28_bwd_k, dim3(M), dim3(f28::kThreads), 0, s, a);
  return (int)hipGetLastError();
}

}  // extern "C"
