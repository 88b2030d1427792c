// Host-only planners of the conv-VAE GEMMs: which kernel and tiling a geometry
// runs with (FwdPlan / WgradPlan, conv_igemm.h). No kernel lives here; hipcc
// compiles the file because the tile constants come from the device headers.
// Deterministic in geometry and environment: the trainer sizes its buffers up front.
#include <stdlib.h>

#include <algorithm>

#include "conv_dwgrad.h"
#include "conv_host.h"
#include "conv_launch.h"
#include "conv_thin_wg.h"
#include "conv_tiles.h"

namespace mdt {
namespace {

int env_int(const char* name, int def) {
  const char* e = getenv(name);
  return e ? atoi(e) : def;
}
bool env_on(const char* name) {  // on unless set to 0...
  const char* e = getenv(name);
  return !(e && e[0] == '0');
}

// The planner overrides (docs/KNOBS.md), parsed once per process: {variable, default,
// parser} each. MDT_DWGRAD_L2 is not among them: dwgrad_cfg reads it on every plan.
struct Overrides {
  // 64-row tiles when 128-row tiles would leave the grid under this many
  // blocks (default 1024 = 4 per CU, measured 3 % faster than 512 on the
  // 128x128 step and 0.5 % on the 28x28 one, profiles/r1_knobs)
  int bm64_below = env_int("MDT_CONV_BM64_BELOW", 1024);
  // narrower column tiles for deep (>= bn_split_min_kt = 16 k-tiles) problems
  // whose grid would stay under bn_split_below = 512 blocks: more workgroups
  // in flight for the wide-N, short-M 128x128 layers (4 % on that step);
  // shallow ones (the 28x28 decoder Linear, K = 32) lose from the extra A
  // re-reads, so they keep their tiles (profiles/r1_knobs)
  int bn_split_below = env_int("MDT_CONV_BN_SPLIT_BELOW", 512);
  int bn_split_min_kt = env_int("MDT_CONV_BN_SPLIT_MIN_KT", 16);
  // ... and, at any depth, while the grid would stay under bn_split_tiny = 512
  // blocks: the shallow Linear GEMMs (the 28x28 decoder Linear / head
  // backward-data, M = 128: 50 blocks of 64x128; the 128x128 model's dec_fc
  // forward and head backward-data, M = 64, K <= 128: 128 blocks) spread over
  // more CUs. 64 -> 512 measured conv128 B=64 0.3727-0.374 -> 0.3644-0.3645
  // ms/step, 1024 0.3767 (profiles/r4_tiles); 28x28 layer path:
  // profiles/r1_defer/bn_tiny
  int bn_split_tiny = env_int("MDT_CONV_BN_SPLIT_TINY", 512);
  // split-K only for deep problems (>= 8 k-tiles) whose grid is under-filled;
  // the combine is fused into a following launch where the model allows it
  // (enc_head -> reparam, dec_fc dgrad -> reparam backward)
  int split_min_kt = env_int("MDT_CONV_SPLIT_MIN_KT", 8);
  // at least this many k-tiles per split (default 1): fewer k-steps per block
  // against more partial slabs for the combine pass to read; 1 measured 3 %
  // faster than 4 on the 28x28 step (profiles/r1_knobs)
  int split_kt_per = std::max(1, env_int("MDT_CONV_SPLIT_KT_PER", 1));
  // pins the weight gradient's block target (0: the default rule of plan_wgrad)
  int wg_target = env_int("MDT_CONV_WG_TARGET", 0);
  // ... of the single-channel-input (thin) layers only: their finalize sits
  // on the optimizer tail
  int wg_target_thin = env_int("MDT_CONV_WG_TARGET_THIN", 0);
  // 0 keeps every layer on the im2col kernels
  bool direct = env_on("MDT_CONV_DIRECT");
  // 0: forward calls only (backward-data keeps the fusable im2col kernel)
  bool dconv_bwd = env_on("MDT_DCONV_BWD");
  // the 16x16 <-> 8x8 geometries (0 keeps them on im2col)
  bool dconv_small = env_on("MDT_DCONV_SMALL");
  // 0 keeps every weight gradient on the im2col kernel
  bool dwgrad = env_on("MDT_DWGRAD");
};

const Overrides& overrides() {
  static const Overrides o;
  return o;
}

}  // namespace

// Patch-resident direct kernel (conv_direct.h) for a geometry: configuration
// index, or -1.
int direct_cfg(int mode, const ConvDesc& d, bool fwd) {
  const Overrides& o = overrides();
  // the two-workgroups-per-CU tiles (R = 4): measured 15-18 % faster than
  // one-per-CU R = 8 tiles and 3-4 % faster than three-per-CU R = 2 tiles at
  // B = 64 and 128 (profiles/r2_dconv)
  if (!o.direct || d.KH != 4 || d.KW != 4 || d.S != 2 || d.P != 1) return -1;
  if (!fwd && !o.dconv_bwd) return -1;
  if (d.H != d.W || d.OH != d.OW || d.H != 2 * d.OH) return -1;
  if (mode == kModeConv) {  // A = input (H, C), columns = CO
    if (d.C == 32 && d.H == 64 && d.CO == 64) return 0;
    if (d.C == 64 && d.H == 32 && d.CO == 128) return 1;
    // 16x16 -> 8x8: forward only; as a backward-data GEMM the im2col kernel
    // fuses with the weight gradient in one launch, which measured faster
    if (d.C == 128 && d.H == 16 && d.CO == 256 && fwd && o.dconv_small) return 4;
  } else {  // A = conv output (OH, CO), columns = C
    if (d.CO == 128 && d.OH == 16 && d.C == 64) return 2;
    if (d.CO == 64 && d.OH == 32 && d.C == 32) return 3;
    if (d.CO == 256 && d.OH == 8 && d.C == 128 && fwd && o.dconv_small) return 5;
  }
  return -1;
}

bool plan_fwd(int mode, const ConvDesc& d, bool allow_split, FwdPlan* p, bool allow_direct, bool fwd) {
  const Overrides& o = overrides();
  FwdPlan q{};
  const int dc = allow_direct ? direct_cfg(mode, d, fwd) : -1;
  if (dc >= 0) {
    q.direct = dc + 1;
    q.classes = mode == kModeConv ? 1 : 4;
    q.M = mode == kModeConv ? d.N * d.OH * d.OW : d.N * d.OH * d.OW;
    q.Ncols = mode == kModeConv ? d.CO : d.C;
    q.K = mode == kModeConv ? 16 * d.C : 4 * d.CO;
    visit_direct(dc, [&](auto t) {
      using CF = typename decltype(t)::type;
      q.BM = CF::MT; q.BN = CF::NB;
      q.mtiles = d.N * CF::RB; q.ntiles = CF::NBB;
      q.colsum_rows = d.N * CF::RB;
    });
    q.ktiles = q.K / 64;
    q.ksplit = 1; q.kt_per_split = q.ktiles;
    q.cfg = kFwdDirectBase + dc;
    *p = q;
    return true;
  }
  if (mode == kModeConv) {
    q.classes = 1;
    q.M = d.N * d.OH * d.OW;
    q.Ncols = d.CO;
    q.K = d.KH * d.KW * d.C;
    q.thin = (d.C % 8) != 0;
  } else {
    if (d.KH % d.S || d.KW % d.S || d.H % d.S || d.W % d.S || d.CO % 8) return false;
    q.classes = d.S * d.S;
    q.M = d.N * (d.H / d.S) * (d.W / d.S);
    q.Ncols = d.C;
    q.K = (d.KH / d.S) * (d.KW / d.S) * d.CO;
    q.thin = 0;
  }
  if (q.K % 8 || q.M <= 0) return false;
  q.BN = q.Ncols >= 128 ? 128 : q.Ncols > 32 ? 64 : q.Ncols > 16 ? 32 : 16;
  if (q.thin) q.BN = 32;
  auto grid64 = [&] { return (long long)q.classes * cdiv(q.M, 64) * cdiv(q.Ncols, q.BN); };
  while (q.BN > 32 && !q.thin &&
         ((cdiv(q.K, 64) >= o.bn_split_min_kt && grid64() < o.bn_split_below) || grid64() < o.bn_split_tiny))
    q.BN /= 2;
  q.ntiles = cdiv(q.Ncols, q.BN);
  q.ktiles = cdiv(q.K, 64);
  q.BM = 128;
  if ((long long)q.classes * cdiv(q.M, 128) * q.ntiles < o.bm64_below) q.BM = 64;
  q.mtiles = cdiv(q.M, q.BM);
  const long long blocks = (long long)q.classes * q.mtiles * q.ntiles;
  q.ksplit = 1;
  if (allow_split && q.classes == 1 && blocks < 256 && q.ktiles >= o.split_min_kt) {
    int ks = cdiv(512, blocks);
    if (ks > q.ktiles / o.split_kt_per) ks = q.ktiles / o.split_kt_per;
    if (ks < 1) ks = 1;
    q.ksplit = ks;
  }
  q.kt_per_split = cdiv(q.ktiles, q.ksplit);
  q.ksplit = cdiv(q.ktiles, q.kt_per_split);
  q.colsum_rows = q.classes * q.mtiles;
  q.cfg = fwd_tile_cfg(q.BM, q.BN);
  *p = q;
  return true;
}

// Direct weight-gradient geometry (conv_dwgrad.h) of `d`: 0 = DwL1, 1 = DwL2,
// -1 = none. DwL2 (the 32x32x64 -> 16x16x128 layer) only with MDT_DWGRAD_L2=1:
// its [N][128][1024] partial rows are 4x the im2col kernel's slab.
int dwgrad_cfg(const ConvDesc& d) {
  const char* e2 = getenv("MDT_DWGRAD_L2");  // read per plan (tests switch it inside one process)
  const bool l2 = e2 && e2[0] == '1';
  if (!overrides().dwgrad || d.S != 2 || d.P != 1 || d.KH != 4 || d.KW != 4 || d.H != d.W || d.OH != d.OW ||
      d.OH * 2 != d.H)
    return -1;
  if (d.H == DwL1::H && d.C == DwL1::C && d.CO == DwL1::CO) return 0;
  if (l2 && d.H == DwL2::H && d.C == DwL2::C && d.CO == DwL2::CO) return 1;
  return -1;
}

bool plan_wgrad(const ConvDesc& d, WgradPlan* p) {
  const Overrides& o = overrides();
  WgradPlan q{};
  if (d.CO % 8) return false;
  q.M = d.N * d.OH * d.OW;
  q.K2 = d.KH * d.KW * d.C;
  const bool thin_mfma = thin_wgrad_mfma_ok(d);  // conv_thin_wg.h: one partial row per 4 output rows
  const int dw = thin_mfma ? -1 : dwgrad_cfg(d);  // one partial row per image (the workgroups of its four kernel rows)
  if (thin_mfma || dw >= 0) {
    q.cfg = thin_mfma ? kWgThinMfma : kWgDirectBase + dw;
    q.thin = thin_mfma;
    q.BM = d.CO;
    q.BN = q.K2;
    q.cotiles = q.ktiles = 1;
    q.mtiles = thin_mfma ? d.N * d.OH / 4 : d.N;
    q.nsplit = q.mtiles;
    q.mt_per_split = 1;
    *p = q;
    return true;
  }
  q.thin = (d.C % 8) != 0;
  q.BM = d.CO > 32 ? 64 : 32;
  q.BN = q.K2 > 32 ? 64 : q.K2 > 16 ? 32 : 16;
  if (q.thin && q.BN == 32) q.BN = 64;
  q.cotiles = cdiv(d.CO, q.BM);
  q.ktiles = cdiv(q.K2, q.BN);
  q.mtiles = cdiv(q.M, 64);
  const int tiles = q.cotiles * q.ktiles;
  // m-splits so the grid reaches ~`target` blocks. Default: ~16 m-steps per
  // block, clamped to [160, 640] blocks -- measured on MI355X (profiles/r1_knobs):
  // the 28x28 layers (98 m-tiles) want few splits (fewer partial slabs for the
  // finalize to read), the 128x128 layers (up to 4096 m-tiles) want the grid
  // wide (a 320-block grid left ~200 serial m-steps per block).
  int target = q.thin && o.wg_target_thin > 0 ? o.wg_target_thin : o.wg_target;
  if (target <= 0) {
    const long long work = (long long)q.mtiles * tiles;
    target = (int)std::min<long long>(640, std::max<long long>(160, work / 16));
  }
  int ns = cdiv(target, tiles);
  if (ns > q.mtiles / 2) ns = q.mtiles / 2;
  if (ns < 1) ns = 1;
  q.mt_per_split = cdiv(q.mtiles, ns);
  q.nsplit = cdiv(q.mtiles, q.mt_per_split);
  q.cfg = wg_tile_cfg(q.BM, q.BN);
  *p = q;
  return true;
}

}  // namespace mdt

extern "C" {

int mdt_igemm_plan(int mode, mdt::ConvDesc d, int allow_split, int fwd, mdt::FwdPlan* q) {
  return mdt::plan_fwd(mode, d, allow_split != 0, q, true, fwd != 0) ? 0 : 1;
}

int mdt_wgrad_plan(mdt::ConvDesc d, mdt::WgradPlan* q) { return mdt::plan_wgrad(d, q) ? 0 : 1; }

}  // extern "C"
