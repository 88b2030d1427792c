// The tile families of the conv kernels, each listed ONCE: configuration index
// -> tile type. A visitor calls f(TileTag<T>{}) for the type of `cfg` (false: no
// such index); launchers, job grids, plans and LDS maxima read the lists through these.
#pragma once
#include "conv_direct.h"
#include "conv_igemm_dev.h"

namespace mdt {

template <class T>
struct TileTag {
  using type = T;
};

// forward-type GEMM tiles; the planner's index of a tile size
constexpr int kNumFwdTiles = 8;
constexpr int fwd_tile_cfg(int bm, int bn) {
  return (bm == 128 ? 0 : 4) + (bn == 128 ? 0 : bn == 64 ? 1 : bn == 32 ? 2 : 3);
}
template <class F>
constexpr bool visit_fwd_tile(int cfg, F&& f) {
  using namespace tiles;
  switch (cfg) {
    case 0: f(TileTag<F0>{}); return true;
    case 1: f(TileTag<F1>{}); return true;
    case 2: f(TileTag<F2>{}); return true;
    case 3: f(TileTag<F3>{}); return true;
    case 4: f(TileTag<F4>{}); return true;
    case 5: f(TileTag<F5>{}); return true;
    case 6: f(TileTag<F6>{}); return true;
    case 7: f(TileTag<F7>{}); return true;
  }
  return false;
}

// weight-gradient tiles (co x k')
constexpr int kNumWgTiles = 6;
constexpr int wg_tile_cfg(int bm, int bn) { return (bm == 64 ? 0 : 3) + (bn == 64 ? 0 : bn == 32 ? 1 : 2); }
template <class F>
constexpr bool visit_wg_tile(int cfg, F&& f) {
  using namespace tiles;
  switch (cfg) {
    case 0: f(TileTag<W0>{}); return true;
    case 1: f(TileTag<W1>{}); return true;
    case 2: f(TileTag<W2>{}); return true;
    case 3: f(TileTag<W3>{}); return true;
    case 4: f(TileTag<W4>{}); return true;
    case 5: f(TileTag<W5>{}); return true;
  }
  return false;
}

// each list holds, at the index the planner computes from a tile size, that tile
constexpr bool tile_lists_ok() {
  bool ok = true;
  for (int cfg = 0; cfg < kNumFwdTiles; ++cfg)
    ok &= visit_fwd_tile(cfg, [&](auto t) { ok &= fwd_tile_cfg(decltype(t)::type::BM, decltype(t)::type::BN) == cfg; });
  for (int cfg = 0; cfg < kNumWgTiles; ++cfg)
    ok &= visit_wg_tile(cfg, [&](auto t) { ok &= wg_tile_cfg(decltype(t)::type::BM, decltype(t)::type::BN) == cfg; });
  return ok && !visit_fwd_tile(kNumFwdTiles, [](auto) {}) && !visit_wg_tile(kNumWgTiles, [](auto) {});
}
static_assert(tile_lists_ok(), "a tile list and the planner's configuration index disagree");

// patch-resident direct configurations (conv_direct.h). 4 and 5, the
// 16x16 <-> 8x8 tiles, are forward-only and have no job form.
constexpr int kNumDirectJobCfgs = 4;
template <class F>
constexpr bool visit_direct(int dc, F&& f) {
  switch (dc) {
    case 0: f(TileTag<DcS1>{}); return true;
    case 1: f(TileTag<DcS2>{}); return true;
    case 2: f(TileTag<DcT2>{}); return true;
    case 3: f(TileTag<DcT3>{}); return true;
    case 4: f(TileTag<DcS3>{}); return true;
    case 5: f(TileTag<DcT1>{}); return true;
  }
  return false;
}

}  // namespace mdt
