// The argument tables of the fused 28x28 step launches (conv28_fused.hip), once.
// A launch takes its buffers as a table of device addresses (const long long*);
// these lists are the only place that says which slot holds what. From them
// come the slot indices and the host checks of the bindings
// (csrc/runtime/conv_ops.cpp), the names the Python side passes its tensors
// under (C.f28_slot_names()), and the stores into the kernels' argument
// structs (fill_* in conv28_fused.hip). Host-clean: g++ and hipcc include it.
//
// One row per slot: S(name, dtype tag, count, unit, need).
//   tag    'f' float32, 'b' bfloat16, 'i' int32, 'l' int64, 'u' uint8 bytes of a TrialState buffer
//   count  elements the tensor must hold at least, in `unit`s
//   need   kRequired; kOptional (null when absent); kTrainOnly (required by a
//          training launch, optional in an eval forward, which stores no activations)
// A row's name is the member it fills: of f28::Weights, of FwdArgs / BwdArgs
// (the *_BUFFER_SLOTS) and of PairCtl. The state blobs are stored by hand.
#pragma once

namespace mdt {
namespace f28 {

enum SlotUnit : int {
  kFixed,         // count elements
  kPerSample,     // count elements per sample of the launch (M)
  kPerBatchRow,   // count elements per row of a whole batch (B)
  kTrainState,    // sizeof(TrainState) bytes
  kHParams,       // sizeof(HParams) bytes
  kPairGranules,  // count * mdt_f28_pair_words() elements per sample
};
enum SlotNeed : int { kRequired, kOptional, kTrainOnly };

struct Slot {
  const char* name;
  char dtype;
  int count;
  SlotUnit unit;
  SlotNeed need;
};

// (weight, bias) per layer in spec order; the single-channel edge layers read their f32 masters
#define MDT_F28_WEIGHT_SLOTS(S)             \
  S(W1f, 'f', 512, kFixed, kRequired)       \
  S(b1, 'f', 32, kFixed, kRequired)         \
  S(W2, 'b', 32768, kFixed, kRequired)      \
  S(b2, 'f', 64, kFixed, kRequired)         \
  S(Wh, 'b', 200704, kFixed, kRequired)     \
  S(bh, 'f', 64, kFixed, kRequired)         \
  S(Wd, 'b', 100352, kFixed, kRequired)     \
  S(bd, 'f', 3136, kFixed, kRequired)       \
  S(W3, 'b', 32768, kFixed, kRequired)      \
  S(b3, 'f', 32, kFixed, kRequired)         \
  S(W4f, 'f', 512, kFixed, kRequired)       \
  S(b4, 'f', 1, kFixed, kRequired)

// X is [rows][784] and idx whole batches of B (cursor * B + n indexes it)
#define MDT_F28_FWD_BUFFER_SLOTS(S)         \
  S(X, 'f', 784, kFixed, kRequired)         \
  S(idx, 'i', 1, kPerBatchRow, kRequired)   \
  S(xb, 'f', 784, kPerSample, kTrainOnly)   \
  S(a1, 'b', 6272, kPerSample, kTrainOnly)  \
  S(a2, 'b', 3136, kPerSample, kTrainOnly)  \
  S(mulv, 'f', 64, kPerSample, kTrainOnly)  \
  S(eps, 'f', 32, kPerSample, kTrainOnly)   \
  S(z16, 'b', 32, kPerSample, kTrainOnly)   \
  S(d0, 'b', 3136, kPerSample, kTrainOnly)  \
  S(d1, 'b', 6272, kPerSample, kTrainOnly)  \
  S(dlog, 'f', 784, kPerSample, kTrainOnly) \
  S(recon, 'f', 784, kPerSample, kOptional) \
  S(bce_part, 'f', 1, kPerSample, kRequired) \
  S(kld_part, 'f', 1, kPerSample, kRequired) \
  S(db4_part, 'f', 1, kPerSample, kOptional) \
  S(stamps, 'l', 32, kPerSample, kOptional) \
  S(xn, 'f', 784, kPerSample, kOptional)    \
  S(xtag, 'i', 1, kPerSample, kOptional)

#define MDT_F28_FWD_SLOTS(S)                \
  MDT_F28_WEIGHT_SLOTS(S)                   \
  S(state, 'u', 1, kTrainState, kRequired)  \
  S(hparams, 'u', 1, kHParams, kRequired)   \
  MDT_F28_FWD_BUFFER_SLOTS(S)

// db2_part is [2][M][64]: a row per half of a pair
#define MDT_F28_BWD_BUFFER_SLOTS(S)             \
  S(mulv, 'f', 64, kPerSample, kRequired)       \
  S(eps, 'f', 32, kPerSample, kRequired)        \
  S(a1, 'b', 6272, kPerSample, kRequired)       \
  S(a2, 'b', 3136, kPerSample, kRequired)       \
  S(d0, 'b', 3136, kPerSample, kRequired)       \
  S(d1, 'b', 6272, kPerSample, kRequired)       \
  S(dlog, 'f', 784, kPerSample, kRequired)      \
  S(gd1, 'b', 6272, kPerSample, kRequired)      \
  S(gd0, 'b', 3136, kPerSample, kRequired)      \
  S(dbd_part, 'f', 3136, kPerSample, kRequired) \
  S(dmulv, 'f', 64, kPerSample, kRequired)      \
  S(dmulv16, 'b', 64, kPerSample, kRequired)    \
  S(ga2, 'b', 3136, kPerSample, kRequired)      \
  S(ga1, 'b', 6272, kPerSample, kRequired)      \
  S(db3_part, 'f', 32, kPerSample, kRequired)   \
  S(db2_part, 'f', 128, kPerSample, kRequired)  \
  S(db1_part, 'f', 32, kPerSample, kRequired)   \
  S(stamps, 'l', 32, kPerSample, kOptional)

#define MDT_F28_BWD_SLOTS(S)                \
  MDT_F28_WEIGHT_SLOTS(S)                   \
  S(hparams, 'u', 1, kHParams, kRequired)   \
  MDT_F28_BWD_BUFFER_SLOTS(S)

// paired launches: exchange granules [M][2][f28_pair_words()], pairing words [M], error word;
// all zero before the first launch
#define MDT_F28_PAIR_SLOTS(S)               \
  S(xg, 'l', 2, kPairGranules, kRequired)   \
  S(pairw, 'i', 1, kPerSample, kRequired)   \
  S(err, 'i', 1, kFixed, kRequired)

// A table and its indices from a list: kW_NAME / kFwd_NAME / kBwd_NAME / kPair_NAME is the slot's place in its
// table. The weights lead both launch tables, so kW_NAME indexes them in either.
#define MDT_F28_SLOT_ROW(name, dtype, count, unit, need) {#name, dtype, count, unit, need},
#define MDT_F28_SLOT_TABLE(table, size, LIST, INDEX) \
  enum : int { LIST(INDEX) size };                   \
  constexpr Slot table[size] = {LIST(MDT_F28_SLOT_ROW)};
#define MDT_F28_W_INDEX(name, ...) kW_##name,
#define MDT_F28_FWD_INDEX(name, ...) kFwd_##name,
#define MDT_F28_BWD_INDEX(name, ...) kBwd_##name,
#define MDT_F28_PAIR_INDEX(name, ...) kPair_##name,
MDT_F28_SLOT_TABLE(kWeightSlots, kNumWeightSlots, MDT_F28_WEIGHT_SLOTS, MDT_F28_W_INDEX)
MDT_F28_SLOT_TABLE(kFwdSlots, kNumFwdSlots, MDT_F28_FWD_SLOTS, MDT_F28_FWD_INDEX)
MDT_F28_SLOT_TABLE(kBwdSlots, kNumBwdSlots, MDT_F28_BWD_SLOTS, MDT_F28_BWD_INDEX)
MDT_F28_SLOT_TABLE(kPairSlots, kNumPairSlots, MDT_F28_PAIR_SLOTS, MDT_F28_PAIR_INDEX)

}  // namespace f28
}  // namespace mdt
