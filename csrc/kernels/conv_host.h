// Host-side helpers shared by the op builders (conv_igemm.hip, conv_thin.hip,
// conv_bf16.hip) and the planners (conv_plan.hip). Host-clean: no device code.
#pragma once
#include <string.h>

#include "conv_igemm.h"

namespace mdt {

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// The argument struct of a job into its (zero-padded) blob.
template <class T>
void put_args(JobBlob* j, const T& a) {
  static_assert(sizeof(T) <= kJobArgBytes, "job arguments exceed the blob");
  memset(j->args, 0, sizeof(j->args));
  memcpy(j->args, &a, sizeof(T));
}

// One job of `nblk` workgroups: every field of `j` is written.
template <class T>
int record_job(JobBlob* j, int kind, int nblk, const T& a) {
  memset(j, 0, sizeof(*j));
  j->kind = kind;
  j->nblk = nblk;
  put_args(j, a);
  return 0;
}

}  // namespace mdt
