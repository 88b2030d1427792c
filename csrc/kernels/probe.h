// Host entry points of the hardware probe kernels (probe.hip), shared with
// their torch wrappers (csrc/runtime/probes.cpp). Host-clean.
#pragma once
#include <hip/hip_runtime.h>

extern "C" {
int mdt_probe_clock(unsigned long long* out, int iters, hipStream_t s);
int mdt_probe_latency(const int* idx, int hops, unsigned long long* out, hipStream_t s);
int mdt_probe_empty(int blocks, int threads, hipStream_t s);
int mdt_probe_ramp(unsigned long long* out, int blocks, int threads, int lds, hipStream_t s);
int mdt_probe_lds_poison(unsigned pattern, int blocks, hipStream_t s);
int mdt_probe_cu_ids(unsigned* out, int blocks, hipStream_t s);
}
