// Thin torch wrappers over the hardware probe kernels (csrc/kernels/probe.hip).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "../kernels/probe.h"

namespace mdt {

void probe_clock(at::Tensor out, int64_t iters) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kInt64 && out.numel() >= 3, "out: cuda int64[3]");
  TORCH_CHECK(mdt_probe_clock(reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()), (int)iters,
                              c10::hip::getCurrentHIPStream().stream()) == 0, "probe_clock");
}

void probe_latency(at::Tensor idx, int64_t hops, at::Tensor out) {
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt32, "idx: cuda int32");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kInt64 && out.numel() >= 2, "out: cuda int64[2]");
  TORCH_CHECK(mdt_probe_latency(idx.data_ptr<int32_t>(), (int)hops,
                                reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()),
                                c10::hip::getCurrentHIPStream().stream()) == 0, "probe_latency");
}

void probe_empty(int64_t blocks, int64_t threads) {
  TORCH_CHECK(mdt_probe_empty((int)blocks, (int)threads, c10::hip::getCurrentHIPStream().stream()) == 0,
              "probe_empty");
}

// out: int64 [blocks][2] (entry tick, XCC / HW_ID bits) of an empty launch of `threads` threads and `lds` static
// LDS bytes per workgroup (0, 65536 or the fused 28x28 step's)
void probe_ramp(at::Tensor out, int64_t threads, int64_t lds) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kInt64 && out.is_contiguous() && out.dim() == 2 &&
                  out.size(1) == 2 && out.size(0) >= 1 && out.size(0) <= 65536,
              "out: contiguous cuda int64[blocks][2]");
  TORCH_CHECK(threads >= 1 && threads <= 512, "probe_ramp: threads");
  TORCH_CHECK(mdt_probe_ramp(reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()), (int)out.size(0),
                             (int)threads, (int)lds, c10::hip::getCurrentHIPStream().stream()) == 0,
              "probe_ramp: lds must be 0, 65536 or the step kernel's bytes");
}

void probe_lds_poison(int64_t pattern, int64_t blocks) {
  TORCH_CHECK(blocks > 0 && blocks <= 65536, "probe_lds_poison: blocks");
  TORCH_CHECK(mdt_probe_lds_poison((unsigned)pattern, (int)blocks, c10::hip::getCurrentHIPStream().stream()) == 0,
              "probe_lds_poison");
}

void probe_cu_ids(at::Tensor out) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kInt32 && out.numel() >= 1, "out: cuda int32[blocks]");
  TORCH_CHECK(mdt_probe_cu_ids(reinterpret_cast<unsigned*>(out.data_ptr<int32_t>()), (int)out.numel(),
                               c10::hip::getCurrentHIPStream().stream()) == 0, "probe_cu_ids");
}

}  // namespace mdt
