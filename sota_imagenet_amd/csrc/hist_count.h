// hist_count.h — the workgroup histogram that the counting kernels of optim_hist.hip (absbin_hist_kernel) and optim_wdist.hip (tbbin_hist_kernel)
// share: a row of unsigned counts in LDS, zeroed by the kernel, filled with LDS atomics while the workgroup walks its work item (a scalar element
// is one atomicAdd of 1; a vector goes through count_four), then ADDED to the tensor's row in global memory (flush_counts).  Integer atomics only:
// the result is exact and the same bit for bit in every run.
//
// Same-address LDS atomics serialise, and the arrays counted here are the worst case for that: a trained network's values sit in a handful of
// bins, and an all-equal array — a BatchNorm weight at its initial value — in one (profiles/grad_dist.json: the all-equal array beside the
// ResNet-50 arrays).  So a thread first merges the equal neighbours among the four bins of its vector, and a wave whose active lanes all hold ONE
// bin adds its whole count once, from its first active lane.
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

// the bins b0..b3 of one thread's f32x4 counted into sh[].  Called from a loop whose trailing iterations leave lanes inactive: the wave-uniform
// test and the count it adds take the active lanes only.
__device__ __forceinline__ void count_four(unsigned* sh, int b0, int b1, int b2, int b3) {
  const int first = __builtin_amdgcn_readfirstlane(b0);
  if (__all((b0 == first) & (b1 == first) & (b2 == first) & (b3 == first))) {  // one bin in the whole wave: one add
    const unsigned long long act = __ballot(1);
    if ((int)__lane_id() == __ffsll((long long)act) - 1) atomicAdd(&sh[first], 4u * (unsigned)__popcll(act));
    return;
  }
  int cur = b0;
  unsigned c = 1u;
  const int rest[3] = {b1, b2, b3};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (rest[k] == cur) {
      ++c;
    } else {
      atomicAdd(&sh[cur], c);
      cur = rest[k], c = 1u;
    }
  }
  atomicAdd(&sh[cur], c);
}

// the non-zero entries of the workgroup's ROW counts added to the tensor's row, by the 256 threads of the workgroup after the barrier that ends
// the counting
template <int ROW>
__device__ __forceinline__ void flush_counts(const unsigned* sh, unsigned* __restrict__ row) {
  constexpr int kUnroll = ROW % 256 ? 1 : ROW / 256;  // a row of whole rounds is straight-line code, any other stays a loop
#pragma unroll kUnroll
  for (int i = threadIdx.x; i < ROW; i += 256) {
    const unsigned c = sh[i];
    if (c) atomicAdd(&row[i], c);
  }
}

}  // namespace mi355
