// optim_sum.h — what the optimizer kernels of optim.hip and optim_lw.hip share: the fixed-order workgroup sum and the alignment test.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace mi355 {

// sum of one double per thread over the T threads of the workgroup, in a fixed order
template <int T>
__device__ __forceinline__ double block_sum(double x, double* sh) {
  sh[threadIdx.x] = x;
  __syncthreads();
#pragma unroll
  for (int w = T / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

inline bool aligned16(const void* q) { return (uintptr_t)q % 16 == 0; }

}  // namespace mi355
