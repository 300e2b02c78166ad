// optim_sum.h — what the optimizer kernels of optim.hip, optim_lw.hip, optim_adamp.hip, optim_sam.hip and optim_sam_lw.hip share: the
// fixed-order workgroup and group sums (block_sum; group_sum, which piece_sums of optim_items.h and the per-slot coefficient kernels call) and
// the alignment test.
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

// sum of one double per thread over each group of G consecutive threads of the 256-thread workgroup, in a fixed order
template <int G>
__device__ __forceinline__ double group_sum(double x, double* sh) {
  const int t = threadIdx.x, l = t & (G - 1);
  sh[t] = x;
  __syncthreads();
#pragma unroll
  for (int w = G / 2; w > 0; w >>= 1) {
    if (l < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  return sh[t - l];
}

inline bool aligned16(const void* q) { return (uintptr_t)q % 16 == 0; }

}  // namespace mi355
