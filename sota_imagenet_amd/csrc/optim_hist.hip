// optim_hist.hip — the device side of the GradDistributionTB callback (the reference's sota_imagenet/callbacks.py:30-60) on flat fp32 arrays
// (gfx950).  Every log_every-th step the reference sorts |x| of every parameter, exp_avg and exp_avg_sq tensor, keeps every subsample-th value of
// each sort, sorts the concatenation, keeps every subsample-th value again and hands log10 of the rest to a histogram.  The sorts are not needed:
// the kept ranks 0, s, 2s, ... of a sorted tensor include exactly ceil(c / s) values below a threshold, c the number of its elements below it, and
// the same holds for the second round — so the bin counts of the twice-subsampled set follow exactly from per-tensor bin counts (DESIGN.md
// section 17).  Two kernels, integer arithmetic only (no floating-point atomics: the result is exact and the same bit for bit in every run):
//   absbin_hist_kernel, one workgroup per work item { first element, length, tensor } (the table of optim_items.h, at ANY element offset: a
//     state of the layer-wise optimizers is one element per tensor): bin (absbin.h) of every element of the item — a scalar head up to the next
//     16-byte boundary, an f32x4 body, a scalar tail (piece_walk) — counted in a 512-entry histogram in LDS, then the non-zero bins ADDED to
//     hist[tensor][512] with integer atomicAdd: the workgroup histogram of hist_count.h, which says why a wave on ONE bin adds once.  Elements
//     outside the items (alignment gaps, the FC padding rows) are never read into a count; a record that does not lie inside [0, n) is skipped.
//   subsample_counts_kernel, one workgroup of 512 threads: c_t(k) = rep[t] * (elements of tensor t in bins below k), C(k) = sum_t ceil(c_t(k) / s),
//     counts[k] = ceil(C(k+1) / s) - ceil(C(k) / s), all in 64 bits.  A wave takes every eighth tensor, a lane eight consecutive bins: the prefix
//     inside the lane, a shuffle scan over the lanes' totals; the eight waves' sums meet in LDS.  rep[t] counts a state that is stored once and
//     shown broadcast (exp_avg_sq of the layer-wise optimizers).  rep is device memory, so rep[t] < 1 cannot fail the call before the launch
//     without a read-back: the kernel then writes ~0 into every counts[k], which no count can be.
#include "absbin.h"
#include "common.h"
#include "hist_count.h"
#include "optim_items.h"

namespace mi355 {
namespace {

constexpr int kNB = kAbsBinBins;

__device__ __forceinline__ int absbin(float x) { return absbin_of_bits(__float_as_uint(x)); }

__global__ __launch_bounds__(256) void absbin_hist_kernel(const float* __restrict__ src, size_t n, const UnitPiece* __restrict__ items,
                                                          int n_tensors, unsigned* __restrict__ hist) {
  __shared__ unsigned sh[kNB];
  const UnitPiece it = items[blockIdx.x];  // { off, len, tensor }: the layout of a work item
  if (!piece_ok(it, n, n_tensors)) return;  // the whole workgroup leaves: no barrier is passed by a part of it
  sh[threadIdx.x] = 0u;
  sh[threadIdx.x + 256] = 0u;
  __syncthreads();
  const float* __restrict__ sp = src + it.off;
  piece_walk<256>(
      it, (int)threadIdx.x, [&](int i) { atomicAdd(&sh[absbin(sp[i])], 1u); },
      [&](int head, int i) {
        const f32x4 v = reinterpret_cast<const f32x4*>(sp + head)[i];
        count_four(sh, absbin(v[0]), absbin(v[1]), absbin(v[2]), absbin(v[3]));
      });
  __syncthreads();
  flush_counts<kNB>(sh, hist + (size_t)it.slot * kNB);
}

__device__ __forceinline__ unsigned long long ceil_div(unsigned long long a, unsigned long long s) { return a / s + (a % s != 0); }

__global__ __launch_bounds__(kNB) void subsample_counts_kernel(const unsigned* __restrict__ hist, const int* __restrict__ rep, int n_tensors,
                                                                unsigned long long s, unsigned long long* __restrict__ counts) {
  constexpr int kWaves = kNB / 64;
  __shared__ unsigned long long sh[kWaves][kNB + 1];
  __shared__ int bad;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  unsigned long long acc[8] = {}, acc_end = 0;  // this wave's part of C(8*lane + j), and of C(512) (lane 63)
  for (int t = wave; t < n_tensors; t += kWaves) {
    const int r = rep[t];
    if (r < 1) {
      bad = 1;  // every writer writes the same value
      continue;
    }
    const uint4* row = reinterpret_cast<const uint4*>(hist + (size_t)t * kNB + 8 * lane);
    const uint4 a = row[0], b = row[1];
    const unsigned h[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned long long tot = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) tot += h[j];
    unsigned long long incl = tot;  // inclusive scan of the lanes' totals
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    unsigned long long below = incl - tot;  // elements of the tensor in bins below 8*lane
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[j] += ceil_div(below * (unsigned long long)r, s);
      below += h[j];
    }
    if (lane == 63) acc_end += ceil_div(below * (unsigned long long)r, s);
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sh[wave][8 * lane + j] = acc[j];
  if (lane == 63) sh[wave][kNB] = acc_end;
  __syncthreads();
  const int k = threadIdx.x;
  unsigned long long lo = 0, hi = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) lo += sh[w][k], hi += sh[w][k + 1];
  counts[k] = bad ? ~0ull : ceil_div(hi, s) - ceil_div(lo, s);
}

}  // namespace

extern "C" int mi355_absbin_hist(const float* src, size_t n, const void* items, size_t n_items, int n_tensors, uint32_t* hist, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(src && items && hist, "absbin_hist: null pointer");
  MI355_ARG(aligned16(src) && aligned16(items) && aligned16(hist), "absbin_hist: misaligned pointer (16 bytes for the array, the table and hist[])");
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1, "absbin_hist: n_items=%zu, n_tensors=%d out of range", n_items, n_tensors);
  hipLaunchKernelGGL(absbin_hist_kernel, dim3((unsigned)n_items), dim3(256), 0, st, src, n, (const UnitPiece*)items, n_tensors, hist);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_subsample_counts(const uint32_t* hist, const int32_t* rep, int n_tensors, int subsample, uint64_t* counts, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(hist && rep && counts, "subsample_counts: null pointer");
  MI355_ARG(aligned16(hist) && (uintptr_t)rep % 4 == 0 && (uintptr_t)counts % 8 == 0,
            "subsample_counts: misaligned pointer (16 bytes for hist[], 4 for rep[], 8 for counts[])");
  MI355_ARG(n_tensors >= 1 && subsample >= 1, "subsample_counts: n_tensors=%d, subsample=%d must be >= 1", n_tensors, subsample);
  hipLaunchKernelGGL(subsample_counts_kernel, dim3(1), dim3(kNB), 0, st, hist, rep, n_tensors, (unsigned long long)subsample,
                     (unsigned long long*)counts);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
