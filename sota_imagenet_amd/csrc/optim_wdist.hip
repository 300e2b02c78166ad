// optim_wdist.hip — the device side of the WeightDistributionTB callback (the reference's sota_imagenet/callbacks.py:11-17: at every epoch's begin
// tb_logger.add_histogram("model/<name>", p.flatten(), step) for every entry of model.state_dict()) on flat fp32 arrays (gfx950).  add_histogram
// with its defaults copies the tensor to the host, widens it to double and runs np.histogram over TensorBoard's 1549 default edges — the 774
// values 1e-12 * 1.1^k below 1e20, their negatives and 0 — which sorts its input; it then takes min, max, sum and the sum of squares in double.
// Here that is one counting pass, tbbin_hist_kernel, one workgroup per work item { first element, length, tensor } (the table of optim_items.h at
// ANY element offset, walked with piece_walk as absbin_hist_kernel of optim_hist.hip walks it):
//   bins    the 774 positive edges lie in LDS as the doubles the host formed by the recurrence (no pow here: the table IS the rule).  c = the
//           number of edges <= |x| (x >= 0, -0.0 too) or < |x| (x < 0: the half-open side flips, e_k < |x| <= e_k+1), found by a binary search
//           of 10 steps on exact double comparisons; the bin is 774 + c or 773 - c.  c = 774 lies outside the table — except x equal to the
//           last edge, which np.histogram puts into the last bin — and is counted, like NaN, in the row's entry 1548: "in no bin".
//   counts  a workgroup histogram of 1548 bins + that entry in LDS, its non-zero entries then ADDED to hist[tensor][1552] with integer atomicAdd:
//           the workgroup histogram of hist_count.h, which says why a wave on ONE bin adds once.
//   stats   partial[item] = { min, max, sum, sum of squares, NaN seen } of the item's elements, in double.  A thread adds its elements in array
//           order, the lanes of a wave meet in a shuffle tree, the four waves are added in their order by thread 0: the same bits in every run.
//           min and max skip NaN (the caller makes them NaN where the flag is set, as numpy does); the sums take every element, so NaN and
//           infinities arrive in them as they do in numpy's.  The square of a float is exact in double.  No floating-point atomics.
// Elements outside the items (alignment gaps, the FC padding rows) are never read; a record that does not lie inside [0, n) is skipped by the
// whole workgroup before any barrier, and its partial[] entry stays as it was.
#include "common.h"
#include "hist_count.h"
#include "optim_items.h"

namespace mi355 {
namespace {

constexpr int kPos = 774;            // positive edges
constexpr int kBins = 2 * kPos;      // 1548
constexpr int kNoBin = kBins;        // the row's entry for values in no bin
constexpr int kRow = 1552;           // entries per row of hist[]: kBins + 1 padded to a multiple of 4
constexpr int kStats = 5;            // doubles per entry of partial[]
static_assert(kRow >= kBins + 1 && kRow % 4 == 0, "a row holds every bin and the no-bin entry and is a whole number of 16-byte vectors");

__device__ __forceinline__ int tbbin(float x, const double* __restrict__ pos) {
  if (x != x) return kNoBin;
  const unsigned bits = __float_as_uint(x);
  const bool neg = (bits >> 31) && (bits << 1);  // -0.0 counts as 0: it lies in [0, e_first)
  const double a = fabs((double)x);
  int c = 0;  // the number of edges <= a (x >= 0) or < a (x < 0): the edges ascend, so the ones that pass are a prefix of the table
#pragma unroll
  for (int s = 512; s > 0; s >>= 1) {  // 512 + ... + 1 = 1023 >= kPos: c collects the binary digits of the count from the top
    const int j = c + s;
    const double e = pos[min(j, kPos) - 1];
    if (j <= kPos && (neg ? e < a : e <= a)) c = j;
  }
  if (neg) return c < kPos ? kPos - 1 - c : kNoBin;
  if (c < kPos) return kPos + c;
  return a == pos[kPos - 1] ? kBins - 1 : kNoBin;  // the last bin is closed on the right
}

struct Stats {
  double mn, mx, sum, sq;
  int nan;
};

__device__ __forceinline__ void take(Stats& s, float x) {
  const double v = (double)x;
  s.sum += v;
  s.sq += v * v;
  if (x != x) {
    s.nan = 1;
  } else {
    s.mn = v < s.mn ? v : s.mn;
    s.mx = v > s.mx ? v : s.mx;
  }
}

__device__ __forceinline__ void meet(Stats& s, const Stats& o) {  // s: the lower lanes / waves, o: the higher ones
  s.mn = o.mn < s.mn ? o.mn : s.mn;
  s.mx = o.mx > s.mx ? o.mx : s.mx;
  s.sum += o.sum;
  s.sq += o.sq;
  s.nan |= o.nan;
}

__global__ __launch_bounds__(256) void tbbin_hist_kernel(const float* __restrict__ src, size_t n, const UnitPiece* __restrict__ items,
                                                         int n_tensors, const double* __restrict__ edges, unsigned* __restrict__ hist,
                                                         double* __restrict__ partial) {
  __shared__ double pos[kPos];
  __shared__ unsigned sh[kRow];
  __shared__ double wsum[4][4];
  __shared__ int wnan[4];
  const UnitPiece it = items[blockIdx.x];  // { off, len, tensor }: the layout of a work item
  if (!piece_ok(it, n, n_tensors)) return;  // the whole workgroup leaves: no barrier is passed by a part of it
  for (int i = threadIdx.x; i < kPos; i += 256) pos[i] = edges[i];
  for (int i = threadIdx.x; i < kRow; i += 256) sh[i] = 0u;
  __syncthreads();
  const float* __restrict__ sp = src + it.off;
  Stats st = {__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0};
  piece_walk<256>(
      it, (int)threadIdx.x,
      [&](int i) {
        const float x = sp[i];
        take(st, x);
        atomicAdd(&sh[tbbin(x, pos)], 1u);
      },
      [&](int head, int i) {
        const f32x4 v = reinterpret_cast<const f32x4*>(sp + head)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) take(st, v[k]);
        count_four(sh, tbbin(v[0], pos), tbbin(v[1], pos), tbbin(v[2], pos), tbbin(v[3], pos));
      });
  // the statistics: a shuffle tree over the wave (every lane takes part; a lane without elements holds the neutral values), then the waves in order
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    Stats o;
    o.mn = __shfl_down(st.mn, d), o.mx = __shfl_down(st.mx, d), o.sum = __shfl_down(st.sum, d), o.sq = __shfl_down(st.sq, d);
    o.nan = __shfl_down(st.nan, d);
    meet(st, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wsum[wave][0] = st.mn, wsum[wave][1] = st.mx, wsum[wave][2] = st.sum, wsum[wave][3] = st.sq;
    wnan[wave] = st.nan;
  }
  __syncthreads();  // also: every count of the workgroup is in sh[]
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      const Stats o = {wsum[w][0], wsum[w][1], wsum[w][2], wsum[w][3], wnan[w]};
      meet(st, o);
    }
    double* __restrict__ out = partial + (size_t)blockIdx.x * kStats;
    out[0] = st.mn, out[1] = st.mx, out[2] = st.sum, out[3] = st.sq, out[4] = st.nan ? 1.0 : 0.0;
  }
  flush_counts<kRow>(sh, hist + (size_t)it.slot * kRow);
}

}  // namespace

extern "C" int mi355_tbbin_hist(const float* src, size_t n, const void* items, size_t n_items, int n_tensors, const double* edges, int n_edges,
                                uint32_t* hist, double* partial, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(src && items && edges && hist && partial, "tbbin_hist: null pointer");
  MI355_ARG(aligned16(src) && aligned16(items) && aligned16(hist) && (uintptr_t)edges % 8 == 0 && (uintptr_t)partial % 8 == 0,
            "tbbin_hist: misaligned pointer (16 bytes for the array, the table and hist[], 8 for edges[] and partial[])");
  MI355_ARG(n_edges == kPos, "tbbin_hist: n_edges=%d, the table holds the %d positive edges", n_edges, kPos);
  MI355_ARG(n_items >= 1 && n_items <= kLwMaxGrid && n_tensors >= 1, "tbbin_hist: n_items=%zu, n_tensors=%d out of range", n_items, n_tensors);
  hipLaunchKernelGGL(tbbin_hist_kernel, dim3((unsigned)n_items), dim3(256), 0, st, src, n, (const UnitPiece*)items, n_tensors, edges, hist, partial);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
