// weight_norm.hip — the reference's `src.callbacks.WeightNorm` (sota_imagenet/callbacks.py:104-123, "backward centered weight normalization";
// recipes 9, 10, 14, 37-39) over a flat fp32 parameter array (gfx950): after every optimizer step each conv filter and each FC row is centred
// on its mean and scaled to unit L2 norm, in place.  Per row x[0..L):
//   S1  = sum (double)x_i                      per thread in the order piece_sweep gives it its elements, then the fixed tree of optim_sum.h
//   m   = (float)(S1 / (double)L)
//   c_i = x_i - m                              float
//   S2  = sum (double)c_i * (double)c_i        the same order
//   nrm = (float)sqrt(S2)
//   x_i = c_i / nrm                            float division
// -ffp-contract=off: every operation is rounded on its own.  A constant row gives 0 / 0: the whole row becomes NaN, as in the reference.
//   item { int64 first; int32 row_len; int32 n_rows }   16 bytes: n_rows consecutive rows of one tensor, starting at element `first` — the
//                                                        RowRecord { off, len, count } of rows.h, tested by its rows_ok
// weight_norm_rows_kernel: ONE launch for the whole model, one 256-thread workgroup per item, which owns its rows from the first read to the
// last write.  Rows of at most kWaveRowMax elements take one wave each, four rows at a time (group_sum<64>); longer rows the whole workgroup
// (block_sum<256>).  A row is read three times — sum, centred sum of squares, write —, at most 18 KB for the longest row of ResNet-50 and at
// most 16 KB per round of four short rows: the second and third read find it in the CU's L1 / the XCD's L2, so HBM sees one read and one write.
// A row starts at any element offset (the stem's rows are 147 long): piece_sweep of optim_items.h, a scalar head up to the next 16-byte boundary,
// an f32x4 body, a scalar tail; each of the three passes is one element rule over rd(x), rd(x) and upd(x) (optim_sweep.h), called on the head
// element, the four lanes of every vector and the tail element.  No floating-point atomics and no sum across workgroups: a row's result
// depends on its elements alone, not on the item or the workgroup that took it, and two runs on the same input agree bit for bit.
// status[i]: 0 done;  2 the item does not fit the array — first >= 0, row_len >= 1, n_rows >= 1 and first + row_len*n_rows <= n are tested
// before anything is accessed through it —: nothing is read or written through it.  Elements outside the items are neither read nor written.
#include <cmath>

#include "common.h"
#include "optim_items.h"
#include "optim_sum.h"
#include "rows.h"

namespace mi355 {
namespace {

#ifndef MI355_WNORM_WAVE_ROW_MAX
#define MI355_WNORM_WAVE_ROW_MAX 1024  // 16 elements per lane and pass
#endif
constexpr int kWaveRowMax = MI355_WNORM_WAVE_ROW_MAX;
static_assert(kWaveRowMax >= 1, "rows up to this length take one wave");

template <int G>
__device__ __forceinline__ double row_sum(double x, double* sh) {
  if constexpr (G == 256)
    return block_sum<256>(x, sh);
  else
    return group_sum<G>(x, sh);
}

// one row over the G threads that share it (l: the thread's place among them); x: the row's first element, off its place in the array (for the
// alignment), L its length.  Every thread of the workgroup comes here with the same trip count (the sums hold barriers); a group without a row
// (active false) touches no memory.  sha and shb take turns: a thread that writes sha for the next sum has passed the barriers of the sum over
// shb, which every reader of sha's last result had reached.
template <int G>
__device__ __forceinline__ void norm_row(float* x, long long off, int L, int l, bool active, double* sha, double* shb) {
  const UnitPiece row = {off, L, 0};
  double s1 = 0.0;
  if (active) piece_sweep<G>(row, l, [&](float& v) { s1 += (double)v; }, rd(x));
  const float m = (float)(row_sum<G>(s1, sha) / (double)L);
  double s2 = 0.0;
  if (active)
    piece_sweep<G>(
        row, l,
        [&](float& v) {
          const float c = v - m;
          s2 += (double)c * (double)c;
        },
        rd(x));
  const float nrm = (float)sqrt(row_sum<G>(s2, shb));
  if (active) piece_sweep<G>(row, l, [&](float& v) { v = (v - m) / nrm; }, upd(x));
}

__global__ __launch_bounds__(256) void weight_norm_rows_kernel(float* w, size_t n, const RowRecord* __restrict__ items, int* __restrict__ status) {
  __shared__ double sha[256], shb[256];
  const RowRecord it = items[blockIdx.x];
  if (!rows_ok(it.off, it.len, it.count, n)) {  // (the same for every thread)
    if (threadIdx.x == 0) status[blockIdx.x] = 2;
    return;
  }
  const int t = threadIdx.x, L = it.len;
  if (L <= kWaveRowMax) {
    const int l = t & 63, wave = t >> 6;
    for (long long r0 = 0; r0 < it.count; r0 += 4) {  // (the same trip count for every thread)
      const long long r = r0 + wave;
      const bool active = r < it.count;
      const long long off = it.off + (active ? r * L : 0);
      norm_row<64>(w + off, off, L, l, active, sha, shb);
    }
  } else {
    for (long long r = 0; r < it.count; ++r) {
      const long long off = it.off + r * L;
      norm_row<256>(w + off, off, L, t, true, sha, shb);
    }
  }
  if (t == 0) status[blockIdx.x] = 0;
}

}  // namespace

extern "C" int mi355_wnorm_wave_row_max(void) { return kWaveRowMax; }

extern "C" int mi355_weight_norm_rows(float* w, size_t n, const void* items, size_t n_items, int* status, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(w && items && status, "weight_norm_rows: null pointer");
  MI355_ARG(aligned16(w) && aligned16(items) && (uintptr_t)status % 4 == 0,
            "weight_norm_rows: misaligned pointer (16 bytes for the array and the table, 4 for status[])");
  MI355_ARG(n >= 1 && n_items >= 1 && n_items <= kLwMaxGrid, "weight_norm_rows: n=%zu, n_items=%zu out of range", n, n_items);
  hipLaunchKernelGGL(weight_norm_rows_kernel, dim3((unsigned)n_items), dim3(256), 0, st, w, n, (const RowRecord*)items, status);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
