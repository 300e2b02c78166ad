// weight_std.hip — the per-filter weight transform of the plain ResNet-50 executor (gfx950): the reference's `weight_standardization: True`
// (train.py:66-67, conv_to_ws_conv) and its ForwardWeightNorm callback (sota_imagenet/callbacks.py:62-84, zero_mean_conv_weight) over rows of a
// flat fp32 array.  The parameters stay raw; the convolutions read w_hat, and the gradient wrt w_hat is turned into the gradient wrt w.
//   row { int64 off; int32 len; int32 reserved }   16 bytes: one output filter, len = K*K*Cin contiguous elements from element `off` (any
//                                                   alignment: the stem's rows are 147 long); row k of the table owns invstd[k].  The RowRecord
//                                                   of rows.h, tested by its rows_ok as one row; the third field is not read
// Forward, per row w[0..L) — the arithmetic of weight_std_fwd_kernel (variant.hip), every operation rounded on its own (-ffp-contract=off):
//   S1 = sum (double)w_i,  S2 = sum (double)w_i * (double)w_i     per lane in the order piece_sweep gives it its elements, then the fixed tree
//                                                                  of group_sum<64>; no floating-point atomics, nothing summed across waves
//   mu = S1 / L,  var = max(S2 / L - mu * mu, 0)                  double
//   is = (float)(1 / sqrt(var + eps))   mode 1 (standardise);     is = 1   mode 2 (centre)            (MI355_WS_STANDARDISE, MI355_WS_CENTRE)
//   w_hat_i = (w_i - (float)mu) * is                              float;   invstd[k] = is
// A constant row has var = 0 (or a rounding's worth): is <= 1 / sqrt(eps) is finite and the row becomes zeros (or values of the order of the
// rounding of its mean), never NaN.
// Backward, per row, from g = the gradient wrt w_hat — the arithmetic of weight_std_bwd_kernel:
//   m1 = (float)(sum (double)g_i / L);   m2 = (float)(sum (double)g_i * (double)w_hat_i / L)   mode 1;   m2 = 0   mode 2
//   v_i = is * (g_i - m1 - w_hat_i * m2)   mode 1;   v_i = is * (g_i - m1)   mode 2 (is = invstd[k], which the forward left at 1)
//   dw_i = (beta != 0 ? beta * dw_i : 0) + v_i
// One wave per row, four rows per 256-thread workgroup, ONE launch per table (forward) or per slice [row_begin, row_end) of it (backward).  A
// wave owns its row from the first read to the last write and every lane writes only elements it has read itself, so the forward may write
// where it reads (w_hat == w: the transform baked into the parameters).  A row is read twice — sums, then the write —, at most 18 KB: the second
// read finds it in the CU's L1 / the XCD's L2.  Two runs on the same input agree bit for bit.  A record that does not lie inside [0, n) — off >= 0,
// len >= 1, off + len <= n are tested before anything is accessed through it — is skipped: nothing is read or written through it, invstd[k]
// included.  Elements outside the rows are neither read nor written.
// Each of the four passes is one element rule under piece_sweep (optim_items.h) over arrays named by use (optim_sweep.h): the forward's sums
// read rd(w) and its write is rd(w), wr(w_hat); the backward's sums read rd(g), rd_when(w_hat, standardise) and its write adds
// upd_when(dw, beta != 0) — in centre mode nothing is loaded through w_hat, with beta == 0 nothing through dw, which may hold anything.
#include <cmath>

#include "common.h"
#include "optim_items.h"
#include "optim_sum.h"
#include "rows.h"

namespace mi355 {
namespace {

// the wave's row of the slice: every thread of the workgroup passes the same barriers (group_sum), a wave without a row touches no memory
__device__ __forceinline__ bool ws_take_row(const RowRecord* __restrict__ rows, size_t row_begin, size_t row_end, size_t n, size_t& k, UnitPiece& pc) {
  k = row_begin + (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  pc = {0, 1, 0};
  if (k >= row_end) return false;
  const RowRecord q = rows[k];
  if (!rows_ok(q.off, q.len, 1, n)) return false;  // (one row per record: q.count is not read)
  pc = {q.off, q.len, 0};
  return true;
}

__global__ __launch_bounds__(256) void weight_std_rows_fwd_kernel(const float* w, float* w_hat, float* __restrict__ invstd, size_t n,
                                                                  const RowRecord* __restrict__ rows, size_t n_rows, int mode, float eps) {
  __shared__ double sha[256], shb[256];
  const int l = threadIdx.x & 63;
  size_t k;
  UnitPiece pc;
  const bool active = ws_take_row(rows, 0, n_rows, n, k, pc);
  const float* x = w + pc.off;
  float* y = w_hat + pc.off;
  double s1 = 0.0, s2 = 0.0;
  if (active)
    piece_sweep<64>(
        pc, l,
        [&](float& xi) {
          const double v = (double)xi;
          s1 += v, s2 += v * v;
        },
        rd(x));
  s1 = group_sum<64>(s1, sha);
  s2 = group_sum<64>(s2, shb);
  if (!active) return;
  const double L = (double)pc.len, mu = s1 / L, var = fmax(s2 / L - mu * mu, 0.0);
  const float m = (float)mu, is = mode == MI355_WS_STANDARDISE ? (float)(1.0 / sqrt(var + (double)eps)) : 1.f;
  if (l == 0) invstd[k] = is;
  piece_sweep<64>(pc, l, [&](float& xi, float& yi) { yi = (xi - m) * is; }, rd(x), wr(y));
}

__global__ __launch_bounds__(256) void weight_std_rows_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w_hat,
                                                                  const float* __restrict__ invstd, float* __restrict__ dw, size_t n,
                                                                  const RowRecord* __restrict__ rows, size_t row_begin, size_t row_end, int mode,
                                                                  float beta) {
  __shared__ double sha[256], shb[256];
  const int l = threadIdx.x & 63;
  size_t k;
  UnitPiece pc;
  const bool active = ws_take_row(rows, row_begin, row_end, n, k, pc);
  const float* gr = g + pc.off;
  const float* wh = w_hat + pc.off;
  float* d = dw + pc.off;
  const bool std_mode = mode == MI355_WS_STANDARDISE, acc = beta != 0.f;  // w_hat is read in standardise mode only, dw only to be accumulated into
  double a = 0.0, b = 0.0;
  if (active)
    piece_sweep<64>(
        pc, l,
        [&](float& gi, float& wi) {
          a += (double)gi;
          if (std_mode) b += (double)gi * (double)wi;
        },
        rd(gr), rd_when(wh, std_mode));
  a = group_sum<64>(a, sha);
  b = group_sum<64>(b, shb);
  if (!active) return;
  const double L = (double)pc.len;
  const float m1 = (float)(a / L), m2 = (float)(b / L), is = invstd[k];
  piece_sweep<64>(
      pc, l,
      [&](float& gi, float& wi, float& di) {
        const float v = std_mode ? is * (gi - m1 - wi * m2) : is * (gi - m1);
        di = (acc ? beta * di : 0.f) + v;
      },
      rd(gr), rd_when(wh, std_mode), upd_when(d, acc));
}

bool ws_mode_ok(int mode) { return mode == MI355_WS_STANDARDISE || mode == MI355_WS_CENTRE; }

}  // namespace

extern "C" int mi355_weight_std_rows_fwd(const float* w, float* w_hat, float* invstd, size_t n, const void* rows, size_t n_rows, int mode, float eps,
                                         void* stream) {
  MI355_ARG(w && w_hat && invstd && rows, "weight_std_rows_fwd: null pointer");
  MI355_ARG(aligned16(w) && aligned16(w_hat) && aligned16(rows) && (uintptr_t)invstd % 4 == 0,
            "weight_std_rows_fwd: misaligned pointer (16 bytes for the arrays and the table, 4 for invstd[])");
  MI355_ARG(ws_mode_ok(mode), "weight_std_rows_fwd: mode %d (1 standardise, 2 centre)", mode);
  MI355_ARG(n >= 1 && n_rows >= 1 && n_rows <= kLwMaxGrid && eps >= 0.f, "weight_std_rows_fwd: n=%zu, n_rows=%zu, eps=%g out of range", n, n_rows, (double)eps);
  hipLaunchKernelGGL(weight_std_rows_fwd_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, w, w_hat, invstd, n,
                     (const RowRecord*)rows, n_rows, mode, eps);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_weight_std_rows_bwd(const float* g, const float* w_hat, const float* invstd, float* dw, size_t n, const void* rows, size_t row_begin,
                                         size_t row_end, int mode, float beta, void* stream) {
  MI355_ARG(g && w_hat && invstd && dw && rows, "weight_std_rows_bwd: null pointer");
  MI355_ARG(aligned16(g) && aligned16(w_hat) && aligned16(dw) && aligned16(rows) && (uintptr_t)invstd % 4 == 0,
            "weight_std_rows_bwd: misaligned pointer (16 bytes for the arrays and the table, 4 for invstd[])");
  MI355_ARG(g != dw && w_hat != dw, "weight_std_rows_bwd: dw must not be the array g or w_hat is read from");
  MI355_ARG(ws_mode_ok(mode), "weight_std_rows_bwd: mode %d (1 standardise, 2 centre)", mode);
  MI355_ARG(n >= 1 && row_begin < row_end && row_end - row_begin <= kLwMaxGrid, "weight_std_rows_bwd: n=%zu, rows [%zu, %zu) out of range", n, row_begin,
            row_end);
  hipLaunchKernelGGL(weight_std_rows_bwd_kernel, dim3((unsigned)((row_end - row_begin + 3) / 4)), dim3(256), 0, (hipStream_t)stream, g, w_hat, invstd,
                     dw, n, (const RowRecord*)rows, row_begin, row_end, mode, beta);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
