// weight_std.hip — the per-filter weight transform of the plain ResNet-50 executor (gfx950): the reference's `weight_standardization: True`
// (train.py:66-67, conv_to_ws_conv) and its ForwardWeightNorm callback (sota_imagenet/callbacks.py:62-84, zero_mean_conv_weight) over rows of a
// flat fp32 array.  The parameters stay raw; the convolutions read w_hat, and the gradient wrt w_hat is turned into the gradient wrt w.
//   row { int64 off; int32 len; int32 reserved }   16 bytes: one output filter, len = K*K*Cin contiguous elements from element `off` (any
//                                                   alignment: the stem's rows are 147 long); row k of the table owns invstd[k]
// Forward, per row w[0..L) — the arithmetic of weight_std_fwd_kernel (variant.hip), every operation rounded on its own (-ffp-contract=off):
//   S1 = sum (double)w_i,  S2 = sum (double)w_i * (double)w_i     per lane in the order piece_walk gives it its elements, then the fixed tree
//                                                                  of group_sum<64>; no floating-point atomics, nothing summed across waves
//   mu = S1 / L,  var = max(S2 / L - mu * mu, 0)                  double
//   is = (float)(1 / sqrt(var + eps))   mode 1 (standardise);     is = 1   mode 2 (centre)
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
#include <cmath>

#include "common.h"
#include "optim_items.h"
#include "optim_sum.h"

namespace mi355 {
namespace {

struct WsRow {
  long long off;  // first element of the row in the flat arrays; any alignment
  int len;        // elements of the row
  int reserved;
};
static_assert(sizeof(WsRow) == 16, "table records are 16 bytes");

__device__ __forceinline__ bool ws_row_ok(const WsRow& r, size_t n) { return r.off >= 0 && r.len >= 1 && (size_t)r.len <= n && (size_t)r.off <= n - (size_t)r.len; }

// the wave's row of the slice: every thread of the workgroup passes the same barriers (group_sum), a wave without a row touches no memory
__device__ __forceinline__ bool ws_take_row(const WsRow* __restrict__ rows, size_t row_begin, size_t row_end, size_t n, size_t& k, WsRow& r) {
  k = row_begin + (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  r = {0, 1, 0};
  if (k >= row_end) return false;
  const WsRow q = rows[k];
  if (!ws_row_ok(q, n)) return false;
  r = q;
  return true;
}

__global__ __launch_bounds__(256) void weight_std_rows_fwd_kernel(const float* w, float* w_hat, float* __restrict__ invstd, size_t n,
                                                                  const WsRow* __restrict__ rows, size_t n_rows, int mode, float eps) {
  __shared__ double sha[256], shb[256];
  const int l = threadIdx.x & 63;
  size_t k;
  WsRow r;
  const bool active = ws_take_row(rows, 0, n_rows, n, k, r);
  const UnitPiece pc = {r.off, r.len, 0};
  const float* x = w + r.off;
  float* y = w_hat + r.off;
  double s1 = 0.0, s2 = 0.0;
  if (active)
    piece_walk<64>(
        pc, l,
        [&](int i) {
          const double v = (double)x[i];
          s1 += v, s2 += v * v;
        },
        [&](int head, int i) {
          const f32x4 v = reinterpret_cast<const f32x4*>(x + head)[i];
#pragma unroll
          for (int j = 0; j < 4; ++j) s1 += (double)v[j], s2 += (double)v[j] * (double)v[j];
        });
  s1 = group_sum<64>(s1, sha);
  s2 = group_sum<64>(s2, shb);
  if (!active) return;
  const double L = (double)r.len, mu = s1 / L, var = fmax(s2 / L - mu * mu, 0.0);
  const float m = (float)mu, is = mode == 1 ? (float)(1.0 / sqrt(var + (double)eps)) : 1.f;
  if (l == 0) invstd[k] = is;
  piece_walk<64>(
      pc, l, [&](int i) { y[i] = (x[i] - m) * is; },
      [&](int head, int i) {
        f32x4 v = reinterpret_cast<const f32x4*>(x + head)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (v[j] - m) * is;
        reinterpret_cast<f32x4*>(y + head)[i] = v;
      });
}

__global__ __launch_bounds__(256) void weight_std_rows_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w_hat,
                                                                  const float* __restrict__ invstd, float* __restrict__ dw, size_t n,
                                                                  const WsRow* __restrict__ rows, size_t row_begin, size_t row_end, int mode,
                                                                  float beta) {
  __shared__ double sha[256], shb[256];
  const int l = threadIdx.x & 63;
  size_t k;
  WsRow r;
  const bool active = ws_take_row(rows, row_begin, row_end, n, k, r);
  const UnitPiece pc = {r.off, r.len, 0};
  const float* gr = g + r.off;
  const float* wh = w_hat + r.off;
  float* d = dw + r.off;
  const bool std_mode = mode == 1;
  double a = 0.0, b = 0.0;
  if (active)
    piece_walk<64>(
        pc, l,
        [&](int i) {
          a += (double)gr[i];
          if (std_mode) b += (double)gr[i] * (double)wh[i];
        },
        [&](int head, int i) {
          const f32x4 v = reinterpret_cast<const f32x4*>(gr + head)[i];
#pragma unroll
          for (int j = 0; j < 4; ++j) a += (double)v[j];
          if (std_mode) {
            const f32x4 u = reinterpret_cast<const f32x4*>(wh + head)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) b += (double)v[j] * (double)u[j];
          }
        });
  a = group_sum<64>(a, sha);
  b = group_sum<64>(b, shb);
  if (!active) return;
  const double L = (double)r.len;
  const float m1 = (float)(a / L), m2 = (float)(b / L), is = invstd[k];
  const auto rule = [&](float gi, float wi, float old) {
    const float v = std_mode ? is * (gi - m1 - wi * m2) : is * (gi - m1);
    return (beta != 0.f ? beta * old : 0.f) + v;
  };
  piece_walk<64>(
      pc, l, [&](int i) { d[i] = rule(gr[i], std_mode ? wh[i] : 0.f, beta != 0.f ? d[i] : 0.f); },
      [&](int head, int i) {
        const f32x4 v = reinterpret_cast<const f32x4*>(gr + head)[i];
        f32x4 u = {0.f, 0.f, 0.f, 0.f}, o = {0.f, 0.f, 0.f, 0.f};
        if (std_mode) u = reinterpret_cast<const f32x4*>(wh + head)[i];
        if (beta != 0.f) o = reinterpret_cast<const f32x4*>(d + head)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = rule(v[j], u[j], o[j]);
        reinterpret_cast<f32x4*>(d + head)[i] = o;
      });
}

bool ws_mode_ok(int mode) { return mode == 1 || mode == 2; }

}  // namespace

extern "C" int mi355_weight_std_rows_fwd(const float* w, float* w_hat, float* invstd, size_t n, const void* rows, size_t n_rows, int mode, float eps,
                                         void* stream) {
  MI355_ARG(w && w_hat && invstd && rows, "weight_std_rows_fwd: null pointer");
  MI355_ARG(aligned16(w) && aligned16(w_hat) && aligned16(rows) && (uintptr_t)invstd % 4 == 0,
            "weight_std_rows_fwd: misaligned pointer (16 bytes for the arrays and the table, 4 for invstd[])");
  MI355_ARG(ws_mode_ok(mode), "weight_std_rows_fwd: mode %d (1 standardise, 2 centre)", mode);
  MI355_ARG(n >= 1 && n_rows >= 1 && n_rows <= kLwMaxGrid && eps >= 0.f, "weight_std_rows_fwd: n=%zu, n_rows=%zu, eps=%g out of range", n, n_rows, (double)eps);
  hipLaunchKernelGGL(weight_std_rows_fwd_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, w, w_hat, invstd, n,
                     (const WsRow*)rows, n_rows, mode, eps);
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
                     dw, n, (const WsRow*)rows, row_begin, row_end, mode, beta);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
