// spectral_norm.hip — the forward spectral normalisation of the plain ResNet-50 executor (gfx950): the reference's ForwardSpectralNorm callback
// (sota_imagenet/callbacks.py:87-101), which registers torch.nn.utils.parametrizations.spectral_norm (dim 0, one power iteration, eps 1e-12) on
// every Conv2d.  The parameters stay raw; the convolutions read w_hat = w / sigma, and the gradient wrt w_hat is turned into the gradient wrt w.
//   mat { RowRecord run; int64 u0; int64 v0 }   32 bytes: run.count rows of run.len contiguous elements from element run.off of the flat fp32
//                                                arrays (rows.h; any alignment: the stem's rows are 147 long); the matrix owns u[u0 .. u0 + rows),
//                                                v[v0 .. v0 + len) and sigma[its index].  u0 and v0 ascend with the index (the prefix sums of the
//                                                rows and of the row lengths): a row or a column finds its matrix by bisection.
// One power iteration of a matrix W [R, L], every operation rounded on its own (-ffp-contract=off), every sum in double:
//   t_r = sum_c W_rc * v_c                    one wave per row (piece_sweep; group_sum<64>)                               sn_wv_kernel
//   tau = sqrt(sum_r t_r^2);  u_r = (float)(t_r / max(tau, eps))       one workgroup per matrix (block_sum<256>)         sn_rows_finish_kernel
//   p_jc = sum_{r in slab j} W_rc * u_r       one thread per (slab, column), rows ascending; MI355_SN_SLABS slabs         sn_col_partials_kernel
//   s_c = sum_j p_jc (j ascending);  zeta = sqrt(sum_c s_c^2);  v_c = (float)(s_c / max(zeta, eps));
//   sigma = (float) sum_c s_c * v_c           one workgroup per matrix                                                    sn_cols_finish_kernel
// Eval (iters == 0): u, v untouched; sigma = (float) sum_r u_r * t_r (sn_rows_finish_kernel's other form).  Then w_hat_rc = W_rc / sigma, one wave
// per row (sn_divide_kernel); a zero matrix has sigma = 0 and becomes NaN, as in torch.
// Backward, u, v, sigma constants: q_r = sum_c g_rc * w_hat_rc (one wave per row, sn_gw_kernel); then every row's wave adds its matrix's q in
// index order, d = sum_r q_r, and writes dw_rc = (beta != 0 ? beta * dw_rc : 0) + (g_rc - ((float)d * u_r) * v_c) / sigma (sn_bwd_kernel).
// Every sum that crosses workgroups is taken by ONE owner, in index order, from values an earlier launch on the same stream left in the
// scratch: no floating-point atomics, no flags, no workgroup waits on another.  Two runs on the same input agree bit for bit.
// scratch (doubles): t[n_u], q[n_u], s[n_v], p[MI355_SN_SLABS][n_v] — mi355_spectral_scratch_doubles.
// A record that does not lie inside [0, n), [0, n_u), [0, n_v) is skipped before anything is accessed through it; elements outside the matrices
// are neither read nor written.  The division writes only what its lane has read: w_hat == w bakes sigma into the array.
#include <cmath>

#include "common.h"
#include "optim_items.h"
#include "optim_sum.h"
#include "rows.h"

namespace mi355 {
namespace {

struct SnDims {
  size_t n, n_u, n_v;
};

constexpr int kSlabs = MI355_SN_SLABS;

__host__ __device__ inline bool sn_span_ok(long long first, int count, size_t cap) {
  return first >= 0 && (size_t)first <= cap && (size_t)count <= cap - (size_t)first;
}
__host__ __device__ inline bool sn_mat_ok(const SpectralMat& q, const SnDims& d) {
  return rows_ok(q.run.off, q.run.len, q.run.count, d.n) && sn_span_ok(q.u0, q.run.count, d.n_u) && sn_span_ok(q.v0, q.run.len, d.n_v);
}

// the matrix that owns row k of u[] (BY_V: column k of v[]): the last record whose u0 (v0) is <= k, if it is a sound record that holds k
template <bool BY_V>
__device__ __forceinline__ bool sn_find(const SpectralMat* __restrict__ mats, int n_mats, const SnDims& d, long long k, SpectralMat& q, int& m) {
  int lo = 0, hi = n_mats;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((BY_V ? mats[mid].v0 : mats[mid].u0) <= k) lo = mid;
    else hi = mid;
  }
  q = mats[lo], m = lo;
  const long long k0 = BY_V ? q.v0 : q.u0;
  return sn_mat_ok(q, d) && k >= k0 && k - k0 < (BY_V ? q.run.len : q.run.count);
}

// the wave's row of the slice [row_begin, row_end) of u[]; a matrix takes part only if the slice holds all its rows (the backward sums over them).
// Every thread of the workgroup passes the same barriers (group_sum), a wave without a row touches no memory
__device__ __forceinline__ bool sn_take_row(const SpectralMat* __restrict__ mats, int n_mats, const SnDims& d, size_t row_begin, size_t row_end, size_t& k,
                                            SpectralMat& q, int& m, UnitPiece& pc) {
  k = row_begin + (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  pc = {0, 1, 0};
  if (k >= row_end || !sn_find<false>(mats, n_mats, d, (long long)k, q, m)) return false;
  if ((size_t)q.u0 < row_begin || (size_t)q.u0 + (size_t)q.run.count > row_end) return false;
  pc = {q.run.off + (long long)(k - (size_t)q.u0) * q.run.len, q.run.len, 0};
  return true;
}

__global__ __launch_bounds__(256) void sn_wv_kernel(const float* w, const float* __restrict__ v, double* __restrict__ t, SnDims d,
                                                    const SpectralMat* __restrict__ mats, int n_mats) {
  __shared__ double sh[256];
  const int l = threadIdx.x & 63;
  size_t k;
  SpectralMat q;
  int m;
  UnitPiece pc;
  const bool active = sn_take_row(mats, n_mats, d, 0, d.n_u, k, q, m, pc);
  double acc = 0.0;
  if (active) piece_sweep<64>(pc, l, [&](float& wi, float& vi) { acc += (double)wi * (double)vi; }, rd(w + pc.off), rd_any(v + q.v0));
  acc = group_sum<64>(acc, sh);
  if (active && l == 0) t[k] = acc;
}

// eval == 0: u = t / max(|t|, eps);  eval != 0: sigma = u . t, u untouched
__global__ __launch_bounds__(256) void sn_rows_finish_kernel(const double* __restrict__ t, float* __restrict__ u, float* __restrict__ sigma, SnDims d,
                                                             const SpectralMat* __restrict__ mats, int eval) {
  __shared__ double sh[256];
  const SpectralMat q = mats[blockIdx.x];
  const bool ok = sn_mat_ok(q, d);
  const int R = ok ? q.run.count : 0;
  double acc = 0.0;
  for (int r = threadIdx.x; r < R; r += 256) {
    const double tr = t[q.u0 + r];
    acc += eval ? (double)u[q.u0 + r] * tr : tr * tr;
  }
  const double tot = block_sum<256>(acc, sh);
  if (eval) {
    if (ok && threadIdx.x == 0) sigma[blockIdx.x] = (float)tot;
    return;
  }
  const double den = fmax(sqrt(tot), (double)MI355_SN_EPS);
  for (int r = threadIdx.x; r < R; r += 256) u[q.u0 + r] = (float)(t[q.u0 + r] / den);
}

// thread = column g of v[] in slab blockIdx.y of its matrix's rows: a wave reads 256 contiguous bytes of every row of the slab
__global__ __launch_bounds__(256) void sn_col_partials_kernel(const float* w, const float* __restrict__ u, double* __restrict__ p, SnDims d,
                                                              const SpectralMat* __restrict__ mats, int n_mats) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  SpectralMat q;
  int m;
  if (g >= d.n_v || !sn_find<true>(mats, n_mats, d, (long long)g, q, m)) return;
  const int R = q.run.count, per = (R + kSlabs - 1) / kSlabs;
  const int r0 = min(R, (int)blockIdx.y * per), r1 = min(R, r0 + per);
  const size_t L = (size_t)q.run.len;
  const float* col = w + q.run.off + (g - (size_t)q.v0);
  const float* ur = u + q.u0;
  double acc = 0.0;
#pragma unroll 4
  for (int r = r0; r < r1; ++r) acc += (double)col[(size_t)r * L] * (double)ur[r];
  p[(size_t)blockIdx.y * d.n_v + g] = acc;
}

__global__ __launch_bounds__(256) void sn_cols_finish_kernel(const double* __restrict__ p, double* __restrict__ s, float* __restrict__ v,
                                                             float* __restrict__ sigma, SnDims d, const SpectralMat* __restrict__ mats) {
  __shared__ double sha[256], shb[256];
  const SpectralMat q = mats[blockIdx.x];
  const bool ok = sn_mat_ok(q, d);
  const int L = ok ? q.run.len : 0;
  double acc = 0.0;
  for (int c = threadIdx.x; c < L; c += 256) {
    double sc = 0.0;
#pragma unroll
    for (int j = 0; j < kSlabs; ++j) sc += p[(size_t)j * d.n_v + (size_t)q.v0 + c];
    s[q.v0 + c] = sc;  // read back by this thread alone
    acc += sc * sc;
  }
  const double den = fmax(sqrt(block_sum<256>(acc, sha)), (double)MI355_SN_EPS);
  acc = 0.0;
  for (int c = threadIdx.x; c < L; c += 256) {
    const double sc = s[q.v0 + c];
    const float vc = (float)(sc / den);
    v[q.v0 + c] = vc;
    acc += sc * (double)vc;
  }
  const double tot = block_sum<256>(acc, shb);
  if (ok && threadIdx.x == 0) sigma[blockIdx.x] = (float)tot;
}

__global__ __launch_bounds__(256) void sn_divide_kernel(const float* w, float* w_hat, const float* __restrict__ sigma, SnDims d,
                                                        const SpectralMat* __restrict__ mats, int n_mats) {
  size_t k;
  SpectralMat q;
  int m;
  UnitPiece pc;
  if (!sn_take_row(mats, n_mats, d, 0, d.n_u, k, q, m, pc)) return;
  const float sg = sigma[m];
  piece_sweep<64>(pc, threadIdx.x & 63, [&](float& wi, float& yi) { yi = wi / sg; }, rd(w + pc.off), wr(w_hat + pc.off));
}

__global__ __launch_bounds__(256) void sn_gw_kernel(const float* __restrict__ g, const float* __restrict__ w_hat, double* __restrict__ qd, SnDims d,
                                                    const SpectralMat* __restrict__ mats, int n_mats, size_t row_begin, size_t row_end) {
  __shared__ double sh[256];
  const int l = threadIdx.x & 63;
  size_t k;
  SpectralMat q;
  int m;
  UnitPiece pc;
  const bool active = sn_take_row(mats, n_mats, d, row_begin, row_end, k, q, m, pc);
  double acc = 0.0;
  if (active) piece_sweep<64>(pc, l, [&](float& gi, float& wi) { acc += (double)gi * (double)wi; }, rd(g + pc.off), rd(w_hat + pc.off));
  acc = group_sum<64>(acc, sh);
  if (active && l == 0) qd[k] = acc;
}

__global__ __launch_bounds__(256) void sn_bwd_kernel(const float* __restrict__ g, const float* __restrict__ u, const float* __restrict__ v,
                                                     const float* __restrict__ sigma, float* __restrict__ dw, const double* __restrict__ qd, SnDims d,
                                                     const SpectralMat* __restrict__ mats, int n_mats, size_t row_begin, size_t row_end, float beta) {
  __shared__ double sh[256];
  const int l = threadIdx.x & 63;
  size_t k;
  SpectralMat q;
  int m;
  UnitPiece pc;
  const bool active = sn_take_row(mats, n_mats, d, row_begin, row_end, k, q, m, pc);
  double acc = 0.0;
  if (active)
    for (int r = l; r < q.run.count; r += 64) acc += qd[q.u0 + r];
  acc = group_sum<64>(acc, sh);  // every wave of the matrix: the same terms in the same order
  if (!active) return;
  const float du = (float)acc * u[k], sg = sigma[m];
  const bool acc_on = beta != 0.f;  // with beta == 0 nothing is loaded through dw, which may hold anything
  piece_sweep<64>(
      pc, l, [&](float& gi, float& vi, float& di) { di = (acc_on ? beta * di : 0.f) + (gi - du * vi) / sg; }, rd(g + pc.off), rd_any(v + q.v0),
      upd_when(dw + pc.off, acc_on));
}

bool sn_dims_ok(size_t n, size_t n_u, size_t n_v, size_t n_mats) {
  return n >= 1 && n_u >= 1 && n_v >= 1 && n_mats >= 1 && n_mats <= 65535 && n_u <= kLwMaxGrid && n_v <= kLwMaxGrid;
}
bool aligned4(const void* q) { return (uintptr_t)q % 4 == 0; }

}  // namespace

extern "C" size_t mi355_spectral_scratch_doubles(size_t n_u, size_t n_v) { return 2 * n_u + (size_t)(1 + kSlabs) * n_v; }

extern "C" int mi355_spectral_fwd(const float* w, float* w_hat, float* u, float* v, float* sigma, double* scratch, size_t n, size_t n_u, size_t n_v,
                                  const void* mats, size_t n_mats, int iters, void* stream) {
  MI355_ARG(w && u && v && sigma && scratch && mats, "spectral_fwd: null pointer (only w_hat may be null: no division)");
  MI355_ARG(aligned16(w) && aligned16(w_hat) && aligned16(mats) && aligned16(scratch) && aligned4(u) && aligned4(v) && aligned4(sigma),
            "spectral_fwd: misaligned pointer (16 bytes for the arrays, the table and the scratch, 4 for u[], v[] and sigma[])");
  MI355_ARG(sn_dims_ok(n, n_u, n_v, n_mats), "spectral_fwd: n=%zu, n_u=%zu, n_v=%zu, n_mats=%zu out of range", n, n_u, n_v, n_mats);
  MI355_ARG(iters >= 0 && iters <= MI355_SN_WARM_ITERS, "spectral_fwd: iters %d (0 eval .. %d)", iters, MI355_SN_WARM_ITERS);
  const SnDims d{n, n_u, n_v};
  const SpectralMat* mt = (const SpectralMat*)mats;
  const int nm = (int)n_mats;
  double *t = scratch, *s = scratch + 2 * n_u, *p = s + n_v;
  hipStream_t st = (hipStream_t)stream;
  const dim3 rows_grid((unsigned)((n_u + 3) / 4)), cols_grid((unsigned)((n_v + 255) / 256), kSlabs);
  for (int it = 0; it < (iters ? iters : 1); ++it) {
    hipLaunchKernelGGL(sn_wv_kernel, rows_grid, dim3(256), 0, st, w, v, t, d, mt, nm);
    hipLaunchKernelGGL(sn_rows_finish_kernel, dim3(nm), dim3(256), 0, st, t, u, sigma, d, mt, iters == 0 ? 1 : 0);
    if (iters == 0) break;
    hipLaunchKernelGGL(sn_col_partials_kernel, cols_grid, dim3(256), 0, st, w, u, p, d, mt, nm);
    hipLaunchKernelGGL(sn_cols_finish_kernel, dim3(nm), dim3(256), 0, st, p, s, v, sigma, d, mt);
  }
  if (w_hat) hipLaunchKernelGGL(sn_divide_kernel, rows_grid, dim3(256), 0, st, w, w_hat, sigma, d, mt, nm);
  MI355_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355_spectral_bwd(const float* g, const float* w_hat, const float* u, const float* v, const float* sigma, float* dw, double* scratch,
                                  size_t n, size_t n_u, size_t n_v, const void* mats, size_t n_mats, size_t row_begin, size_t row_end, float beta,
                                  void* stream) {
  MI355_ARG(g && w_hat && u && v && sigma && dw && scratch && mats, "spectral_bwd: null pointer");
  MI355_ARG(aligned16(g) && aligned16(w_hat) && aligned16(dw) && aligned16(mats) && aligned16(scratch) && aligned4(u) && aligned4(v) && aligned4(sigma),
            "spectral_bwd: misaligned pointer (16 bytes for the arrays, the table and the scratch, 4 for u[], v[] and sigma[])");
  MI355_ARG(g != dw && w_hat != dw, "spectral_bwd: dw must not be the array g or w_hat is read from");
  MI355_ARG(sn_dims_ok(n, n_u, n_v, n_mats), "spectral_bwd: n=%zu, n_u=%zu, n_v=%zu, n_mats=%zu out of range", n, n_u, n_v, n_mats);
  MI355_ARG(row_begin < row_end && row_end <= n_u, "spectral_bwd: rows [%zu, %zu) of u[%zu]", row_begin, row_end, n_u);
  const SnDims d{n, n_u, n_v};
  const SpectralMat* mt = (const SpectralMat*)mats;
  double* qd = scratch + n_u;
  const dim3 grid((unsigned)((row_end - row_begin + 3) / 4));
  hipLaunchKernelGGL(sn_gw_kernel, grid, dim3(256), 0, (hipStream_t)stream, g, w_hat, qd, d, mt, (int)n_mats, row_begin, row_end);
  hipLaunchKernelGGL(sn_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, g, u, v, sigma, dw, qd, d, mt, (int)n_mats, row_begin, row_end, beta);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
