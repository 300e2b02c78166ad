// init_ortho.hip — orthogonal initialisation (`src.callbacks.OrthoInitClb`, sota_imagenet/callbacks.py:250-266, i.e. torch.nn.init.orthogonal_;
// recipes 46-48, 50-53, 55) of the conv and FC weights of a flat fp32 parameter array (gfx950).  The host fills the matrices with N(0,1) draws;
// this file turns every one of them, in place, into the Q of its QR factorisation with a positive diagonal of R — which is what Gram-Schmidt
// produces, so no QR routine is needed: vector by vector in order, each loses its components along the earlier ones and is normalised.
//   record { int64 off; int32 rows; int32 chans; int32 taps; int32 pad },  cols = chans * taps,
//   logical element M[r][ci*taps + t] at w[off + r*cols + t*chans + ci]   (taps == 1: plain row-major; taps > 1: a conv weight in KRSC memory)
//   rows < cols:  the vectors are the rows, r = 0, 1, ...  (a row is one contiguous run; the order of the elements inside it plays no part)
//   otherwise:    the vectors are the columns in LOGICAL order c = ci*taps + t, which is not memory order when taps > 1
// ortho_init_kernel: ONE 1024-thread workgroup per matrix, the vector loop inside it; the matrices of a launch run side by side and no workgroup
// waits on another.  Per vector v (classical Gram-Schmidt, every vector projected TWICE — one projection leaves an orthogonality defect of
// eps * cond(M)):
//   n0 = |v|;   twice { h_j = <q_j, v> for the earlier vectors j;  v = v - sum_j h_j q_j };   n2 = |v|;   v = v / n2
// The earlier vectors are taken 1024 at a time (their h_j sit in LDS), so for more than 1024 vectors a projection is classical inside a chunk and
// modified from chunk to chunk.  Arithmetic: the fp32 elements are converted to double, every dot product, every sum_j and the subtraction are
// double (one rounding per operation, -ffp-contract=off), and v is rounded to fp32 once per projection and once when it is normalised; the last
// pass stores fl(q * gain), one float multiply (gain == 1: q itself).  No floating-point atomics; every sum across threads goes through the fixed
// trees of optim_sum.h, every other sum is one thread's loop in index order: two runs on the same input agree bit for bit.
//   rows case  dots: one wave per earlier row, lanes along the row (group_sum<64>);  update: one thread per element, the earlier rows in order
//   tall case  dots: one thread per earlier column, down the rows (v staged in LDS), lanes across the columns (contiguous along a row);  update: 16 lanes per row
//              across the columns (group_sum<16>), 64 rows per round
// status[i]: 0 done;  1 a vector's residual n2 was zero, non-finite or below 2^-12 * n0 (rank-deficient input): that vector is zeroed, the ones
// before it are orthonormal (gain not applied), the ones behind it keep their input;  2 the record does not fit the array (off + rows*cols <= n,
// rows, chans, taps >= 1): nothing is accessed through it.  Every loop bound comes from a record that passed that test.
#include <cmath>

#include "common.h"
#include "optim_sum.h"

namespace mi355 {
namespace {

constexpr int kT = 1024;      // threads of the workgroup that owns one matrix
constexpr int kChunk = 1024;  // earlier vectors per projection chunk: their coefficients h[] in LDS
static_assert(kChunk == kT, "the tall case keeps one coefficient per thread");

struct OrthoMat {
  long long off;  // first element in the flat array
  int rows, chans, taps, pad;
};
static_assert(sizeof(OrthoMat) == 24, "records are 24 bytes");

__device__ __forceinline__ bool mat_ok(const OrthoMat& m, size_t n) {
  if (m.off < 0 || m.rows < 1 || m.chans < 1 || m.taps < 1) return false;
  const size_t cols = (size_t)m.chans * (size_t)m.taps;  // < 2^62
  if (cols > n || (size_t)m.rows > n / cols) return false;
  return (size_t)m.off <= n - (size_t)m.rows * cols;
}

// what both orientations do with the two norms of a vector: false for a residual that cannot be normalised
__device__ __forceinline__ bool residual_ok(double n0sq, double n2sq, double& inv) {
  const double r0 = sqrt(n0sq), r2 = sqrt(n2sq);
  inv = 1.0 / r2;
  return r2 > 0.0 && isfinite(r2) && !(r2 < r0 * (1.0 / 4096.0));
}

// rows < cols: the vectors are the nv rows of L contiguous elements
__device__ int ortho_rows(float* a, int nv, size_t L, double* sh, double* h) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int k = 0; k < nv; ++k) {
    float* v = a + (size_t)k * L;
    const auto norm_sq = [&]() {
      double s = 0.0;
      for (size_t e = t; e < L; e += kT) {
        const double x = (double)v[e];
        s += x * x;
      }
      const double r = block_sum<kT>(s, sh);
      __syncthreads();  // sh is reused
      return r;
    };
    const double n0sq = norm_sq();
    for (int pass = 0; pass < 2; ++pass)
      for (int j0 = 0; j0 < k; j0 += kChunk) {
        const int cnt = min(kChunk, k - j0);
        const float* q0 = a + (size_t)j0 * L;
        for (int jj = 0; jj < cnt; jj += kT / 64) {  // (the same trip count for every thread: group_sum holds barriers)
          const int j = jj + wave;
          double p = 0.0;
          if (j < cnt) {
            const float* q = q0 + (size_t)j * L;
#pragma unroll 8
            for (size_t e = lane; e < L; e += 64) p += (double)q[e] * (double)v[e];
          }
          const double d = group_sum<64>(p, sh);
          if (j < cnt && lane == 0) h[j] = d;
          __syncthreads();  // sh is reused; after the last round h[] is complete
        }
        for (size_t e = t; e < L; e += kT) {
          double acc = 0.0;
#pragma unroll 8
          for (int j = 0; j < cnt; ++j) acc += h[j] * (double)q0[(size_t)j * L + e];
          v[e] = (float)((double)v[e] - acc);
        }
        __syncthreads();  // v is read by every wave, h[] is rewritten
      }
    const double n2sq = norm_sq();
    double inv;
    const bool ok = residual_ok(n0sq, n2sq, inv);  // (the same for every thread)
    for (size_t e = t; e < L; e += kT) v[e] = ok ? (float)((double)v[e] * inv) : 0.f;
    if (!ok) return 1;
    __syncthreads();
  }
  return 0;
}

// rows >= cols: the vectors are the columns, L = rows elements each, in logical order; memory column mm holds logical column
// (mm % chans)*taps + mm / chans
__device__ int ortho_cols(float* a, int L, int chans, int taps, double* sh, double* h, float* vs) {
  const int t = threadIdx.x, l16 = t & 15, rr = t >> 4;
  const int cols = chans * taps;  // <= rows
  for (int k = 0; k < cols; ++k) {
    const int mk = taps == 1 ? k : (k % taps) * chans + k / taps;
    float* v = a + mk;                       // element r at v[r*cols]
    const int mend = taps == 1 ? k : cols;   // the memory columns that can hold an earlier vector
    const auto norm_sq = [&]() {
      double s = 0.0;
      for (long long r = t; r < L; r += kT) {
        const double x = (double)v[(size_t)r * cols];
        s += x * x;
      }
      const double r = block_sum<kT>(s, sh);
      __syncthreads();
      return r;
    };
    const double n0sq = norm_sq();
    for (int pass = 0; pass < 2; ++pass)
      for (int m0 = 0; m0 < mend; m0 += kChunk) {
        const int cnt = min(kChunk, mend - m0);
        {
          const int mm = m0 + t;
          const bool earlier = t < cnt && (taps == 1 ? mm : (mm % chans) * taps + mm / chans) < k;
          double d = 0.0;  // stays exactly 0 for a column that holds no earlier vector: the update skips it
          for (long long r0 = 0; r0 < L; r0 += kT) {  // v goes through LDS, kT rows at a time (the same trip count for every thread)
            const int nr = (int)min((long long)kT, L - r0);
            if (t < nr) vs[t] = v[(size_t)(r0 + t) * cols];
            __syncthreads();
            if (earlier) {
              const float* q = a + (size_t)r0 * cols + mm;
#pragma unroll 16
              for (int r = 0; r < nr; ++r) d += (double)q[(size_t)r * cols] * (double)vs[r];
            }
            __syncthreads();
          }
          h[t] = d;
        }
        __syncthreads();
        for (long long r0 = 0; r0 < L; r0 += kT / 16) {  // (the same trip count for every thread)
          const long long r = r0 + rr;
          double p = 0.0;
          if (r < L) {
            const float* q = a + (size_t)r * cols + m0;
#pragma unroll 8
            for (int c = l16; c < cnt; c += 16) {
              const double hc = h[c], x = (double)q[c];
              p += hc != 0.0 ? hc * x : 0.0;  // (a select, not a branch: the loads of a round are in flight together)
            }
          }
          const double tot = group_sum<16>(p, sh);
          if (r < L && l16 == 0) v[(size_t)r * cols] = (float)((double)v[(size_t)r * cols] - tot);
          __syncthreads();  // sh is reused; after the last round v is complete and h[] may be rewritten
        }
      }
    const double n2sq = norm_sq();
    double inv;
    const bool ok = residual_ok(n0sq, n2sq, inv);
    for (long long r = t; r < L; r += kT) v[(size_t)r * cols] = ok ? (float)((double)v[(size_t)r * cols] * inv) : 0.f;
    if (!ok) return 1;
    __syncthreads();
  }
  return 0;
}

__global__ __launch_bounds__(kT) void ortho_init_kernel(float* w, size_t n, const OrthoMat* __restrict__ mats, float gain, int* __restrict__ status) {
  __shared__ double sh[kT];
  __shared__ double h[kChunk];
  __shared__ float vs[kT];  // the tall case: the current vector, kT elements at a time
  const OrthoMat m = mats[blockIdx.x];
  if (!mat_ok(m, n)) {  // (the same for every thread)
    if (threadIdx.x == 0) status[blockIdx.x] = 2;
    return;
  }
  float* a = w + m.off;
  const size_t cols = (size_t)m.chans * (size_t)m.taps;
  const int st = (size_t)m.rows < cols ? ortho_rows(a, m.rows, cols, sh, h) : ortho_cols(a, m.rows, m.chans, m.taps, sh, h, vs);
  if (st == 0 && gain != 1.f) {  // (both functions end on a barrier when they return 0)
    const size_t len = (size_t)m.rows * cols;
    for (size_t e = threadIdx.x; e < len; e += kT) a[e] = a[e] * gain;
  }
  if (threadIdx.x == 0) status[blockIdx.x] = st;
}

}  // namespace

extern "C" int mi355_ortho_init(float* w, size_t n, const void* mats, size_t n_mats, float gain, int* status, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  MI355_ARG(w && mats && status, "ortho_init: null pointer");
  MI355_ARG((uintptr_t)w % 4 == 0 && (uintptr_t)mats % 8 == 0 && (uintptr_t)status % 4 == 0,
            "ortho_init: misaligned pointer (8 bytes for the records, 4 for the array and status[])");
  MI355_ARG(n >= 1 && n_mats >= 1 && n_mats <= (1u << 20), "ortho_init: n=%zu, n_mats=%zu out of range", n, n_mats);
  MI355_ARG(std::isfinite(gain), "ortho_init: gain=%g is not finite", (double)gain);
  hipLaunchKernelGGL(ortho_init_kernel, dim3((unsigned)n_mats), dim3(kT), 0, st, w, n, (const OrthoMat*)mats, gain, status);
  MI355_LAUNCH_CHECK();
  return 0;
}

}  // namespace mi355
