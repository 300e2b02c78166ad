// rows.h — the 16-byte record of the row tables (csrc/weight_norm.hip, csrc/weight_std.hip and the executor that builds the latter's table), the
// test a kernel makes before it touches memory through one, and the matrix record csrc/spectral_norm.hip builds on it.  Plain C++ for host and device.
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

namespace mi355 {

struct RowRecord {
  long long off;  // first element of the first row in the flat arrays; any alignment
  int len;        // elements per row
  int count;      // consecutive rows (weight_norm's n_rows); weight_std's tables hold one row per record and their kernels do not read it
};
static_assert(sizeof(RowRecord) == 16, "table records are 16 bytes");

// `count` rows of `len` elements from element `off` lie inside [0, n)
__host__ __device__ inline bool rows_ok(long long off, int len, int count, size_t n) {
  if (off < 0 || len < 1 || count < 1) return false;
  const size_t total = (size_t)len * (size_t)count;  // < 2^62
  return total <= n && (size_t)off <= n - total;
}

// a matrix of the spectral normalisation (csrc/spectral_norm.hip and the executor that builds its table): a run of rows and its places in the
// vectors of the power iteration
struct SpectralMat {
  RowRecord run;  // count = R rows of len = L elements
  long long u0;   // the matrix owns u[u0 .. u0 + R)
  long long v0;   // and v[v0 .. v0 + L); u0 and v0 ascend with the index in the table
};
static_assert(sizeof(SpectralMat) == 32, "matrix records are 32 bytes");

}  // namespace mi355
