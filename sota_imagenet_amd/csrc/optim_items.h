// optim_items.h — the work-item table that the kernels of optim_lw.hip, optim_sam.hip and optim_sam_lw.hip walk: its record and the test every kernel makes before
// it touches memory through one.
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

namespace mi355 {

#ifndef MI355_LW_ITEM_ELEMS
#define MI355_LW_ITEM_ELEMS 4096  // 16 elements per thread: the ResNet-50 array is 6.3 k work items.  Other values: profiles/layerwise_step.json
#endif
constexpr int kLwItemElems = MI355_LW_ITEM_ELEMS;
static_assert(kLwItemElems >= 256 && kLwItemElems % 4 == 0, "an item is a whole number of float4, at least one per thread of a wave");

struct LwItem {
  long long off;  // first element, relative to the array pointers of the launch
  int len;        // 1 .. kLwItemElems
  int tensor;     // index into the per-tensor arrays of the launch (coef[], kind[])
};
static_assert(sizeof(LwItem) == 16, "table records are 16 bytes");

// a record that does not lie inside the arrays of the launch is skipped: the tables are checked by the host when they are built, this keeps a
// stale or foreign table from ever becoming an out-of-bounds access
__device__ __forceinline__ bool item_ok(const LwItem& it, size_t n, int n_tensors) {
  return it.off >= 0 && it.len > 0 && it.len <= kLwItemElems && (size_t)it.off + (size_t)it.len <= n && it.tensor >= 0 && it.tensor < n_tensors &&
         (it.off & 3) == 0;
}

constexpr size_t kLwMaxGrid = 1u << 30;

}  // namespace mi355
