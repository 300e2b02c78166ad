// optim_items.h — the tables that the kernels of optim_lw.hip, optim_sam.hip and optim_sam_lw.hip walk: the work items, and for the statistics
// taken per output unit the pieces, slots and tensor records; the test every kernel makes before it touches memory through a record, and the walk
// over the elements of a piece.
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

// A slot is what one statistic is taken of: a whole tensor, or one output unit of it (one index of dim 0, a contiguous run of unit_len elements).
struct UnitPiece {
  long long off;  // first element, relative to the array pointers of the launch; any alignment
  int len;        // 1 .. kLwItemElems, inside one unit
  int slot;       // the unit's slot
};
struct UnitSlot {
  int first, count;  // the slot's consecutive entries of partial[]
};
struct UnitTensor {
  long long start;  // the tensor's first element, relative to the array pointers of the launch
  int unit_len;     // elements per slot: numel for a whole-tensor slot
  int slot0;        // slot of the tensor's first element
};
static_assert(sizeof(UnitPiece) == 16 && sizeof(UnitTensor) == 16 && sizeof(UnitSlot) == 8, "table records are 16 / 16 / 8 bytes");

__device__ __forceinline__ bool piece_ok(const UnitPiece& pc, size_t n, int n_slots) {
  return pc.off >= 0 && pc.len > 0 && pc.len <= kLwItemElems && (size_t)pc.off + (size_t)pc.len <= n && pc.slot >= 0 && pc.slot < n_slots;
}

// the elements of one piece over the G threads that share it (l: the thread's place among them).  A unit starts at any element offset, the arrays
// are 16-byte aligned, so off & 3 is the first element's place in its vector: a scalar head up to the next 16-byte boundary, an f32x4 body, a
// scalar tail.  one(i) takes element i of the piece, four(head, i) vector i behind the head; a thread sees its elements in array order.
template <int G, typename One, typename Four>
__device__ __forceinline__ void piece_walk(const UnitPiece& pc, int l, One one, Four four) {
  const int head = min((int)((4 - (pc.off & 3)) & 3), pc.len);
  const int n4 = (pc.len - head) >> 2, tail = (pc.len - head) & 3;
  if (l < head) one(l);
  for (int i = l; i < n4; i += G) four(head, i);
  if (l < tail) one(head + 4 * n4 + l);
}

}  // namespace mi355
