// optim_items.h — the tables that the kernels of optim_lw.hip, optim_adamp.hip, optim_sam.hip and optim_sam_lw.hip walk: the work items, and
// for the statistics taken per output unit the pieces, slots and tensor records; the test every kernel makes before it touches memory through a
// record; the walk of a run of elements that starts at any element offset, bare (piece_walk) and with one element rule (piece_sweep: the row
// kernels of weight_norm.hip and weight_std.hip); and the three loops that the unit-wise families share: the sums of a piece (piece_sums), the
// gather of a slot's partial sums (slot_gather) and the update of an item whose elements take a coefficient per slot (unit_item_sweep).
#pragma once
#include <cstddef>

#include <hip/hip_runtime.h>

#include "optim_sum.h"
#include "optim_sweep.h"

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

// piece_walk with the element rule stated once (optim_sweep.h): rule(float&...) gets one reference per array, the head element, then the four
// lanes of every vector in order, then the tail element.  The arrays, named by use (rd, upd, wr, ...), are already offset to the piece's first
// element; the rows of weight_norm.hip and weight_std.hip are walked this way.
template <int G, typename Rule, typename... A>
__device__ __forceinline__ void piece_sweep(const UnitPiece& pc, int l, Rule rule, const A&... a) {
  constexpr std::index_sequence_for<A...> js;
  piece_walk<G>(
      pc, l, [&](int i) { sweep_element(i, rule, js, a...); }, [&](int head, int i) { sweep_vector(i, rule, js, a.at(head)...); });
}

// K sums per piece, one group of G threads per piece, 256 / G pieces per workgroup: add(acc, x...) takes one element of every array of src, in
// the order piece_walk gives a thread its elements; each acc[j] then goes through group_sum, and the group's first thread writes
// partial[K*k .. K*k + K-1] of piece k.  Plain loads: what is summed here is read again by the update.  sh: one LDS array of 256 doubles per
// sum, which the kernel declares — as separate arrays where it can: a tree over a row of one two-dimensional array costs an address add a step.
template <int G, int K, typename Add, typename... P>
__device__ __forceinline__ void piece_sums(const UnitPiece* __restrict__ pieces, size_t n_pieces, size_t n, int n_slots,
                                           double* __restrict__ partial, double* const (&sh)[K], Add add, const P*... src) {
  const int l = threadIdx.x & (G - 1);
  const size_t k = (size_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  double acc[K] = {};
  if (k < n_pieces) {
    const UnitPiece pc = pieces[k];
    if (piece_ok(pc, n, n_slots)) {
      const auto walk = [&](const auto*... sp) {  // the arrays at the piece's first element
        piece_walk<G>(
            pc, l, [&](int i) { add(acc, sp[i]...); },
            [&](int head, int i) {
              [&](const auto&... v) {
#pragma unroll
                for (int j = 0; j < 4; ++j) add(acc, v[j]...);
              }(reinterpret_cast<const f32x4*>(sp + head)[i]...);
            });
      };
      walk((src + pc.off)...);
    }
  }
  double tot[K];
#pragma unroll
  for (int j = 0; j < K; ++j) tot[j] = group_sum<G>(acc[j], sh[j]);
  if (l == 0 && k < n_pieces) {
#pragma unroll
    for (int j = 0; j < K; ++j) partial[K * k + j] = tot[j];
  }
}

// a slot's entries lie inside partial[] (n_partial entries of K doubles each)
__device__ __forceinline__ bool slot_ok(const UnitSlot& sl, size_t n_partial) {
  return sl.first >= 0 && sl.count > 0 && (size_t)sl.first + (size_t)sl.count <= n_partial;
}

// thread l of G adds entries l, l + G, ... of the slot's K-wide partial sums into acc[]
template <int G, int K>
__device__ __forceinline__ void slot_gather(const UnitSlot& sl, const double* __restrict__ partial, int l, double (&acc)[K]) {
  for (int i = l; i < sl.count; i += G) {
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] += partial[K * ((size_t)sl.first + i) + j];
  }
}

// Where an item lies among the units of its tensor: the slot of an element is slot0 + (its offset inside the tensor) / unit_len.
struct UnitSpan {
  int e0;           // the item's first element inside its tensor
  int unit_len;
  int first, last;  // the units of its first and last element
  int slot0;        // slot of the tensor's unit 0; slot0 + last is inside the launch's slots
};

// false for a record through which the item would reach outside the launch's n_slots slots
__device__ __forceinline__ bool unit_span(const LwItem& it, const UnitTensor& t, int n_slots, UnitSpan& sp) {
  const long long e0 = it.off - t.start;
  if (t.unit_len <= 0 || t.slot0 < 0 || e0 < 0 || e0 + it.len > 0x7fffffffLL) return false;
  sp.e0 = (int)e0, sp.unit_len = t.unit_len, sp.slot0 = t.slot0;
  sp.first = sp.e0 / t.unit_len, sp.last = (sp.e0 + it.len - 1) / t.unit_len;
  return (long long)t.slot0 + sp.last < n_slots;
}

// item_sweep for an item whose elements take a coefficient per unit: coef_of(unit of the tensor) -> C, elem(const C&, float&...) with one
// reference per array; the array pointers are already offset to the item.  An item inside one unit — every item of a whole-tensor slot —
// takes its coefficient once and runs item_sweep.  Any other item sets (unit, place inside it) at the start of every vector and of a tail
// element and advances it element by element: an f32x4 can straddle two units or, with unit_len < 4, cover several.
template <typename CoefOf, typename Elem, typename... A>
__device__ __forceinline__ void unit_item_sweep(int len, const UnitSpan& sp, CoefOf coef_of, Elem elem, const A&... a) {
  if (sp.first == sp.last) {
    const auto c = coef_of(sp.first);
    item_sweep(len, [&](auto&... x) { elem(c, x...); }, a...);
    return;
  }
  const int u = sp.unit_len;
  int s = 0, r = 0;
  auto rule = [&](auto&... x) {
    elem(coef_of(s), x...);
    if (++r == u) r = 0, ++s;
  };
  const auto at = [&](int e) { s = (sp.e0 + e) / u, r = sp.e0 + e - s * u; };
  constexpr std::index_sequence_for<A...> js;
  const int n4 = len >> 2;
  for (int i = threadIdx.x; i < n4; i += 256) {
    at(4 * i);
    sweep_vector(i, rule, js, a...);
  }
  if ((int)threadIdx.x < (len & 3)) {
    at(4 * n4 + (int)threadIdx.x);
    sweep_element(4 * n4 + (int)threadIdx.x, rule, js, a...);
  }
}

}  // namespace mi355
