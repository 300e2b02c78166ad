// optim_sweep.h — the loop every element-wise optimizer kernel runs over flat fp32 arrays, stated once: an f32x4 body and a scalar tail for the
// n % 4 elements behind it, both calling the same element rule.  A kernel names its arrays in load order, each with how it is used:
//   rd(q)    read                                  (const float*)
//   last(q)  read for the last time in the step: the vector load is non-temporal, the lines are not kept in L2 / Infinity Cache   (const float*)
//   upd(q)   read, and written back after the rule (float*); an array the rule overwrites without reading it costs no load
//   upd_if<ON>(q)  upd(q) where ON; an array that is not there otherwise (the moving average of a step without one): nothing is loaded or
//            stored through q and the rule gets a zero, so a kernel names the array once and only its element rule asks whether it exists
//   wr(q)    written after the rule, never read: the rule gets a zero   (float*)
//   rd_when(q, on)   rd(q) where the run-time flag `on` holds; otherwise nothing is loaded through q and the rule gets a zero   (const float*)
//   upd_when(q, on)  upd(q) where `on` holds, wr(q) otherwise: an accumulation beta * old + new whose beta may be zero, old then being anything
//   rd_any(q)        read, q at any 4-byte phase against the sweep's vectors: scalar loads   (const float*)
// rule(float&...) gets one reference per array, in the same order; it is called four times per vector and once per tail element, so a reduction
// that adds into a captured variable sees a thread's elements in array order.  Stores cover the upd() and wr() arrays only.  The arrays must not
// overlap, except that a wr() array may be an rd() array of the same sweep: a thread has read its elements of every array before it writes any.
// a.at(e) is the same kind of array e elements further on (piece_sweep of optim_items.h: the vectors behind a scalar head).
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"

namespace mi355 {

template <typename T, bool NONTEMPORAL, bool ON = true, bool LOAD = ON>
struct SweepArray {
  T* q;
  static constexpr bool kStore = ON && !std::is_const<T>::value;
  __device__ __forceinline__ SweepArray at(int e) const { return {q + e}; }
  template <typename I>
  __device__ __forceinline__ f32x4 load4(I i) const {
    if constexpr (!LOAD) return f32x4{0.f, 0.f, 0.f, 0.f};
    else if constexpr (NONTEMPORAL) return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(q) + i);
    else return reinterpret_cast<const f32x4*>(q)[i];
  }
  template <typename I>
  __device__ __forceinline__ float load1(I i) const {
    if constexpr (LOAD) return q[i];
    else return 0.f;
  }
  template <typename I>
  __device__ __forceinline__ void store4(I i, const f32x4& x) const {
    if constexpr (kStore) reinterpret_cast<f32x4*>(q)[i] = x;
  }
  template <typename I>
  __device__ __forceinline__ void store1(I i, float x) const {
    if constexpr (kStore) q[i] = x;
  }
};

__device__ __forceinline__ SweepArray<const float, false> rd(const float* q) { return {q}; }
__device__ __forceinline__ SweepArray<const float, true> last(const float* q) { return {q}; }
__device__ __forceinline__ SweepArray<float, false> upd(float* q) { return {q}; }
template <bool ON>
__device__ __forceinline__ SweepArray<float, false, ON> upd_if(float* q) { return {q}; }
__device__ __forceinline__ SweepArray<float, false, true, false> wr(float* q) { return {q}; }

// rd(q) / upd(q) whose load is decided at run time (the same for every element of the sweep)
template <typename T>
struct SweepArrayWhen {
  T* q;
  bool on;
  __device__ __forceinline__ SweepArrayWhen at(int e) const { return {q + e, on}; }
  template <typename I>
  __device__ __forceinline__ f32x4 load4(I i) const {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (on) v = reinterpret_cast<const f32x4*>(q)[i];
    return v;
  }
  template <typename I>
  __device__ __forceinline__ float load1(I i) const {
    return on ? q[i] : 0.f;
  }
  template <typename I>
  __device__ __forceinline__ void store4(I i, const f32x4& x) const {
    if constexpr (!std::is_const<T>::value) reinterpret_cast<f32x4*>(q)[i] = x;
  }
  template <typename I>
  __device__ __forceinline__ void store1(I i, float x) const {
    if constexpr (!std::is_const<T>::value) q[i] = x;
  }
};

__device__ __forceinline__ SweepArrayWhen<const float> rd_when(const float* q, bool on) { return {q, on}; }
__device__ __forceinline__ SweepArrayWhen<float> upd_when(float* q, bool on) { return {q, on}; }

// rd(q) of an array that does not share the sweep's 16-byte phase (the vector v next to a matrix row that starts at any element: spectral_norm.hip):
// four scalar loads per vector, nothing stored
struct SweepArrayAny {
  const float* q;
  __device__ __forceinline__ SweepArrayAny at(int e) const { return {q + e}; }
  template <typename I>
  __device__ __forceinline__ f32x4 load4(I i) const {
    const float* p = q + 4 * (size_t)i;
    return f32x4{p[0], p[1], p[2], p[3]};
  }
  template <typename I>
  __device__ __forceinline__ float load1(I i) const {
    return q[i];
  }
  template <typename I>
  __device__ __forceinline__ void store4(I, const f32x4&) const {}
  template <typename I>
  __device__ __forceinline__ void store1(I, float) const {}
};

__device__ __forceinline__ SweepArrayAny rd_any(const float* q) { return {q}; }

// vector i of every array
template <typename I, typename Rule, size_t... J, typename... A>
__device__ __forceinline__ void sweep_vector(I i, Rule& rule, std::index_sequence<J...>, const A&... a) {
  f32x4 v[] = {a.load4(i)...};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float x[] = {v[J][k]...};
    rule(x[J]...);
    ((v[J][k] = x[J]), ...);
  }
  (a.store4(i, v[J]), ...);
}

// element i of every array
template <typename I, typename Rule, size_t... J, typename... A>
__device__ __forceinline__ void sweep_element(I i, Rule& rule, std::index_sequence<J...>, const A&... a) {
  float x[] = {a.load1(i)...};
  rule(x[J]...);
  (a.store1(i, x[J]), ...);
}

// grid-stride form over arrays of n = 4 * n4 + (n & 3) elements: workgroup 0's first n & 3 threads take the tail
template <typename Rule, typename... A>
__device__ __forceinline__ void flat_sweep(size_t n4, size_t n, Rule rule, const A&... a) {
  constexpr std::index_sequence_for<A...> js;
  // blockDim.x, read as the kernels themselves read it: spelled blockDim.x in a device function it also allows for a partial last workgroup,
  // which no launch has, and costs every wave a dependent global load before its first vector
  const size_t threads = __builtin_amdgcn_workgroup_size_x();
  for (size_t i = blockIdx.x * threads + threadIdx.x; i < n4; i += gridDim.x * threads) sweep_vector(i, rule, js, a...);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) sweep_element(n4 * 4 + threadIdx.x, rule, js, a...);
}

// one workgroup of 256 threads per work item of len elements (optim_items.h); the array pointers are already offset to the item
template <typename Rule, typename... A>
__device__ __forceinline__ void item_sweep(int len, Rule rule, const A&... a) {
  constexpr std::index_sequence_for<A...> js;
  const int n4 = len >> 2;
  for (int i = threadIdx.x; i < n4; i += 256) sweep_vector(i, rule, js, a...);
  if ((int)threadIdx.x < (len & 3)) sweep_element(n4 * 4 + (int)threadIdx.x, rule, js, a...);
}

}  // namespace mi355
