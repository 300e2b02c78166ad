// dispatch.h — runtime value -> template argument, written once for the host-side launchers (host only; each returns the callback's status).
//   with_elem(dtype, who, f)          f(Elem<float>{}) / f(Elem<bf16_t>{}); any other code: "<who>: bad dtype <n>", MI355_E_ARG, f not called
//   with_bool(b, f)                   f(std::true_type{}) / f(std::false_type{})
//   with_int<V0, V1, ..>(v, who, f)   f(std::integral_constant<int, Vi>{}) for the Vi equal to v; MI355_E_ARG when none is
// The callbacks declare `-> int` (MI355_ARG / MI355_LAUNCH_CHECK return enumerators, `return 0` an int).  A constant names its template
// argument where it is bound — with_bool(residual != nullptr, [&](auto RES) -> int { ... kernel<T, RES> ... }) —, the element type is
// `using T = typename decltype(e)::type`, the vector width Vec16<T>::N.  Every combination a nest of these calls can reach is instantiated:
// a launcher dispatches only over the axes that vary at that point.
#pragma once
#include <type_traits>

#include "common.h"

namespace mi355 {

template <typename T>
struct Elem { using type = T; };

template <typename F>
int with_elem(int dtype, const char* who, F&& f) {
  if (dtype == MI355_F32) return f(Elem<float>{});
  if (dtype == MI355_BF16) return f(Elem<bf16_t>{});
  set_error("%s: bad dtype %d", who, dtype);
  return MI355_E_ARG;
}

template <typename F>
int with_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

template <int... Vs, typename F>
int with_int(int v, const char* who, F&& f) {
  int rc = MI355_E_ARG;
  const bool hit = (... || (v == Vs && (rc = f(std::integral_constant<int, Vs>{}), true)));  // the first Vi equal to v, in the order given
  if (!hit) set_error("%s: value %d outside the dispatched set", who, v);
  return rc;
}

}  // namespace mi355
