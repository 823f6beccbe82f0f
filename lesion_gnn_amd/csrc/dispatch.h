// Runtime value -> template argument, at the launch site. Plain C++17, no HIP: a host compiler
// builds this header alone (tests/test_dispatch_host.py does).
#pragma once
#include <type_traits>
#include <utility>

// Calls f(std::integral_constant<V>) for the first V among Vs that equals v, and
// f(std::integral_constant<D>) when none does. f runs exactly once. The list is the call site's:
// only the constants named there are instantiated, so
//   one_of<0, 2, 8>(nck, [&](auto NC) { launch(k<NC>, ...); });
// builds k<0>, k<2> and k<8> and runs k<0> for every other nck. An argument that depends on
// another is derived inside the lambda (constexpr bool XIN = NL == 4;) or guarded with
// if constexpr, so that a site instantiates no more than its ladder did.
// v is compared as its own type T (each V is cast to T): pass one_of<false, true> a bool
// (flag != 0, p != nullptr), since an int 2 equals neither constant and would take the default.
template <auto D, auto... Vs, class T, class F>
inline void one_of(T v, F&& f) {
  const bool hit =
      ((v == static_cast<T>(Vs) ? (f(std::integral_constant<decltype(Vs), Vs>{}), true) : false) ||
       ...);
  if (!hit) f(std::integral_constant<decltype(D), D>{});
}
