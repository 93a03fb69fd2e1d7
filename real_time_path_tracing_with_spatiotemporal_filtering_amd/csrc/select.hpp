// select.hpp — from a run-time value to a template argument.  A kernel family lists its instantiations ONCE, as a
// type_list of tag types; the prepare function visits every entry, the launch function the first entry that matches, and
// a run-time bool reaches a generic lambda as std::true_type / std::false_type, a mode of N values as an integral_constant (with_mode<N>).
#pragma once

#include <type_traits>

namespace rt {
namespace {

template <class... E>
struct type_list {};

// f(E{}) for every entry, in order
template <class... E, class F>
inline void visit_all(type_list<E...>, F&& f) {
  (f(E{}), ...);
}
// f(E{}) in order until one returns true (the entry matched and f launched it); false: no entry matched
template <class... E, class F>
inline bool visit_first(type_list<E...>, F&& f) {
  return (f(E{}) || ...);
}

// f(std::true_type{}) or f(std::false_type{}); read the constant back with decltype(tag)::value
template <class F>
inline void with_bool(bool b, F&& f) {
  if (b)
    f(std::true_type{});
  else
    f(std::false_type{});
}
// f(std::integral_constant<int, mode>{}) for a mode in [0, N) (anything else is 0): the many-valued template axes of the tracing
// kernels — with_mode<3> for scene_mode (closest_hit.hpp), tex_mode and the queue kernels' spec_mode (shade_segment.hpp),
// with_mode<kSpecModes> for the tile kernels' SPEC (kernels.hpp)
template <int N, class F>
inline void with_mode(int mode, F&& f) {
  if constexpr (N > 1) {
    if (mode == N - 1)
      f(std::integral_constant<int, N - 1>{});
    else
      with_mode<N - 1>(mode, f);
  } else {
    f(std::integral_constant<int, 0>{});
  }
}
// f(FINAL, EXACT): the two bools every filter kernel is instantiated over
template <class F>
inline void with_final_exact(bool final_pass, bool exact, F&& f) {
  with_bool(final_pass, [&](auto fin) { with_bool(exact, [&](auto ex) { f(fin, ex); }); });
}
// all four of them (prepare functions)
template <class F>
inline void each_final_exact(F&& f) {
  for (int i = 0; i < 4; i++) with_final_exact(i & 1, i & 2, f);
}

}  // namespace
}  // namespace rt
