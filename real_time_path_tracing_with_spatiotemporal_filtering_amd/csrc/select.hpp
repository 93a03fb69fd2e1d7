// select.hpp — from a run-time value to a template argument.  A kernel family lists its instantiations ONCE, as a
// type_list of tag types; the prepare function visits every entry, the launch function the first entry that matches, and
// a run-time bool reaches a generic lambda as std::true_type / std::false_type, a three-valued mode as an integral_constant.
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
// f(std::integral_constant<int, mode>{}) for a mode of 0, 1 or 2 (anything else is 0): the three-valued template axes of the
// tracing kernels, whose modes scene_mode (closest_hit.hpp), tex_mode and spec_mode (shade_segment.hpp) compute
template <class F>
inline void with_mode3(int mode, F&& f) {
  if (mode == 2)
    f(std::integral_constant<int, 2>{});
  else if (mode == 1)
    f(std::integral_constant<int, 1>{});
  else
    f(std::integral_constant<int, 0>{});
}
// ... and for a mode of 0 to 3: shade_segment's material axis in the tile kernels, whose fourth value samples lights (spec_mode)
template <class F>
inline void with_mode4(int mode, F&& f) {
  if (mode == 3)
    f(std::integral_constant<int, 3>{});
  else
    with_mode3(mode, f);
}
// ... and of 0 to 4: the fifth value samples the analytic sphere light as well
template <class F>
inline void with_mode5(int mode, F&& f) {
  if (mode == 4)
    f(std::integral_constant<int, 4>{});
  else
    with_mode4(mode, f);
}
// ... and of 0 to 6: 5 and 6 are 3 and 4 with the weighted light pick
template <class F>
inline void with_mode7(int mode, F&& f) {
  if (mode == 5)
    f(std::integral_constant<int, 5>{});
  else if (mode == 6)
    f(std::integral_constant<int, 6>{});
  else
    with_mode5(mode, f);
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
