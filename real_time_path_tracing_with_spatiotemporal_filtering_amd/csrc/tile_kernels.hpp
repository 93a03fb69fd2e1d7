// tile_kernels.hpp — the four K2 tile kernels over pathtrace_tile.hpp's body, stated once for the translation units that instantiate
// them: kernels.hip (every instantiation without an EnvView, and everything that shares a launch with K0, K1 or K3) and
// kernels_env.hip (the instantiations of the ENV axis, kernels.hpp).  The templates live in an anonymous namespace, so each unit
// emits its own instantiations and no name is defined twice.
#pragma once

#include "pathtrace_tile.hpp"

namespace rt {
namespace {

// The four tile kernels.  LV: the light list of an instantiation that samples lights, as a trailing parameter pack that is empty
// for every other one or holds spec_lights_t<SPEC> (kernels.hpp): a LightView, or a LightTableView where the pick is weighted.
// The list travels as a parameter of its own, and of those instantiations only, so that the argument segments of the kernels
// that take none — the kernels of a build that samples no light — stay what they were.
template <int BVH, bool COMPACT, bool DEMOD, int TEX, int SPEC, class... LV>
__global__ __launch_bounds__(kPtThreads)
__attribute__((amdgpu_waves_per_eu(kPtBvhWaves, kPtBvhWaves)))
void k_pathtrace(PathtraceArgs a, TexView tex, LV... lights) {
  static_assert(pack_takes<SPEC, LV...>(), "the light argument SPEC asks for, then a NormalView or nothing");
  pathtrace_tile<BVH, COMPACT, false, DEMOD, TEX, SPEC>(a, tex, 0, 0, 0, lights...);
}
template <bool COMPACT, bool DEMOD, int TEX, int SPEC, class... LV>
__global__ __launch_bounds__(kPtThreads)
__attribute__((amdgpu_waves_per_eu(kPtWaves, kPtWaves)))
void k_pathtrace_small(PathtraceArgs a, TexView tex, LV... lights) {
  static_assert(pack_takes<SPEC, LV...>(), "the light argument SPEC asks for, then a NormalView or nothing");
  pathtrace_tile<0, COMPACT, false, DEMOD, TEX, SPEC>(a, tex, 0, 0, 0, lights...);
}

// K0 + K1 + K2 in one launch (rtpt_gbuffer / rtpt_temporal_gradient recorded right before rtpt_raytrace: main.cpp:1105-1107
// is that order; compacting variants only, the default policy).  Workgroups are dispatched in the order of their linear
// index: rows [0, a.tiles_y) of the grid are the tracing tiles — long ones first, pathtrace_tile — and the rows behind them
// the G-buffer's 64 x 4 tiles, a few microseconds each, which therefore start while the last tracing tiles drain: the
// G-buffer's work fills the tail of the trace instead of having a launch, a ramp and a tail of its own.  Nothing in the
// trace reads what the G-buffer writes except the depth in the traced image's alpha, and that the G-buffer workgroups
// store themselves (gbuffer_pixel) while the tracing ones store the colour's 12 bytes — disjoint bytes, any order.
template <int BVH, bool DEMOD, int TEX, int SPEC, class... LV>
__global__ __launch_bounds__(kPtThreads)
__attribute__((amdgpu_waves_per_eu(kPtBvhWaves, kPtBvhWaves)))
void k_gbuffer_pathtrace(PathtraceArgs a, GbufferArgs g, TexView tex, LV... lights) {
  static_assert(pack_takes<SPEC, LV...>(), "the light argument SPEC asks for, then a NormalView or nothing");
  gbuffer_pathtrace_body<BVH, DEMOD, TEX, SPEC>(a, g, tex, lights...);
}
template <bool DEMOD, int TEX, int SPEC, class... LV>
__global__ __launch_bounds__(kPtThreads)
__attribute__((amdgpu_waves_per_eu(kPtWaves, kPtWaves)))
void k_gbuffer_pathtrace_small(PathtraceArgs a, GbufferArgs g, TexView tex, LV... lights) {
  static_assert(pack_takes<SPEC, LV...>(), "the light argument SPEC asks for, then a NormalView or nothing");
  gbuffer_pathtrace_body<0, DEMOD, TEX, SPEC>(a, g, tex, lights...);
}

}  // namespace
}  // namespace rt
