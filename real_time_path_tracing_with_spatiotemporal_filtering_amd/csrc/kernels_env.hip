// kernels_env.hip — the instantiations of the ENV axis of the K2 tile kernels (kernels.hpp: EnvView; env.hpp: the lookup), the
// kernels of a context with an environment map (rtpt_set_environment), and their selection table.
//
// A translation unit of its own, unlike every other kernel of the frame (kernels.hip says why those share one): an environment
// launch shares its grid with K0 + K1 only through the fused tile kernels, which are instantiated here with it, and with K3 never
// (it carries no final pass); and what kernels.hip's kernels are compiled to must not move when this axis is added.  The dynamic
// LDS array `stack` is first declared here by the tile body, aligned(16): it starts at byte 32 of these kernels' LDS where
// kernels.hip's start at byte 24, which nothing reads (PathtraceArgs::multi_off counts from the array's own start).
//
// The product: scene mode (3) x DEMOD (2) x TEX (3) x SPEC (kSpecModes) x {fused, unfused compacting} x NRM (the BVH modes only).
// RTPT_ENV_PART = 0 .. 4 compiles one part of it (the Makefile builds the five side by side); undefined, all of them
// (scripts/device_asm_diff.py, make resource-usage).
#include "select.hpp"
#include "tile_kernels.hpp"

#ifndef RTPT_ENV_PART
#define RTPT_ENV_PART -1
#endif
#define RTPT_ENV_HAS(p) (RTPT_ENV_PART == -1 || RTPT_ENV_PART == (p))

namespace rt {
namespace {

// scene mode M, with a NormalView (N) or without: DEMOD x TEX x SPEC x {fused, unfused}
template <int M, bool N>
void launch_env_part(const PathtraceArgs& b, const GbufferArgs* gb, const TexView& tex, int spec, dim3 grid, dim3 block, size_t dyn, hipStream_t s,
                     const LightTableView& lights, const NormalView& normals, const EnvView& envmap) {
  static_assert(M != 0 || !N, "a scene with normals traces through its tree");
  with_bool(b.albedo != nullptr, [&](auto demod) {
    constexpr bool D = decltype(demod)::value;
    with_mode<3>(tex_mode(tex), [&](auto tmode) {
      constexpr int T = decltype(tmode)::value;
      with_mode<kSpecModes>(spec, [&](auto smode) {
        constexpr int S = decltype(smode)::value;
        const auto go = [&](auto... l) {  // (the launch syntax: kernels.hip's `go` says why)
          if (gb) {
            if constexpr (M != 0)
              k_gbuffer_pathtrace<M, D, T, S><<<grid, block, dyn, s>>>(b, *gb, tex, l...);
            else
              k_gbuffer_pathtrace_small<D, T, S><<<grid, block, dyn, s>>>(b, *gb, tex, l...);
          } else {
            if constexpr (M != 0)
              k_pathtrace<M, true, D, T, S><<<grid, block, dyn, s>>>(b, tex, l...);
            else
              k_pathtrace_small<true, D, T, S><<<grid, block, dyn, s>>>(b, tex, l...);
          }
        };
        const auto with_lights = [&](auto... n) {
          if constexpr (spec_power(S))
            go(lights, n...);
          else if constexpr (spec_lights(S))
            go(LightView{lights.ids, lights.n}, n...);
          else
            go(n...);
        };
        if constexpr (N)
          with_lights(normals, envmap);
        else
          with_lights(envmap);
      });
    });
  });
}

}  // namespace

#define RTPT_ENV_PART_DEF(p, M, N)                                                                                                     \
  void launch_pathtrace_env_p##p(const PathtraceArgs& b, const GbufferArgs* gb, const TexView& tex, int spec, dim3 grid, dim3 block, \
                                 size_t dyn, hipStream_t s, const LightTableView& lights, const NormalView& normals, const EnvView& envmap) { \
    launch_env_part<M, N>(b, gb, tex, spec, grid, block, dyn, s, lights, normals, envmap);                                             \
  }
#if RTPT_ENV_HAS(0)
RTPT_ENV_PART_DEF(0, 0, false)
#endif
#if RTPT_ENV_HAS(1)
RTPT_ENV_PART_DEF(1, 1, false)
#endif
#if RTPT_ENV_HAS(2)
RTPT_ENV_PART_DEF(2, 1, true)
#endif
#if RTPT_ENV_HAS(3)
RTPT_ENV_PART_DEF(3, 2, false)
#endif
#if RTPT_ENV_HAS(4)
RTPT_ENV_PART_DEF(4, 2, true)
#endif

}  // namespace rt
