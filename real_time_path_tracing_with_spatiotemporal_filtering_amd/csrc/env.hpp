// env.hpp — the environment map (rtpt_set_environment): the colour of a path that meets nothing.  ONE definition, env::color, used
// by the instantiations of shade_segment that take an EnvView (kernels.hpp: the ENV axis) where every other one multiplies by
// sky_color(d), and by the lookup self test (rtpt_selftest_environment).  Not reference behaviour: the reference's sky is the
// constant gradient of raytrace.comp.glsl:95-107.  No image instructions, no LDS: plain 16-byte global loads of RGBA32F texels.
//
// The map is OCTAHEDRAL, a square of n x n texels: the contract has no atan2 and no acos, and this lookup needs none.  The rules,
// stated so that numpy float32 reproduces them bit for bit (the build has -ffp-contract=off: only the fmas written here fuse;
// tests/environment_maps.py restates them, include/rtpt.h repeats them for callers):
//   E1  e = (dot(r0, d), dot(r1, d), dot(r2, d)) with exact::dot; r0, r1, r2 the rows of the environment's rotation.  Always
//       computed: a call without a rotation stores the identity.
//   E2  s = (|e.x| + |e.y|) + |e.z|.  !(s > 0) or s infinite: the colour is (0, 0, 0) and no texel is read — a NaN, the zero
//       direction, an infinite or overflowing component.
//   E3  p = e.x / s, q = e.z / s (exact::div_, correctly rounded).  The upper sheet is e.y >= 0.0f (a -0 is on it).
//   E4  upper sheet: (u, v) = (p, q).  Lower sheet: u = copysign(1 - |q|, p), v = copysign(1 - |p|, q).
//   E5  U = fma(u, 0.5, 0.5), V = fma(v, 0.5, 0.5); row 0 holds V in [0, 1/n), column 0 U in [0, 1/n).
//       bilinear (the default): x = U * (float)n - 0.5f, x0 = floorf(x), f = x - x0; the taps are clamp((int)x0, 0, n - 1) and
//       clamp((int)x0 + 1, 0, n - 1); rows likewise from V; the four texels combine as tex::sample combines them, tex::lerp4 along
//       x for both rows, then along y.
//       RTPT_TEX_NEAREST: the texel (min(n - 1, (int)floorf(U * (float)n)), the same of V).
//       Addressing is CLAMPED, not repeated: the square's edges are the folds of the lower hemisphere, and a tap beyond an edge
//       belongs to the texel mirrored along that edge, not to this one.  Known limit: half a texel of error along those four lines.
//   E6  colour = texel.rgb * scale.rgb, one multiply per channel.
// Bounds: s >= |e.x| and s >= |e.z| (a rounded sum of non-negative terms is no smaller than either), so |p|, |q| <= 1, u and v lie in
// [-1, 1], U and V in [0, 1], and every index is clamped to [0, n - 1] besides; the host refuses n == 0 (that is "no environment")
// and n > 4096, so an index times n stays far below 2^32.  No lane reads outside the n x n texels.
#pragma once

#include "kernels.hpp"
#include "rtpt_math.hpp"

namespace rt {
namespace env {

__device__ __forceinline__ int clamp_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

__device__ __forceinline__ f3 color(const EnvView& ev, f3 d) {
  const f3 e{exact::dot(f3{ev.r0.x, ev.r0.y, ev.r0.z}, d), exact::dot(f3{ev.r1.x, ev.r1.y, ev.r1.z}, d),
             exact::dot(f3{ev.r2.x, ev.r2.y, ev.r2.z}, d)};                                                  // E1
  const float s = (__builtin_fabsf(e.x) + __builtin_fabsf(e.y)) + __builtin_fabsf(e.z);                      // E2
  if (!(s > 0.0f) || s == __builtin_inff()) return f3{0.f, 0.f, 0.f};
  const float p = exact::div_(e.x, s), q = exact::div_(e.z, s);                                              // E3
  float u = p, v = q;                                                                                        // E4
  if (!(e.y >= 0.0f)) {
    u = __builtin_copysignf(1.0f - __builtin_fabsf(q), p);
    v = __builtin_copysignf(1.0f - __builtin_fabsf(p), q);
  }
  const float U = fmaf_(u, 0.5f, 0.5f), V = fmaf_(v, 0.5f, 0.5f);                                            // E5
  const int n = static_cast<int>(ev.n);
  const float fn = static_cast<float>(n);
  float4 t;
  if (ev.flags & kTexNearest) {
    const int i = clamp_index(static_cast<int>(__builtin_floorf(U * fn)), n);
    const int j = clamp_index(static_cast<int>(__builtin_floorf(V * fn)), n);
    t = ev.texels[static_cast<uint32_t>(j) * ev.n + static_cast<uint32_t>(i)];
  } else {
    const float x = U * fn - 0.5f, y = V * fn - 0.5f;
    const float x0 = __builtin_floorf(x), y0 = __builtin_floorf(y);
    const float fx = x - x0, fy = y - y0;
    const int i0 = clamp_index(static_cast<int>(x0), n), i1 = clamp_index(static_cast<int>(x0) + 1, n);
    const int j0 = clamp_index(static_cast<int>(y0), n), j1 = clamp_index(static_cast<int>(y0) + 1, n);
    const uint32_t r0 = static_cast<uint32_t>(j0) * ev.n, r1 = static_cast<uint32_t>(j1) * ev.n;
    const float4 a = ev.texels[r0 + static_cast<uint32_t>(i0)], b = ev.texels[r0 + static_cast<uint32_t>(i1)];
    const float4 c = ev.texels[r1 + static_cast<uint32_t>(i0)], g = ev.texels[r1 + static_cast<uint32_t>(i1)];
    t = tex::lerp4(tex::lerp4(a, b, fx), tex::lerp4(c, g, fx), fy);
  }
  return f3{t.x * ev.scale.x, t.y * ev.scale.y, t.z * ev.scale.z};                                           // E6
}

}  // namespace env
}  // namespace rt
