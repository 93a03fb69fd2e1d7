// specular.hpp — the specular bounce (rtpt_scene_set_materials_ext, RTPT_MAT_SPECULAR).  ONE definition, used by every kernel that
// shades a hit (shade_segment.hpp: shade_segment<..., SPEC = 1>) and by the self test (rtpt_selftest_bounce).  Not reference
// behaviour: the reference traces no reflection (its only reflect() is a highlight of the gradient shader).  A material is
// diffuse or specular, never a mixture; no Fresnel term, no refraction here — a smooth dielectric is a third kind of material,
// dielectric.hpp.
//
// The arithmetic, contract functions only (rtpt_math.hpp), stated so that numpy float32 reproduces it bit for bit (the build
// has -ffp-contract=off: only the fmas written here fuse; tests/specular_scenes.py restates it).  n: the triangle's unit normal,
// d: the unit ray direction, u1, u2: the segment's two RNG floats in the order the diffuse bounce draws them
// (raytrace.comp.glsl:256-257), g: the material's roughness in [0, 1]:
//   faceforward        if (!(dot(n, d) < 0)) n = -n                                    as the diffuse bounce (:247)
//   mirror direction   c = dot(n, d);  r = fmaf(-2c, n, d)                            per component, -2c = -2.0f * c (exact)
//   sphere point       (sn, cs) = sincos2pi(u1);  u = fmaf(2, u2, -1);  rho = sqrt(fmaf(-u, u, 1))      (:256-258)
//                      s = (rho * cs, rho * sn, u)                                     each product rounded to binary32
//   lobe               d' = normalize(fmaf(g, s, r))                                   per component
//   absorption         !(dot(n, d') > 0): the lobe left the surface (a NaN too) — the path ends with colour 0
// g == 0 is a perfect mirror (d' = normalize(r)) and still takes both draws, so a pixel's random stream does not depend on the
// materials its path meets.  The LAST segment of a path (seg + 1 >= max_segments) returns its throughput before any bounce, as
// for a diffuse hit: it is never absorbed.
//
// The device record (SceneView::materials, m0.w — the spare word of the first float4): 0 (all bits) = diffuse; specular =
// -g, so the mirror is -0.0f (0x80000000) and every g in [0, 1] is kept exactly.
#pragma once

#include "rtpt_math.hpp"

namespace rt {
namespace spec {

__device__ __forceinline__ bool is_specular(float m0w) { return f2u(m0w) != 0u; }
__device__ __forceinline__ float roughness(float m0w) { return __builtin_fabsf(m0w); }

// the lobe around the mirror direction of d at the FACEFORWARDED normal n; rho, cs, sn, u: the sphere point's parts as the
// diffuse bounce computes them.  Returns d'; *absorbed: d' does not leave the surface.
__device__ __forceinline__ f3 lobe(f3 n, f3 d, float rho, float cs, float sn, float u, float g, bool* absorbed) {
  const float c2 = -2.0f * exact::dot(n, d);
  const f3 r{fmaf_(c2, n.x, d.x), fmaf_(c2, n.y, d.y), fmaf_(c2, n.z, d.z)};
  const f3 s{rho * cs, rho * sn, u};
  const f3 dn = exact::normalize(f3{fmaf_(g, s.x, r.x), fmaf_(g, s.y, r.y), fmaf_(g, s.z, r.z)});
  *absorbed = !(exact::dot(n, dn) > 0.0f);
  return dn;
}

// the whole bounce from its operands: faceforward, the sphere point of the two draws, the lobe (rtpt_selftest_bounce)
__device__ __forceinline__ f3 bounce(f3 n, f3 d, float u1, float u2, float g, bool* absorbed) {
  if (!(exact::dot(n, d) < 0.0f)) n = -n;
  float sn, cs;
  exact::sincos2pi(u1, sn, cs);
  const float u = fmaf_(2.0f, u2, -1.0f);
  const float rho = exact::sqrt_(fmaf_(-u, u, 1.0f));
  return lobe(n, d, rho, cs, sn, u, g, absorbed);
}

}  // namespace spec
}  // namespace rt
