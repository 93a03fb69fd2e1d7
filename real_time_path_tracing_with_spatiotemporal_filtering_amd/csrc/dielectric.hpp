// dielectric.hpp — the dielectric interface (rtpt_scene_set_materials_ext, RTPT_MAT_DIELECTRIC): Fresnel reflection or refraction
// at a perfectly smooth surface.  ONE definition, used by every kernel that shades a hit (shade_segment.hpp: shade_segment<..., SPEC = 2>)
// and by the self test (rtpt_selftest_refract).  Not reference behaviour: the reference traces neither.
//
// The arithmetic, contract functions only (rtpt_math.hpp: exact::dot, exact::sqrt_, exact::normalize, fmaf_) and plain binary32
// products and differences, stated so that numpy float32 reproduces it bit for bit (the build has -ffp-contract=off: only the
// fmas written here fuse; tests/dielectric_scenes.py restates it).  n: the triangle's unit normal AS STORED, pointing out of the
// medium; d: the unit ray direction; u1, u2: the segment's two RNG floats in the order the diffuse bounce draws them; ior >= 1.
// The host computes in binary32 and stores in the record   inv = 1.0f / ior,   q = (ior - 1.0f) / (ior + 1.0f),   R0 = q * q.
//   side          c = dot(n, d);  entering = c < 0;  nf = entering ? n : -n  (the diffuse bounce's faceforward);
//                 eta = entering ? inv : ior
//   cosines       ci = -dot(nf, d);  s2 = (eta * eta) * fmaf(-ci, ci, 1);  k = 1 - s2;  tir = !(k > 0);  ct = sqrt_(k) unless tir
//   Fresnel       Schlick, with the cosine on the rarer side:  x = 1 - (entering ? ci : ct);  x2 = x * x;  x5 = (x2 * x2) * x;
//                 F = fmaf(1 - R0, x5, R0);  under tir F = 1
//   choice        reflect exactly when tir || u1 < F.  Both draws are always taken, so a pixel's random stream does not depend on
//                 the materials its path meets; u2 is unused
//   reflected     d' = normalize(fmaf(2 * ci, nf, d)) per component;  origin fmaf(ray_offset, nf, pos), as for every other bounce
//   transmitted   a = fmaf(eta, ci, -ct);  d' = normalize(fmaf(a, nf, eta * d)) per component;  origin fmaf(-ray_offset, nf, pos),
//                 on the far side of the surface
// A dielectric hit is never absorbed.  ior is meant to be a physical index (1 to about 3): beyond 1.8e19 eta^2 overflows
// and every hit from inside reflects (inf * 0 is a NaN, and !(NaN > 0) is total reflection); where a * nf cancels eta * d to the
// last bit (ior above about 1e7, u1 = F = 1) the direction is a NaN, and such a ray meets nothing and ends in the sky's lower half.
// The LAST segment of a path returns its throughput before any of this, as for every hit.
// The two directions are one expression, d' = normalize(fmaf(w, nf, m * d)) with (w, m) = (2 * ci, 1) or (a, eta): 1 * d is d in
// every bit, so the kernels select two scalars, not two vectors, and the origin's offset gets its sign the same way — the hit
// point is live once.
//
// The device record (SceneView::materials): m0 = (colour, ior), m1 = (inv, R0, 0, 0).  ior >= 1 > 0 keeps the spare word apart
// from the diffuse 0 and the specular -roughness (specular.hpp).
#pragma once

#include "rtpt_math.hpp"

namespace rt {
namespace diel {

__device__ __forceinline__ bool is_dielectric(float m0w) { return m0w > 0.0f; }

// nf: the FACEFORWARDED normal, entering: the stored one faced the ray (dot(n, d) < 0).  Returns d'; *transmitted: the path
// crosses the surface (the origin goes to the far side); *fresnel: F.
__device__ __forceinline__ f3 interface(f3 nf, bool entering, f3 d, float u1, float ior, float inv, float r0, bool* transmitted,
                                        float* fresnel) {
  const float eta = entering ? inv : ior;
  const float ci = -exact::dot(nf, d);
  const float s2 = (eta * eta) * fmaf_(-ci, ci, 1.0f);
  const float k = 1.0f - s2;
  const bool tir = !(k > 0.0f);
  const float ct = tir ? 0.0f : exact::sqrt_(k);
  const float x = 1.0f - (entering ? ci : ct);
  const float x2 = x * x;
  const float x5 = (x2 * x2) * x;
  const float F = tir ? 1.0f : fmaf_(1.0f - r0, x5, r0);
  const bool reflect = tir || u1 < F;
  const float w = reflect ? 2.0f * ci : fmaf_(eta, ci, -ct);
  const float m = reflect ? 1.0f : eta;
  *transmitted = !reflect;
  *fresnel = F;
  return exact::normalize(f3{fmaf_(w, nf.x, m * d.x), fmaf_(w, nf.y, m * d.y), fmaf_(w, nf.z, m * d.z)});
}

// the whole interface from its operands: the side, the record's two derived values, the choice (rtpt_selftest_refract)
__device__ __forceinline__ f3 refract(f3 n, f3 d, float u1, float ior, bool* transmitted, float* fresnel) {
  const bool entering = exact::dot(n, d) < 0.0f;
  if (!entering) n = -n;
  const float q = (ior - 1.0f) / (ior + 1.0f);
  return interface(n, entering, d, u1, ior, 1.0f / ior, q * q, transmitted, fresnel);
}

}  // namespace diel
}  // namespace rt
