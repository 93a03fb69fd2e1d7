// shading_normal.hpp — smooth shading (rtpt_scene_set_normals): THE statement of how a hit's interpolated vertex normal is
// formed, carried through the hit's pose and kept on the right side of the real surface.  shade_segment (shade_segment.hpp) is the
// only user in a frame; rtpt_selftest_shading_normal runs the same functions operand by operand, and tests/normal_paths.py restates
// them in numpy.  Everything is binary32 in the order written here; -ffp-contract=off, every fused multiply-add is spelled fmaf_.
//
// DEVICE DATA (kernels.hpp: NormalView), two small arrays:
//   records  three float4 per BASE triangle t: (n0.xyz, smooth as bits), (n1.xyz, 0), (n2.xyz, 0) — the corners' normals in the
//            mesh's own space, in rtpt_scene_upload's triangle and corner order; smooth == 0: the triangle keeps its geometric normal
//   cof      three float4 per INSTANCE i: the rows of the cofactor matrix C_i of L_i (w = 0), where L_i is the 3 x 3 linear part of
//            model x instance transform (linear_part below).  C = det(L) L^-T carries a normal through any affine pose, mirrors
//            included, without a division: for a mirror det < 0 turns the normal over, and rule 6 turns it back.
// A hit with id1 reads record t = (id1 - 1) % n_base_tris and matrix i = (id1 - 1) / n_base_tris.
//
// THE RULES, at a hit whose record has smooth != 0 and that is not the path's early-returning last segment:
//   1. m  = b0 n0 + b1 n1 + b2 n2 with the hit's barycentrics: per component fma(b2, n2, fma(b1, n1, b0 * n0))
//   2. w  = C_i m, row by row: w.r = fma(C[r][2], m.z, fma(C[r][1], m.y, C[r][0] * m.x))
//   3. ns = exact::normalize(w)
//   4. any component of ns NaN or infinite (a zero w gives NaN): the triangle is NOT SMOOTH AT THIS HIT — today's statements run,
//      the three side tests below included in "not run"
//   5. ng = the geometric normal after the faceforward (raytrace.comp.glsl:247), or after the dielectric's entering test
//   6. dot(ns, ng) < 0: ns = -ns      (inverted vn records and mirrored poses shade like their proper twins)
//   7. !(dot(ns, d) < 0): ns = ng     (the silhouette: the interpolated normal faces away from the incoming ray; the hit stays smooth)
// ng keeps: the offset origin, the dielectric's entering test, the normal-keyed albedo, the texture footprint, an emitter's own
// cosine and area, K0's ids, world positions and depth, K1, the LUT, the reprojection, the same-primitive tests, and every filter
// kernel of a context without RTPT_FLAG_EXT_SMOOTH_GUIDE.  ns takes: the diffuse direction normalize(ns + point), spec::lobe's
// mirror axis, diel::interface's normal, nf of light::sample and light::sphere_sample, the cosine cb of RTPT_FLAG_EXT_NEE_MIS.
//
// THE GUIDE NORMAL (RTPT_FLAG_EXT_SMOOTH_GUIDE, active while the context has the flag and the scene holds normals): what K0
// (gbuffer_tile.hpp) writes into the per-pixel normal plane that the filter's edge stop reads, at a pixel whose pixel-centre ray
// hits id1 > 0, from K0's own barycentrics b0, b1, b2 (the ones that form its world position):
//   G1-G3. rules 1 to 3 (interpolate), with record (id1 - 1) % n_base_tris and the cof rows of instance (id1 - 1) / n_base_tris
//   G4.    the record is not smooth, or interpolate returns false (a NaN or infinite ns; a zero w gives NaN), or ns is the zero vector
//          (a w whose squared length overflows binary32, normals of length 1e20: normalize scales it by 1 / inf; in a path rule 7
//          catches that ns, here nothing would, and a zero cell weighs every tap of its pixel 0): the cell is normal_tab[id1], all
//          four words, as without the switch
//   G5.    ng = xyz(normal_tab[id1]), the LUT's unfaced normal that G4 stores; dot(ns, ng) < 0: ns = -ns   (inverted vn records and
//          mirrored poses agree with their not-smooth neighbours)
//   Rules 5 and 7 are not applied: the guide does not depend on the incoming ray.
//   The cell is (ns.x, ns.y, ns.z, powi(max(0, dot(ns, ns)), sigma_n)), k_lut's formula for normal_tab[t + 1].w; id 0 keeps
//   normal_tab[0].  tests/guide_normals.py restates G1-G5 in numpy.
// THE SIDE TESTS, at a smooth hit (rule 4 passed), keep rays off the wrong side of the real surface:
//   * a diffuse or specular direction d' with !(dot(d', ng) > 0) is absorbed: the path ends with colour 0 (what R holds is kept);
//   * a light sample or sphere sample is valid only if dot(wd, ng) > 0 as well (draws, sampled bit and sphere bit as they were);
//   * a dielectric is never absorbed: its origin offset is -ray_offset where dot(d', ng) < 0 and +ray_offset otherwise, whatever
//     the `transmitted` flag says.
// The draws, their count and their order are unchanged everywhere.
#pragma once

#include "rtpt_math.hpp"

namespace rt {
namespace nrm {

// L = the 3 x 3 linear part of model x xf, row-major in l[9]: model is column-major 4 x 4 (rtpt_ubo::model, m[4 c + r]), xf a row-major
// 3 x 4 instance transform or NULL (one identity instance: L is the model's).  The product is what launch_pose applies to what
// k_flatten wrote, as one matrix: L[r][c] = fma(M[r][2], X[2][c], fma(M[r][1], X[1][c], M[r][0] * X[0][c])).
RT_HD void linear_part(const float* model, const float* xf, float* l) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++)
      l[3 * r + c] = xf ? fmaf_(model[8 + r], xf[8 + c], fmaf_(model[4 + r], xf[4 + c], model[r] * xf[c])) : model[4 * c + r];
}

// The nine 2 x 2 minors with their signs: c[3 r + k] = cofactor (r, k) of the row-major l.  Each is (p * q) - (s * t): two rounded
// products and one rounded subtraction, never fused, so the host route and the device route agree bit for bit.
RT_HD void cofactor(const float* l, float* c) {
  c[0] = (l[4] * l[8]) - (l[5] * l[7]);
  c[1] = (l[5] * l[6]) - (l[3] * l[8]);
  c[2] = (l[3] * l[7]) - (l[4] * l[6]);
  c[3] = (l[2] * l[7]) - (l[1] * l[8]);
  c[4] = (l[0] * l[8]) - (l[2] * l[6]);
  c[5] = (l[1] * l[6]) - (l[0] * l[7]);
  c[6] = (l[1] * l[5]) - (l[2] * l[4]);
  c[7] = (l[2] * l[3]) - (l[0] * l[5]);
  c[8] = (l[0] * l[4]) - (l[1] * l[3]);
}

// the twelve floats of instance i's three cof rows (w = 0) from the model and the instance's transform (NULL: none)
RT_HD void cof_rows(const float* model, const float* xf, float* out12) {
  float l[9], c[9];
  linear_part(model, xf, l);
  cofactor(l, c);
  for (int r = 0; r < 3; r++) {
    out12[4 * r] = c[3 * r];
    out12[4 * r + 1] = c[3 * r + 1];
    out12[4 * r + 2] = c[3 * r + 2];
    out12[4 * r + 3] = 0.0f;
  }
}

RT_HD bool finite_(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

// rules 1 to 4: false where the hit is not smooth (*ns is then not to be read)
RT_HD bool interpolate(f3 n0, f3 n1, f3 n2, float b0, float b1, float b2, f3 c0, f3 c1, f3 c2, f3* ns) {
  const f3 m{fmaf_(b2, n2.x, fmaf_(b1, n1.x, b0 * n0.x)), fmaf_(b2, n2.y, fmaf_(b1, n1.y, b0 * n0.y)), fmaf_(b2, n2.z, fmaf_(b1, n1.z, b0 * n0.z))};
  const f3 w{fmaf_(c0.z, m.z, fmaf_(c0.y, m.y, c0.x * m.x)), fmaf_(c1.z, m.z, fmaf_(c1.y, m.y, c1.x * m.x)),
             fmaf_(c2.z, m.z, fmaf_(c2.y, m.y, c2.x * m.x))};
  const f3 n = exact::normalize(w);
  *ns = n;
  return finite_(n.x) && finite_(n.y) && finite_(n.z);
}

// rules 6 and 7, on the ns of a smooth hit
RT_HD f3 orient(f3 ns, f3 ng, f3 d) {
  if (exact::dot(ns, ng) < 0.0f) ns = -ns;
  if (!(exact::dot(ns, d) < 0.0f)) ns = ng;
  return ns;
}

// G1 to G5 without the cell: false where the cell is normal_tab[id1] (G4; *ns is then not to be read).  ng = xyz(normal_tab[id1])
RT_HD bool guide(f3 n0, f3 n1, f3 n2, float b0, float b1, float b2, f3 c0, f3 c1, f3 c2, f3 ng, f3* ns) {
  f3 n;
  if (!interpolate(n0, n1, n2, b0, b1, b2, c0, c1, c2, &n)) return false;
  if (n.x == 0.0f && n.y == 0.0f && n.z == 0.0f) return false;  // |w|^2 overflowed: normalize scaled w by 1 / inf
  if (exact::dot(n, ng) < 0.0f) n = -n;
  *ns = n;
  return true;
}
// the fourth word of a guide cell: the self weight pow(max(0, dot(ns, ns)), sigma_n) as k_lut forms it
RT_HD float guide_self_weight(f3 ns, int sigma_n) { return exact::powi(glsl_max(0.0f, exact::dot(ns, ns)), sigma_n); }

// the side tests
RT_HD bool absorbed(f3 d_new, f3 ng) { return !(exact::dot(d_new, ng) > 0.0f); }          // a diffuse or specular direction
RT_HD bool sample_side(f3 wd, f3 ng) { return exact::dot(wd, ng) > 0.0f; }                 // a light or sphere sample stays valid
RT_HD float dielectric_offset(f3 d_new, f3 ng, float ray_offset) { return exact::dot(d_new, ng) < 0.0f ? -ray_offset : ray_offset; }

}  // namespace nrm
}  // namespace rt
