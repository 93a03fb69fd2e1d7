// shade_segment.hpp — one path segment after its closest-hit query (raytrace.comp.glsl:226-267), stated once for the tile
// kernels and the queue kernel (pathtrace_tile.hpp, kernels.hip): the light test, the sky, the albedo with its textures, and the
// diffuse, specular or dielectric bounce.  The self-test kernels (selftest_kernels.hip) call its pieces.  Everything here is
// force-inlined.
#pragma once

#include "closest_hit.hpp"
#include "dielectric.hpp"
#include "env.hpp"
#include "light_sample.hpp"
#include "shading_normal.hpp"
#include "specular.hpp"

#include <type_traits>

namespace rt {
namespace {

// ------------------------------------------------------------------------------------------
// K2 path trace
// ------------------------------------------------------------------------------------------
// raytrace.comp.glsl:168-198 — only the boolean is consumed (:226), and the sphere is tested
// regardless of the triangle hit distance (the light is never occluded)
__device__ __forceinline__ bool ray_hits_light(f3 o, f3 d, f3 c, float r2) {
  f3 oc = o - c;
  float a = exact::dot(d, d);
  float b = 2.0f * exact::dot(oc, d);
  float cc = exact::dot(oc, oc) - r2;
  float disc = fmaf_(b, b, -((4.0f * a) * cc));
  if (disc < 0.0f) return false;
  float sq = exact::sqrt_(disc);
  // :190-197 "t1 > 0 || t2 > 0" with t1 = (-b - sq) / 2a, t2 = (-b + sq) / 2a.  sq >= 0 and 2a >= 0, and both the
  // addition and the correctly-rounded division are monotonic, so t1 <= t2 whenever neither is NaN: t1 > 0 implies
  // t2 > 0, and the disjunction IS "t2 > 0" (NaN operands make both comparisons false either way; 2a == 0 gives +-inf /
  // NaN with the same signs).  One division less per path segment.
#if RTPT_TRACE_ITEMS & 2
  // ... and of t2 only the sign is asked for: exact::quotient_positive is "num / den > 0.0f" on every pair of operands and
  // divides only where the sign is not num's (2a is 2 |d|^2, about 2)
  return exact::quotient_positive(-b + sq, 2.0f * a);
#else
  float t2 = RTPT_DIV_SH(-b + sq, 2.0f * a);
  return t2 > 0.0f;
#endif
}

__device__ __forceinline__ f3 sky_color(f3 d) {  // raytrace.comp.glsl:95-107
  if (d.y > 0.0f) {
    float t = d.y, it = 1.0f - t;
    return f3{fmaf_(0.25f, t, it), fmaf_(0.5f, t, it), fmaf_(1.0f, t, it)};
  }
  return f3{0.03f, 0.03f, 0.03f};
}

// the colour of a pixel of an "rgbd" image without touching its alpha (one global_store_dwordx3)
__device__ __forceinline__ void store_rgb(float4* px, f3 c) {
  typedef float v3f_ __attribute__((ext_vector_type(3)));
  *reinterpret_cast<v3f_*>(px) = v3f_{c.x, c.y, c.z};
}

// The level a hit's texture is sampled at (texture.hpp states the arithmetic): the footprint of segment 0 is the pixel's,
// t * 2 * slope / H of the FULL frame, so strips agree; every later segment starts over from its own length, t * spread —
// nothing is carried between segments.  Density and areas come from the hit's own records, so instances, a changed model
// and moved instances are right without host bookkeeping.  td: the hit's descriptor; s, t0, t1: its shade and uv records.
__device__ __forceinline__ float hit_texture_lod(const TexDesc td, float4 s0, float4 s1, float4 s2, float4 t0, float4 t1, float t, f3 d,
                                                 bool primary, float slope, int frame_h, float bounce_spread) {
  if (!(td.flags & kTexMipmap)) return 0.0f;
  const float w = t * (primary ? (2.0f * slope) / static_cast<float>(frame_h) : bounce_spread);
  return tex::footprint_lod(w, exact::dot(f3{s0.w, s1.w, s2.w}, d), s0, s1, s2, t0, t1, td.width, td.height);
}

// b1 = -u / ad, b2 = v / ad, b0 = 1 - b1 - b2 (:134).  SHORT_DIV: exact::div2_, for the wave-uniform brute-force kernels that have
// the registers; the BVH kernels, pinned at 64 VGPRs, keep hipcc's divisions (RTPT_DIV_SH, closest_hit.hpp)
template <bool SHORT_DIV>
__device__ __forceinline__ void hit_barycentrics(const HitRec& h, float& b0, float& b1, float& b2) {
  if (SHORT_DIV) {
    exact::div2_(-h.u, h.v, h.ad, b1, b2);
  } else {
    b1 = RTPT_DIV_SH(-h.u, h.ad);
    b2 = RTPT_DIV_SH(h.v, h.ad);
  }
  b0 = 1.0f - b1 - b2;
}

// One path segment after its closest-hit query (raytrace.comp.glsl:226-267): the unoccluded light test, the sky, or a
// diffuse bounce.  Returns true when the path ended (its colour is then `acc`).
// alb_px (RTPT_FLAG_EXT_DEMODULATE; non-NULL only at segment 0 of the tile kernel): the pixel of PathtraceArgs::albedo.  The
// albedo of this hit goes there instead of into the throughput, and a path that ends here stores (1, 1, 1) and keeps its colour.
// TEX: the scene has albedo textures (rtpt_scene_set_textures): the albedo is (Kd or the normal-keyed colour) x texel.rgb, one
// multiply per channel, at every segment.  A compile-time switch for DEMOD's reason: the instantiations without it are the
// kernels of a build that knows no textures, register for register.  TEX == 2: some texture of the scene has RTPT_TEX_MIPMAP,
// and the texel comes from the level of the ray's footprint (hit_texture_lod, tex::sample_lod); 1: level 0, as before mips.
// BVH: the caller's closest-hit structure; SHORT_DIV: see hit_barycentrics (the defaults are the kernels before either).
// The LAST segment of a path (seg + 1 >= a.max_segments — the path's budget, not the launch's window seg_end: behind a window
// boundary the queue kernel goes on with o, d and rng) ends after its throughput update: the hit point, the faceforward, the
// offset origin, the two draws' floats, sincos2pi, the square root and the normalize make an o and a d that nothing reads.  What
// stays: the barycentrics where the hit samples a texture, and with samples_per_pixel > 1 the two steps of the RNG state, which
// the pixel's next sample continues from (rng_pix, pathtrace_tile).
// Two places keep the bounce, for their registers (make resource-usage, profiles/r15_trace_shading_ab.txt): the untextured
// instantiations over fan pairs (BVH == 2, TEX == 0; pinned at 64 VGPRs with 8 to 14 spilled ones — the early return cost
// k_gbuffer_pathtrace<2, false, 0>, the kernel of the instanced frame, one more: 36 -> 40 bytes of scratch) and the segment that
// stores the albedo plane (alb_px; 0 -> 8 bytes in the brute-force DEMOD kernels), which is a path's last only with max_segments 1.
// SPEC (kernels.hpp names the axis and its predicates; every value is a compile-time switch for DEMOD's and TEX's reason, and each is
// the instantiation before it, statement for statement, where its predicate is false):
// spec_material(SPEC) >= 1: some triangle's material is specular (rtpt_scene_set_materials_ext; specular.hpp states the bounce): such
// a hit takes Ks where a diffuse one takes Kd — the record's colour, so everything above happens to it unchanged — and leaves along
// the lobe around its mirror direction, with the same two draws.  These instantiations return early on every last segment (no
// exception for their registers: they are new), so that no schedule absorbs a path there.
// spec_material(SPEC) == 2: some triangle's material is a dielectric too (RTPT_MAT_DIELECTRIC; dielectric.hpp states the interface):
// such a hit takes the record's colour the same way, takes both draws, and leaves reflected or refracted by its first draw against
// the Fresnel term.  The origin is formed after the choice, its offset's sign selected once, so that the hit point is live once (the
// BVH variants are pinned at 64 VGPRs).
// spec_lights(SPEC): the light sample of next-event estimation besides (RTPT_FLAG_EXT_NEE on a scene whose light list has entries;
// light_sample.hpp states the rules, the estimator and the order of the draws).  A DIFFUSE hit that is not the path's last segment
// takes three more draws (u_l, u_a, u_b) behind its offset origin and in front of the bounce's two, samples one point of one
// entry of the list and leaves in `nee` the shadow ray's direction, the triangle it must reach and the colour the pixel's radiance
// gains if it does, (T * Ke) * g per channel; the caller sends the query (pathtrace_tile).  nee.sampled is the path's sampled bit:
// set by such a hit whether or not the sample was valid, cleared by a specular or dielectric one, and an emissive triangle met
// with the bit set ends the path with colour 0 — its light was already collected at the hit before.
// spec_sphere(SPEC): the sample of the analytic sphere light too (RTPT_FLAG_EXT_NEE_SPHERE; light_sample.hpp states the rules):
// two more draws (u_c, u_p) behind the triangle sample's three, no query; the gain (T * light_col) * g is left in `nee` (sphere_c,
// sphere_valid) for the caller to add to R before it sends the triangle's shadow query, and nee.sphere is the path's sphere bit,
// with which a segment that meets the light ends with colour 0.  Without the weighted pick the triangle sample is taken only where
// the list has entries (wave-uniform): with the sphere flag alone these instantiations run without a list and without a material
// table.  A compile-time switch because a run-time one cost the kernels that sample triangles only 3.5 % of a frame with the switch
// off (profiles/r23_nee_sphere_measure.txt).
// spec_power(SPEC): the weighted pick of RTPT_FLAG_EXT_NEE_POWER (light_sample.hpp: pick_power): the draw u_l names an entry through
// the cumulative table that travels with the list (spec_lights_t<SPEC> is then LightTableView), and the sample's weight takes the
// inverse of the pick's probability where the uniform pick's takes L.  The list has entries wherever these are launched.
// spec_mis(SPEC): RTPT_FLAG_EXT_NEE_MIS (light_sample.hpp: MULTIPLE IMPORTANCE SAMPLING): the sample's weight g becomes g * m(g); a
// diffuse hit that goes on leaves the cosine of its new direction in nee.cb; and an emissive triangle met with the sampled bit set
// ends the path with (T * Ke) * wb(g_hit) where the others end it with 0 — that return needs the hit's barycentrics, also on a
// path's last segment.  The list has entries wherever these are launched.  The sphere sample is as without the bit.
struct NeeState {
  f3 wd;          // the shadow ray's direction, from the path's new origin
  f3 c;           // (T * Ke) * g
  uint32_t id1;   // the sampled triangle, id + 1
  bool valid;     // this segment took a sample whose shadow query is to be sent
  bool sampled;   // the path's sampled bit
  f3 sphere_c;        // spec_sphere(SPEC): (T * light_col) * g of the sphere sample
  bool sphere_valid;  // ... this segment took a sphere sample that adds sphere_c to R
  bool sphere;        // ... the path's sphere bit
  float cb;           // spec_mis(SPEC): the cosine the path's last diffuse bounce left with; read only while `sampled` is set
};
// what the instantiations that sample lights take behind alb_px (LV: their spec_lights_t<SPEC>), and what every other one takes
// there: nothing.  (As two more parameters with defaults, a list and a pointer nobody read, the untextured queue kernels came out
// with their registers renamed.)
template <class LV>
struct NeeArgs {
  LV lights;
  NeeState* st;
};
struct NoNee {};
// NRM (NV = NormalView; every other instantiation takes NoNormals there, nothing, and is the instantiation before the axis, statement
// for statement): the scene has vertex normals (rtpt_scene_set_normals; shading_normal.hpp states the rules).  A hit on a triangle
// whose record is smooth bounces, refracts and samples lights about the interpolated normal ns; the offset origin and everything
// above the bounce keep the geometric normal.  These instantiations return early on every last segment, like the specular ones.
struct NoNormals {};
// ENV (EV = EnvView; every other instantiation takes NoEnv there, nothing, and is the instantiation before the axis, statement for
// statement): the context has an environment map (rtpt_set_environment; env.hpp states the lookup).  A path that meets nothing is
// multiplied by env::color(d) where the others multiply by sky_color(d).  Nothing else changes: the light test comes first, the albedo
// plane of such a path is (1, 1, 1), and no path changes direction, length or random stream.
struct NoEnv {};
// the hit's ns by rules 1 to 7, from the records of base triangle (id1 - 1) % n_base and the matrix of instance (id1 - 1) / n_base;
// false (ns = ng) where the hit is not smooth.  The matrix is loaded only behind a smooth record.
__device__ __forceinline__ bool hit_shading_normal(const NormalView& nv, uint32_t id1, uint32_t n_base, float b0, float b1, float b2, f3 ng, f3 d,
                                                   f3* ns) {
  *ns = ng;
  const uint32_t t = (id1 - 1) % n_base, i = (id1 - 1) / n_base;
  const float4* r = nv.records + 3 * static_cast<size_t>(t);
  const float4 r0 = r[0];
  if (__float_as_uint(r0.w) == 0u) return false;
  const float4 r1 = r[1], r2 = r[2];
  const float4* c = nv.cof + 3 * static_cast<size_t>(i);
  const float4 c0 = c[0], c1 = c[1], c2 = c[2];
  f3 n;
  if (!nrm::interpolate(xyz(r0), xyz(r1), xyz(r2), b0, b1, b2, xyz(c0), xyz(c1), xyz(c2), &n)) return false;
  *ns = nrm::orient(n, ng, d);
  return true;
}
template <int TEX, int BVH = 1, bool SHORT_DIV = false, int SPEC = 0, class NEE = NoNee, class NV = NoNormals, class EV = NoEnv>
__device__ __forceinline__ bool shade_segment(const PathtraceArgs& a, const HitRec& h, uint32_t seg, f3 light_c, f3& o, f3& d,
                                              f3& acc, uint32_t& rng, const TexView& tex, float4* alb_px = nullptr,
                                              [[maybe_unused]] NEE nee_args = NEE{}, [[maybe_unused]] NV normals = NV{},
                                              [[maybe_unused]] EV envmap = EV{}) {
  static_assert(std::is_same<NEE, std::conditional_t<spec_lights(SPEC), NeeArgs<spec_lights_t<SPEC>>, NoNee>>::value,
                "the instantiations that sample lights, and only they, take NeeArgs, with the list their SPEC asks for");
  constexpr bool NRM = std::is_same<NV, NormalView>::value;
  static_assert(NRM || std::is_same<NV, NoNormals>::value, "NormalView or nothing");
  constexpr bool ENV = std::is_same<EV, EnvView>::value;
  static_assert(ENV || std::is_same<EV, NoEnv>::value, "EnvView or nothing");
  if (ray_hits_light(o, d, light_c, a.light_r2)) {  // :226
    acc = acc * (seg == 0 ? ld3(a.light_col_first) : ld3(a.light_col));  // :229,:233
    if constexpr (spec_sphere(SPEC)) {
      if (nee_args.st->sphere) acc = f3{0.f, 0.f, 0.f};  // the hit before sampled the sphere: this hit's light is counted there
    }
    if (alb_px) *alb_px = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    return true;
  }
  if (h.id1 == 0) {
    if constexpr (ENV)
      acc = acc * env::color(envmap, d);  // the environment map where the reference has its sky
    else
      acc = acc * sky_color(d);  // :266
    if (alb_px) *alb_px = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    return true;
  }
  const float4* s = a.scene.shade + 3 * static_cast<size_t>(h.id1 - 1);
  float4 s0 = s[0], s1 = s[1], s2 = s[2];
  const bool last = (RTPT_TRACE_ITEMS & 1) && (spec_material(SPEC) != 0 || NRM || (!(BVH == 2 && TEX == 0) && !alb_px)) && seg + 1 >= a.max_segments;  // block-uniform
  float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
  f3 pos{0.f, 0.f, 0.f};
  if (!last) {
    hit_barycentrics<SHORT_DIV>(h, b0, b1, b2);
    pos = bary_point(xyz(s0), xyz(s1), xyz(s2), b0, b1, b2);      // :137
  }
  f3 n{s0.w, s1.w, s2.w};                                          // :150 (precomputed per triangle)
  [[maybe_unused]] float spec_w = 0.0f;  // SPEC: the record's spare word, 0 = diffuse (specular.hpp), > 0 = the ior (dielectric.hpp)
  [[maybe_unused]] float diel_inv = 0.0f, diel_r0 = 0.0f;  // spec_material(SPEC) == 2: 1 / ior and R0 of a dielectric's record
  f3 alb = (n.x > 0.99f) ? f3{1.f, 0.f, 0.f} : ((-n.x > 0.99f) ? f3{0.f, 1.f, 0.f} : f3{0.7f, 0.7f, 0.7f});  // :155-163
  if (a.scene.materials) {
    // SURVEY 8(f) rank 4, not reference behaviour: a material library replaces the normal-keyed colours; a surface
    // with emission ends the path like the analytic light does (:226-234), throughput *= Ke
    const float4* m = a.scene.materials + 2 * static_cast<size_t>((h.id1 - 1) % a.scene.n_base_tris);
    const float4 m0 = m[0], m1 = m[1];
    if (m1.w != 0.0f) {
      acc = acc * f3{m1.x, m1.y, m1.z};
      if constexpr (spec_lights(SPEC)) {
        if constexpr (spec_mis(SPEC)) {
          // the hit before sampled the lights: this emission is one of two estimators, weighed by the power heuristic
          if (nee_args.st->sampled) {
            const spec_lights_t<SPEC> lights = nee_args.lights;
            float e0, e1, e2;
            hit_barycentrics<SHORT_DIV>(h, e0, e1, e2);
            float inv_p = static_cast<float>(lights.n);
            bool reached = true;  // the pick can name this emitter
            if constexpr (spec_power(SPEC)) reached = light::hit_inv_p_power(lights.ids, lights.cdf, lights.n, h.id1, &inv_p);
            float wb = 1.0f;
            if (reached)
              wb = light::mis_bounce(light::hit_weight(xyz(s0), xyz(s1), xyz(s2), f3{s0.w, s1.w, s2.w}, o, d, e0, e1, e2, nee_args.st->cb, inv_p));
            acc = f3{acc.x * wb, acc.y * wb, acc.z * wb};
          }
        } else {
          if (nee_args.st->sampled) acc = f3{0.f, 0.f, 0.f};  // the hit before sampled the lights: this one's emission is counted there
        }
      }
      if (alb_px) *alb_px = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
      return true;
    }
    alb = f3{m0.x, m0.y, m0.z};
    if constexpr (spec_material(SPEC) != 0) spec_w = m0.w;
    if constexpr (spec_material(SPEC) == 2) {
      diel_inv = m1.x;
      diel_r0 = m1.y;
    }
  }
  if (TEX) {
    const float4* tr = tex.records + 2 * static_cast<size_t>((h.id1 - 1) % a.scene.n_base_tris);
    const float4 t0 = tr[0], t1 = tr[1];
    const uint32_t ti = __float_as_uint(t1.z);
    if (ti) {
      if (last) hit_barycentrics<SHORT_DIV>(h, b0, b1, b2);
      const float tu = tex::interp_uv(b0, b1, b2, t0.x, t0.z, t1.x), tv = tex::interp_uv(b0, b1, b2, t0.y, t0.w, t1.y);
      float4 tx;
      if constexpr (TEX == 2) {
        const TexDesc td = tex.desc[ti - 1];
        const float lambda = hit_texture_lod(td, s0, s1, s2, t0, t1, h.t, d, seg == 0, a.slope, a.g.H, tex.bounce_spread);
        tx = tex::sample_lod(td, tex.levels + kTexLevelRow * static_cast<size_t>(ti - 1), tex.texels, tu, tv, lambda);
      } else {
        tx = tex::sample(tex.desc[ti - 1], tex.texels, tu, tv);
      }
      alb = f3{alb.x * tx.x, alb.y * tx.y, alb.z * tx.z};
    }
  }
  if (alb_px)
    *alb_px = make_float4(alb.x, alb.y, alb.z, 0.0f);  // demodulated: rtpt_modulate / rtpt_present multiply it back
  else
    acc = acc * alb;                                               // :244
  if (last) {  // budget exhausted: the path returns its throughput (:270)
    if (a.spp > 1) {
      exact::rng_skip(rng);  // :256
      exact::rng_skip(rng);  // :257
    }
    return true;
  }
  if constexpr (spec_material(SPEC) == 2) {
    if (diel::is_dielectric(spec_w)) {
      if constexpr (spec_lights(SPEC)) nee_args.st->sampled = false;
      if constexpr (spec_sphere(SPEC)) nee_args.st->sphere = false;
      const bool entering = exact::dot(n, d) < 0.0f;
      if (!entering) n = -n;
      const float u1 = exact::rng_next(rng);                       // :256
      exact::rng_skip(rng);                                        // :257 (drawn, unused)
      bool transmitted;
      float fresnel;
      if constexpr (NRM) {
        f3 ns;
        const bool smooth = hit_shading_normal(normals, h.id1, a.scene.n_base_tris, b0, b1, b2, n, d, &ns);
        d = diel::interface(ns, entering, d, u1, spec_w, diel_inv, diel_r0, &transmitted, &fresnel);
        float off = transmitted ? -a.ray_offset : a.ray_offset;
        if (smooth) off = nrm::dielectric_offset(d, n, a.ray_offset);
        o = f3{fmaf_(off, n.x, pos.x), fmaf_(off, n.y, pos.y), fmaf_(off, n.z, pos.z)};
        return seg + 1 >= a.max_segments;
      }
      d = diel::interface(n, entering, d, u1, spec_w, diel_inv, diel_r0, &transmitted, &fresnel);
      const float off = transmitted ? -a.ray_offset : a.ray_offset;
      o = f3{fmaf_(off, n.x, pos.x), fmaf_(off, n.y, pos.y), fmaf_(off, n.z, pos.z)};
      return seg + 1 >= a.max_segments;  // never absorbed (only builds without the early return get here on a last segment)
    }
  }
  if (!(exact::dot(n, d) < 0.0f)) n = -n;                          // :247 faceforward
  o = f3{fmaf_(a.ray_offset, n.x, pos.x), fmaf_(a.ray_offset, n.y, pos.y), fmaf_(a.ray_offset, n.z, pos.z)};  // :250
  // NRM: from here on n is the shading normal ns and ng the geometric one (shading_normal.hpp); without the axis both names are gone
  [[maybe_unused]] f3 ng = n;
  [[maybe_unused]] bool smooth = false;
  if constexpr (NRM) smooth = hit_shading_normal(normals, h.id1, a.scene.n_base_tris, b0, b1, b2, ng, d, &n);
  if constexpr (spec_lights(SPEC)) {
    // next-event estimation (light_sample.hpp): o is the sample's x, n its nf, acc its T
    const spec_lights_t<SPEC> lights = nee_args.lights;
    NeeState* const nee = nee_args.st;
    const bool diffuse = !spec::is_specular(spec_w);
    if (diffuse && seg + 1 < a.max_segments) {
      // the list has entries, except where the sphere light is sampled without the weighted pick: there it may be empty (wave-uniform)
      constexpr bool kMayBeEmpty = spec_may_be_empty(SPEC);
      if (!kMayBeEmpty || lights.n > 0) {
        const float u_l = exact::rng_next(rng);
        const float u_a = exact::rng_next(rng);
        const float u_b = exact::rng_next(rng);
        uint32_t entry;
        float inv_p;  // of the pick's probability
        if constexpr (spec_power(SPEC)) {
          const light::Pick pk = light::pick_power(u_l, lights.cdf, lights.n);
          entry = pk.i;
          inv_p = pk.inv_p;
        } else {
          entry = light::pick(u_l, lights.n);
          inv_p = static_cast<float>(lights.n);
        }
        const uint32_t id1 = lights.ids[entry];
        const float4* ls = a.scene.shade + 3 * static_cast<size_t>(id1 - 1);
        const float4 l0 = ls[0], l1 = ls[1], l2 = ls[2];
        const float4 ke = a.scene.materials[2 * static_cast<size_t>((id1 - 1) % a.scene.n_base_tris) + 1];
        const light::Sample sm = light::sample(xyz(l0), xyz(l1), xyz(l2), f3{l0.w, l1.w, l2.w}, o, n, u_a, u_b, inv_p);
        nee->wd = sm.wd;
        float g = sm.g;
        if constexpr (spec_mis(SPEC)) g = sm.g * light::mis_light(sm.g);  // gm: one multiply behind the division
        nee->c = f3{(acc.x * ke.x) * g, (acc.y * ke.y) * g, (acc.z * ke.z) * g};  // two roundings a channel, in this order
        nee->id1 = id1;
        nee->valid = sm.valid;
        if constexpr (NRM) {
          if (smooth) nee->valid = sm.valid && nrm::sample_side(sm.wd, ng);
        }
        nee->sampled = true;
      }
      if constexpr (spec_sphere(SPEC)) {  // the sphere sample: light_c, a.light_r2 and a.light_col are ray_hits_light's light
        const float u_c = exact::rng_next(rng);
        const float u_p = exact::rng_next(rng);
        const light::SphereSample ss = light::sphere_sample(o, n, light_c, a.light_r2, u_c, u_p);
        const f3 lc = ld3(a.light_col);
        nee->sphere_c = f3{(acc.x * lc.x) * ss.g, (acc.y * lc.y) * ss.g, (acc.z * lc.z) * ss.g};
        nee->sphere_valid = ss.valid;
        if constexpr (NRM) {
          if (smooth) nee->sphere_valid = ss.valid && nrm::sample_side(ss.wd, ng);
        }
        nee->sphere = ss.taken;
      }
    } else if (!diffuse) {
      nee->sampled = false;
      if constexpr (spec_sphere(SPEC)) nee->sphere = false;
    }
  }
  float st_, ct;
  exact::sincos2pi(exact::rng_next(rng), st_, ct);                 // :256
  float u = fmaf_(2.0f, exact::rng_next(rng), -1.0f);              // :257
  float r = exact::sqrt_(fmaf_(-u, u, 1.0f));                      // :258
  if constexpr (spec_material(SPEC) != 0) {
    if (spec::is_specular(spec_w)) {
      bool absorbed;
      d = spec::lobe(n, d, r, ct, st_, u, spec::roughness(spec_w), &absorbed);
      if (seg + 1 >= a.max_segments) return true;  // (only builds without the early return get here)
      if constexpr (NRM) {
        if (smooth && nrm::absorbed(d, ng)) absorbed = true;
      }
      if (absorbed) acc = f3{0.f, 0.f, 0.f};
      return absorbed;
    }
  }
  d = exact::normalize(f3{fmaf_(r, ct, n.x), fmaf_(r, st_, n.y), n.z + u});  // :259-261
  if constexpr (spec_mis(SPEC)) nee_args.st->cb = exact::dot(n, d);  // (a last segment returned above: this hit took the triangle draw)
  if constexpr (NRM) {
    if (seg + 1 >= a.max_segments) return true;  // (only builds without the early return get here)
    if (smooth && nrm::absorbed(d, ng)) {
      acc = f3{0.f, 0.f, 0.f};
      return true;
    }
    return false;
  }
  return seg + 1 >= a.max_segments;  // budget exhausted: the path returns its throughput (:270)
}

// shade_segment's TEX for with_mode<3> (select.hpp): 2 the scene has textures and some of them a mip chain (the level table
// exists), 1 textures without mips, 0 no textures
inline int tex_mode(const TexView& tex) { return tex.records ? (tex.levels ? 2 : 1) : 0; }
// shade_segment's SPEC of a launch's `specular` (kernels.hpp: the SPEC axis): the value itself where it lies on the axis, else 0;
// an unnamed value above kSpecNeeSphere samples the sphere light
inline int spec_mode(int specular) {
  if (specular < 0) return 0;
  return specular < kSpecModes ? specular : kSpecNeeSphere;
}

}  // namespace
}  // namespace rt
