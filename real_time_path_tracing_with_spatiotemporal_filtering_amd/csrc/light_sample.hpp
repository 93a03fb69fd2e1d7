// light_sample.hpp — the light sample of next-event estimation: one point on one emissive triangle per diffuse hit, stated once.
// The instantiations of the tile kernels that sample lights call it (spec_lights(SPEC): shade_segment.hpp, pathtrace_tile.hpp), and
// the self test (rtpt_selftest_light_sample, k_selftest_light_sample).  Below it, the sample of the analytic sphere light
// (sphere_sample, RTPT_FLAG_EXT_NEE_SPHERE), which the spec_sphere(SPEC) instantiations call besides.  Not reference behaviour: the reference collects light only by hitting
// it.  Contract functions only (rtpt_math.hpp), no new transcendental; tests/nee_scenes.py restates every step in numpy float32,
// tests/nee_paths.py walks whole paths with it.
//
// THE RULES (RTPT_FLAG_EXT_NEE on a scene whose light list has L > 0 entries; in every other case frames, ray counts and the
// kernels chosen are those of a context without the flag, bit for bit):
//   * A sample is taken at a DIFFUSE hit that is not the path's last segment (seg + 1 < max_segments): after the albedo went into
//     the throughput T (into the albedo plane at segment 0 with RTPT_FLAG_EXT_DEMODULATE), after the faceforward and the offset
//     origin x = o, before the bounce's two draws.
//   * Three draws u_l, u_a, u_b in that order; entry i = pick(u_l, L) names posed triangle id = lights[i] (id + 1, as
//     HitRec::id1); its vertices and unit normal come from its shade record, its Ke from the material record of
//     (id - 1) % n_base_tris; s = sample(v0, v1, v2, nl, x, nf, u_a, u_b, float(L)).
//   * If s.valid, ONE closest-hit query goes from x along s.wd, with the launch's tmax and the path's own closest_hit<BVH>, tie
//     rule included; if it returns id, the pixel's radiance R gains ((T.c * Ke.c) * s.g) per channel c: two multiplies in that
//     order, one addition into R, a rounding each.  The query counts as a ray for pixels inside the count rows.
//   * The path's SAMPLED BIT is set by such a hit whether or not the sample was valid; a specular or dielectric hit takes no light
//     draw (its random stream is unchanged) and clears it; the primary ray starts with it clear.  The bounce then takes its two
//     draws as before.  A path's last segment takes no light draw and sends no query (with samples_per_pixel > 1 its two rng_skip
//     stay two).
//   * A path that meets an emissive triangle with the bit set ends with terminal colour 0, with the bit clear with T * Ke as
//     without the flag.  The analytic sphere light, the sky and the end of the segment budget end a path as without the flag: none
//     of them is sampled.
//   * The pixel stores R + terminal, one addition per channel; with samples_per_pixel > 1 that value goes into the sample sum and
//     R restarts at 0 for every sample.  With demodulation T at segment 0 lacks the first albedo, so the gain of segment 0 is
//     illumination, like the terminal colour; an emitter seen directly stores albedo (1, 1, 1).
//
// The estimator at a diffuse hit x with shading normal nf (faced against the ray) and albedo alb already in the throughput T:
//   light i uniform among the L entries of the scene's light list, y uniform on it by area (pdf 1 / (L * area)),
//   contribution T * Ke * (alb / pi is in T but for the 1 / pi) * cos(x) * cos(y) / r^2 / pdf = (T * Ke) * g with
//   g = ((cs * cl) * (a2 * L)) / (2 pi * r2),   a2 = |cross(v1 - v0, v2 - v0)| = twice the area,
// counted when the closest hit from x towards y is that triangle.
#pragma once

#include "closest_hit.hpp"
#include "light_list_host.hpp"

namespace rt {
namespace light {

constexpr float k2Pi = 6.28318548202514648f;  // the binary32 nearest 2 pi
constexpr uint32_t kMaxLights = 1u << 24;     // u_l has 24 bits: a longer list would have entries the pick never reaches (the
                                              // bound a light list has to keep; the self test is told L).  The weighted
                                              // pick (RTPT_FLAG_EXT_NEE_POWER, below) has a limit of the same kind: an entry
                                              // whose quantised weight q_i has q_i * 2^24 < S can be skipped by all 2^24 values
                                              // of the draw, and its share of the light is lost; that needs S > 2^24, hundreds of
                                              // full-weight lights beside one of the smallest weight
static_assert(kMaxLights == rtpt_light::kMaxLights, "the host refuses the lists the pick cannot reach");

// entry of a list of L > 0 lights that draw u_l in [0, 1) picks
__device__ __forceinline__ uint32_t pick(float u_l, uint32_t L) {
  const uint32_t i = static_cast<uint32_t>(u_l * static_cast<float>(L));
  return i < L - 1u ? i : L - 1u;
}

struct Sample {
  f3 y;       // the point on the light
  f3 wd;      // unit direction from x to it
  float g;    // the weight of (T * Ke)
  bool valid; // x faces the light's plane from a distance and the light has an area: only then is the shadow query sent
};

// v0, v1, v2, nl: the light's vertices and unit normal (its shade record); x: the bounce origin; nf: the hit's normal, faced
// against the arriving ray; u_a, u_b: the draws behind u_l; inv_p: the inverse of the pick's probability — float(L) for the
// uniform pick among L entries, Pick::inv_p for the weighted one
__device__ __forceinline__ Sample sample(f3 v0, f3 v1, f3 v2, f3 nl, f3 x, f3 nf, float u_a, float u_b, float inv_p) {
  Sample s;
  const float su = exact::sqrt_(u_a);
  const float b0 = 1.0f - su, b1 = su * (1.0f - u_b), b2 = su * u_b;
  s.y = bary_point(v0, v1, v2, b0, b1, b2);
  const f3 w = s.y - x;
  const float r2 = exact::dot(w, w);
  s.wd = exact::normalize(w);
  const float cs = exact::dot(nf, s.wd);
  const float cl = __builtin_fabsf(exact::dot(nl, s.wd));  // emitters shine from both sides, as they do when a path hits them
  const f3 c = exact::cross(v1 - v0, v2 - v0);
  const float a2 = exact::sqrt_(exact::dot(c, c));
  s.valid = (cs > 0.0f) && (cl > 0.0f) && (r2 > 0.0f) && (a2 > 0.0f);  // NaN fails every comparison
  s.g = exact::div_((cs * cl) * (a2 * inv_p), k2Pi * r2);
  return s;
}

// ------------------------------------------------------------------------------------------------------------------------------
// THE WEIGHTED PICK (RTPT_FLAG_EXT_NEE_POWER together with RTPT_FLAG_EXT_NEE on a scene whose light list has L > 0 entries; alone,
// or with only RTPT_FLAG_EXT_NEE_SPHERE, the bit is ignored, and without it every frame, ray count, kernel and allocation is that of
// a context without it, bit for bit).  Every rule above holds unchanged — the place of the sample, the three draws and their
// order, the sampled bit, the shadow query and its tie rule, R — except two: WHICH ENTRY the draw u_l names, and that float(L) in
// g becomes inv_p, the inverse of the pick's probability.  Entries are picked in proportion to area times emission, from a
// cumulative table of integers that light_table.hip builds on the device; all of its arithmetic is fixed so that a parallel build
// gives the same bits in any order.  tests/nee_power.py restates weights, table and pick, and walks whole paths with them.
//   * Weight of entry i (posed id, vertices from its shade record, Ke from material record (id - 1) % n_base_tris): w_i = a2_i * k_i,
//     a2_i = sample()'s a2 (exact::cross, exact::dot, exact::sqrt_), k_i = max(|Ke.r|, |Ke.g|, |Ke.b|) as k = |r|; if (|g| > k)
//     k = |g|; if (|b| > k) k = |b|.  A w_i that is NaN, infinite or not > 0 counts as 0: a degenerate emitter is never picked.
//   * w_max = max_i w_i: of non-negative finite floats, so the unsigned maximum of their bit patterns, in any order.
//   * Quantised weight q_i: 1 for every entry where w_max == 0 (the uniform pick); else max(1, uint32(exact::div_(w_i, w_max) *
//     65536.0f)) where w_i > 0 and 0 elsewhere.  q_i <= 2^16.
//   * C_i = sum_{j <= i} q_j as uint64, S = C_{L-1} <= 2^40: integer sums, any scan order.  8 bytes an entry.
//   * Pick: m = uint32(u_l * 2^24), exact since a draw is a multiple of 2^-24; t = (uint64(m) * S) >> 24 (the product is below
//     2^64); the entry is the smallest i with C_i > t, by binary search; inv_p = exact::div_(float(S), float(q_i)), the
//     uint64 -> binary32 conversion rounding to nearest even.
//   * g = exact::div_((cs * cl) * (a2 * inv_p), k2Pi * r2): sample() above, with this inv_p where the uniform pick passes float(L).
// KNOWN LIMIT, of the kind of kMaxLights: an entry with q_i * 2^24 < S can be skipped by all 2^24 values of the draw, and its
// share of the light is then lost.  That needs S > 2^24: hundreds of full-weight lights beside one of the smallest weight.
constexpr float kPickScale = 16777216.0f;    // 2^24
constexpr float kWeightScale = 65536.0f;     // 2^16: the quantised weight of the heaviest entry

// w_i of the rules above from the light's vertices and its Ke, before "counts as 0"
__device__ __forceinline__ float weight(f3 v0, f3 v1, f3 v2, f3 ke) {
  const f3 c = exact::cross(v1 - v0, v2 - v0);
  const float a2 = exact::sqrt_(exact::dot(c, c));
  const float r = __builtin_fabsf(ke.x), g = __builtin_fabsf(ke.y), b = __builtin_fabsf(ke.z);
  float k = r;
  if (g > k) k = g;
  if (b > k) k = b;
  return a2 * k;
}
// ... and "counts as 0": the bits of w where it is finite and > 0, else 0
__device__ __forceinline__ uint32_t weight_bits(float w) {
  return (w > 0.0f && w < __builtin_inff()) ? f2u(w) : 0u;
}
// q_i of a weight that went through weight_bits, given the maximum's bits
__device__ __forceinline__ uint32_t quantise(uint32_t w_bits, uint32_t w_max_bits) {
  if (w_max_bits == 0u) return 1u;
  if (w_bits == 0u) return 0u;
  const uint32_t q = static_cast<uint32_t>(exact::div_(u2f(w_bits), u2f(w_max_bits)) * kWeightScale);
  return q > 1u ? q : 1u;
}

struct Pick {
  uint32_t i;    // the entry
  float inv_p;   // S / q_i
};
// entry of the table C[0, L), L > 0, that draw u_l in [0, 1) picks.  Every index read lies in [0, L) whatever u_l and C hold.
__device__ __forceinline__ Pick pick_power(float u_l, const uint64_t* C, uint32_t L) {
  const uint64_t S = C[L - 1u];
  const uint32_t m = static_cast<uint32_t>(u_l * kPickScale);
  const uint64_t t = (static_cast<uint64_t>(m) * S) >> 24;
  uint32_t lo = 0u, hi = L - 1u;  // t < S = C[L - 1]: the answer lies in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (C[mid] > t)
      hi = mid;
    else
      lo = mid + 1u;
  }
  const uint64_t q = C[lo] - (lo ? C[lo - 1u] : 0ull);
  return Pick{lo, exact::div_(static_cast<float>(S), static_cast<float>(q))};
}

// ------------------------------------------------------------------------------------------------------------------------------
// MULTIPLE IMPORTANCE SAMPLING (RTPT_FLAG_EXT_NEE_MIS together with RTPT_FLAG_EXT_NEE on a scene whose light list has L > 0 entries,
// with the uniform or the weighted pick, with or without RTPT_FLAG_EXT_NEE_SPHERE; alone, with only the sphere flag, or on an empty
// list the bit is ignored, and in every ignored case and without it every frame, ray count, kernel and allocation is that of a
// context without it, bit for bit).  The light sample and the bounce that meets the same emitter are two estimators of one
// integral; each is weighed by the POWER HEURISTIC (beta = 2).  Everything not named here is as the rules above state it: the place
// of the sample, the three draws and their order, the sampled bit, the shadow query and its tie rule, R, the order of the sphere's
// and the triangle's additions, demodulation.  THE SPHERE SAMPLE AND THE SPHERE BIT ARE UNCHANGED: the cone sample of a sphere is
// already close to the bounce's own density; its weighing is left for later.  tests/nee_mis.py restates every step in numpy float32
// and walks whole paths with it.
//   With g2 = g * g:   light side   m(g)  = exact::div_(1.0f, 1.0f + g2)
//                      bounce side  wb(g) = (g2 < +inf) ? exact::div_(g2, 1.0f + g2) : 1.0f        (a NaN fails the comparison)
//   g is the ratio of the bounce's density cs / pi to the light sample's density in solid angle, so these are p_l^2 / (p_l^2 +
//   p_b^2) and p_b^2 / (p_l^2 + p_b^2).
//   1. THE LIGHT SAMPLE: sample()'s g becomes gm = g * m(g), one multiply behind the division; the gain is ((T.c * Ke.c) * gm) per
//      channel.  gm <= 0.5 wherever it is a number (g = +inf gives inf * 0, a NaN, as g = NaN does).  Validity, the query and the
//      ray count are unchanged.
//   2. THE BOUNCE'S COSINE: a diffuse hit that is not the path's last segment and that took the triangle draw records cb =
//      exact::dot(nf, d') behind the normalize of the diffuse direction d'.  cb travels with the path like the sampled bit, is read
//      only while that bit is set, and nothing resets it: the primary ray starts with the bit clear.
//   3. AN EMISSIVE TRIANGLE MET WITH THE SAMPLED BIT SET ends the path with (T * Ke) * wb(g_hit): the multiply by Ke as before,
//      then one multiply by wb per channel — no longer 0.  With the bit clear: T * Ke, as before.  g_hit is the light sample's
//      weight function at the point the ray hit (hit_weight below): y = bary_point of the hit's barycentrics on the hit triangle's
//      shade record, as shade_segment forms a bounce's hit point; w = y - o; r2 = exact::dot(w, w); cl = |exact::dot(nl, d)| with
//      the ray's own unit d and the record's normal; a2 as sample() computes it; g_hit = exact::div_((cb * cl) * (a2 * inv_p),
//      k2Pi * r2).  inv_p is float(L) for the uniform pick; for the weighted pick it is the hit triangle's: i = the index of the
//      hit's id1 in the ascending list (rtpt_light::find, light_list_host.hpp: a binary search, every index read in [0, L)),
//      q_i = C_i - C_{i-1}, inv_p = exact::div_(float(S), float(q_i)) as pick_power forms it.  Where q_i == 0 the pick never
//      reaches that emitter, so the hit before collected nothing for it: wb = 1; likewise for an id the list does not hold, which
//      no frame can produce.
// KNOWN LIMITS, inherited: an entry the weighted pick's 24-bit draw can skip (q_i * 2^24 < S) still loses that share; a launch
// with the flag has a sampling launch's limits (every segment in the tile kernel, no queues, no deferred final pass).
__device__ __forceinline__ float mis_light(float g) {
  const float g2 = g * g;
  return exact::div_(1.0f, 1.0f + g2);
}
__device__ __forceinline__ float mis_bounce(float g) {
  const float g2 = g * g;
  return (g2 < __builtin_inff()) ? exact::div_(g2, 1.0f + g2) : 1.0f;
}
// g_hit of rule 3.  v0, v1, v2, nl: the hit emitter's vertices and unit normal (its shade record); o, d: the ray that hit it;
// b0, b1, b2: the hit's barycentrics (hit_barycentrics); cb: the cosine the bounce left with; inv_p: of the pick that would name
// this emitter
__device__ __forceinline__ float hit_weight(f3 v0, f3 v1, f3 v2, f3 nl, f3 o, f3 d, float b0, float b1, float b2, float cb, float inv_p) {
  const f3 y = bary_point(v0, v1, v2, b0, b1, b2);
  const f3 w = y - o;
  const float r2 = exact::dot(w, w);
  const float cl = __builtin_fabsf(exact::dot(nl, d));
  const f3 c = exact::cross(v1 - v0, v2 - v0);
  const float a2 = exact::sqrt_(exact::dot(c, c));
  return exact::div_((cb * cl) * (a2 * inv_p), k2Pi * r2);
}
// inv_p of the weighted pick for the emitter id1 of the list ids[0, L) with the table C[0, L), L > 0; false where the pick never
// names it (q_i == 0, or the list does not hold it): the bounce's weight is then 1
__device__ __forceinline__ bool hit_inv_p_power(const uint32_t* ids, const uint64_t* C, uint32_t L, uint32_t id1, float* inv_p) {
  const uint32_t i = rtpt_light::find(ids, L, id1);
  if (i >= L) return false;
  const uint64_t q = C[i] - (i ? C[i - 1u] : 0ull);
  if (q == 0ull) return false;
  *inv_p = exact::div_(static_cast<float>(C[L - 1u]), static_cast<float>(q));
  return true;
}

// ------------------------------------------------------------------------------------------------------------------------------
// THE SPHERE SAMPLE (RTPT_FLAG_EXT_NEE_SPHERE, independent of RTPT_FLAG_EXT_NEE and combinable with it; without the flag frames,
// ray counts and the kernels chosen are those of a context without it, bit for bit): one direction inside the cone the analytic
// sphere light (centre c = lightPos, squared radius r2 = PathtraceArgs::light_r2) subtends from x.  ray_hits_light tests the
// sphere whatever the triangle hit distance — the light is never occluded — so the sample needs no shadow query: no query is sent
// and no ray is counted.  tests/nee_sphere.py restates every step in numpy float32 and walks whole paths with it.
//   * Where: at a DIFFUSE hit that is not the path's last segment (seg + 1 < max_segments), the triangle sample's place: after the
//     albedo, the faceforward and the offset origin x = o, before the bounce's two draws.
//   * Draws: two, u_c then u_p, behind the triangle sample's three where that one is taken and in front of the bounce's two; taken
//     whether or not the sample turns out valid.  A specular or dielectric hit takes none, nor does a last segment (with
//     samples_per_pixel > 1 its two rng_skip stay two).
//   * The sample: sphere_sample below, step by step.  TAKEN when d2 > r2 (NaN fails; x inside or on the sphere fails: every bounce
//     from there hits the light anyway).  VALID when taken and cs = dot(nf, wd) > 0.
//   * Weight g = (2 cs) k with k = 1 - cos(theta_max): the bounce's pdf is cs / pi and the cone's 1 / (2 pi k), so a bounce that
//     returns T * light_col on a hit has the expectation of (T * light_col) * g.  The colour is PathtraceArgs::light_col, never
//     light_col_first: the sample stands for a hit at segment >= 1.  A valid sample adds ((T.c * light_col.c) * g) per channel c to
//     the pixel's radiance R: two multiplies in this order, one addition, a rounding each.
//   * Where a hit takes both samples the sphere's gain goes into R first, the triangle's after its shadow query.
//   * The path's SPHERE BIT (0x200 of the pix word through the compaction, beside the sampled bit 0x100): set by a diffuse non-last
//     hit whose sample was taken, valid or not; cleared by a diffuse hit whose sample was not taken and by a specular or dielectric
//     hit; clear on the primary ray.  A segment whose ray_hits_light is true with the bit set ends the path with terminal colour
//     0, with the bit clear as without the flag.  The bit does not touch emissive triangles, the sampled bit not the sphere.
//   * With demodulation T at segment 0 lacks the first albedo, so the gain of segment 0 is illumination, as the triangle's.
struct SphereSample {
  f3 wd;       // unit direction from x into the cone
  float g;     // the weight of (T * light_col)
  bool taken;  // d2 > r2
  bool valid;  // taken and the direction leaves the surface
};

// x: the bounce origin; nf: the hit's normal, faced against the arriving ray; c, r2: the light; u_c, u_p: the two draws
__device__ __forceinline__ SphereSample sphere_sample(f3 x, f3 nf, f3 c, float r2, float u_c, float u_p) {
  SphereSample s;
  const f3 dc = c - x;
  const float d2 = exact::dot(dc, dc);
  const f3 w = exact::normalize(dc);
  const float q = exact::div_(r2, d2);                  // sin^2(theta_max)
  const float cm = exact::sqrt_(1.0f - q);              // cos(theta_max); NaN where q > 1: not taken
  const float k = exact::div_(q, 1.0f + cm);            // 1 - cm without the cancellation of a far light (LIGHT_FAR: q = 1.6e-9)
  const float ct = fmaf_(-u_c, k, 1.0f);                // uniform in [cm, 1]
  const float st = exact::sqrt_(glsl_max(0.0f, fmaf_(-ct, ct, 1.0f)));  // glsl_max: 0 where the operand is NaN
  float sp, cp;
  exact::sincos2pi(u_p, sp, cp);
  // an orthonormal pair (t, b) around w, branch-free and without a singular direction (Duff et al. 2017, the copysign form):
  //   sg = copysign(1, w.z);  a = -1 / (sg + w.z);  b_ = (w.x * w.y) * a;  sx = sg * w.x
  //   t = (fma(sx, w.x * a, 1), sg * b_, -sx),  b = (b_, fma(w.y, w.y * a, sg), -w.y)
  const float sg = __builtin_copysignf(1.0f, w.z);
  const float a = exact::div_(-1.0f, sg + w.z);
  const float b_ = (w.x * w.y) * a;
  const float sx = sg * w.x;
  const f3 t{fmaf_(sx, w.x * a, 1.0f), sg * b_, -sx};
  const f3 b{b_, fmaf_(w.y, w.y * a, sg), -w.y};
  // v = (st cp) t + (st sp) b + ct w, per channel fma(ct, w, fma(st sp, b, (st cp) * t))
  const float ac = st * cp, as = st * sp;
  s.wd = exact::normalize(f3{fmaf_(ct, w.x, fmaf_(as, b.x, ac * t.x)), fmaf_(ct, w.y, fmaf_(as, b.y, ac * t.y)),
                             fmaf_(ct, w.z, fmaf_(as, b.z, ac * t.z))});
  const float cs = exact::dot(nf, s.wd);
  s.taken = d2 > r2;  // NaN fails
  s.valid = s.taken && (cs > 0.0f);
  s.g = (2.0f * cs) * k;
  return s;
}

}  // namespace light
}  // namespace rt
