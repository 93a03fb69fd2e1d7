// selftest_kernels.hip — the kernels behind rtpt_selftest_* (api_selftest.hip) and their launchers: the functions the frame
// kernels call, one per launch, on operands the tests choose.  A translation unit of its own: nothing here runs in a frame, and
// an edit here does not recompile the frame kernels (kernels.hip).
#include "closest_hit.hpp"
#include "dielectric.hpp"
#include "light_sample.hpp"
#include "select.hpp"
#include "shade_segment.hpp"
#include "specular.hpp"
#include "texture.hpp"

namespace rt {
namespace {

__global__ void k_selftest_math(int op, const float* in, float* out, size_t n) {
  size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x = in[i], r = 0.f, s, c;
  switch (op) {
    case 0: r = exact::log_(x); break;
    case 1: exact::sincos2pi(x, s, c); r = s; break;
    case 2: exact::sincos2pi(x, s, c); r = c; break;
    case 3: r = exact::sqrt_(x); break;
    case 4: r = exact::rcp_(x); break;
    case 5: r = fast::exp_(x); break;
    case 6: { uint32_t st = f2u(x); r = exact::rng_next(st); break; }
    case 7: r = exact::exp_(x); break;
    default: break;
  }
  out[i] = r;
}

// every binary32 pattern through exact::sqrt_ (op 3) / exact::rcp_ (op 4) against hipcc's IEEE expansion of the same
// operation: out[0] = patterns whose results differ in any bit, out[1..4] = the first few of them
__global__ void k_selftest_exhaustive(int op, unsigned long long* out) {
  const uint64_t base = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) * 64u;
  for (uint32_t k = 0; k < 64u; k++) {
    const uint32_t b = static_cast<uint32_t>(base + k);
    const float x = u2f(b);
    const float got = op == 3 ? exact::sqrt_(x) : exact::rcp_(x);
    const float want = op == 3 ? __builtin_sqrtf(x) : 1.0f / x;
    if (f2u(got) != f2u(want)) {
      const unsigned long long n = atomicAdd(out, 1ull);
      if (n < 4) out[1 + n] = b;
    }
  }
}

// exact::div_ against hipcc's division.  mode 0: slice `pass` of 256 of the enumeration of all 2^23 x 2^23 significand pairs
// (thread = one b, 2^15 values of a); mode 1: 2^33 operand pairs of arbitrary bits (every exponent, sign, zero, infinity,
// NaN and denormal class gets hit: the long path and the range test) from a counter-based generator; mode 2: mode 1's pairs through
// exact::quotient_positive(a, b) against a / b > 0.0f (mode 3 is k_selftest_div2 below)
__global__ void k_selftest_div(int mode, uint32_t pass, unsigned long long* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // 0 .. 2^23-1
  unsigned bad = 0;
  uint32_t fa = 0, fb = 0;
  if (mode == 0) {
    const float b = u2f(0x3f800000u | t);
    for (uint32_t i = 0; i < (1u << 15); i++) {
      const uint32_t ma = (pass << 15) + i;
      const float a = u2f(0x3f800000u | ma);
      if (f2u(exact::div_(a, b)) != f2u(a / b)) { bad++; fa = f2u(a); fb = f2u(b); }
    }
  } else {
    uint32_t st = exact::rng_seed(t, pass, 0x9e3779b9u, 1u);
    for (uint32_t i = 0; i < (1u << 10); i++) {
      st = st * 747796405u + 2891336453u;
      uint32_t ua = ((st >> ((st >> 28) + 4u)) ^ st) * 277803737u;
      ua ^= ua >> 22;
      st = st * 747796405u + 2891336453u;
      uint32_t ub = ((st >> ((st >> 28) + 4u)) ^ st) * 277803737u;
      ub ^= ub >> 22;
      if (i & 1u) ub = (ub & 0x807fffffu) | (ua & 0x7f800000u);  // every other pair: same exponent (quotients near 1)
      const float a = u2f(ua), b = u2f(ub);
      if (mode == 2) {
        if (exact::quotient_positive(a, b) != (a / b > 0.0f)) { bad++; fa = ua; fb = ub; }
        continue;
      }
      const uint32_t got = f2u(exact::div_(a, b)), want = f2u(a / b);
      if (got != want && !((got & 0x7fffffffu) > 0x7f800000u && (want & 0x7fffffffu) > 0x7f800000u)) { bad++; fa = ua; fb = ub; }
    }
  }
  if (bad && atomicAdd(out, static_cast<unsigned long long>(bad)) == 0) {
    out[1] = fa;
    out[2] = fb;
  }
}

// rtpt_selftest_div mode 3: mode 1's generator with a third operand through exact::div2_(a0, a1, b) against hipcc's a0 / b and a1 / b,
// mode 1's NaN rule for either quotient (each counts; out[1] is the numerator of the offending one).  A kernel of its own so that
// k_selftest_div stays the kernel it was.
__global__ void k_selftest_div2(uint32_t pass, unsigned long long* out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // 0 .. 2^23-1
  unsigned bad = 0;
  uint32_t fa = 0, fb = 0;
  uint32_t st = exact::rng_seed(t, pass, 0x9e3779b9u, 1u);
  auto draw = [&]() {
    st = st * 747796405u + 2891336453u;
    uint32_t u = ((st >> ((st >> 28) + 4u)) ^ st) * 277803737u;
    return u ^ (u >> 22);
  };
  auto differ = [](uint32_t got, uint32_t want) {
    return got != want && !((got & 0x7fffffffu) > 0x7f800000u && (want & 0x7fffffffu) > 0x7f800000u);
  };
  for (uint32_t i = 0; i < (1u << 10); i++) {
    const uint32_t ua = draw();
    uint32_t ub = draw(), uc = draw();
    if (i & 1u) ub = (ub & 0x807fffffu) | (ua & 0x7f800000u);  // every other triple: b in a0's binade (quotients near 1)
    if (i & 2u) uc = (uc & 0x807fffffu) | (ua & 0x7f800000u);  // ... and a1 in it in half of either kind
    const float a0 = u2f(ua), a1 = u2f(uc), b = u2f(ub);
    float q0, q1;
    exact::div2_(a0, a1, b, q0, q1);
    if (differ(f2u(q0), f2u(a0 / b))) { bad++; fa = ua; fb = ub; }
    if (differ(f2u(q1), f2u(a1 / b))) { bad++; fa = uc; fb = ub; }
  }
  if (bad && atomicAdd(out, static_cast<unsigned long long>(bad)) == 0) {
    out[1] = fa;
    out[2] = fb;
  }
}

// One numerics-contract function per launch on raw 32-bit words, one thread per item (rtpt_selftest_contract; the table of fn
// and its words per item is kContractWords, kernels.hpp).  Every case calls the function the frame kernels call, compiled
// with the same macros (RTPT_DIV_*, RTPT_TRACE_ITEMS: closest_hit.hpp), so a change to any of them is a change to what runs here.
__global__ void k_selftest_contract(int fn, uint32_t n_in, uint32_t n_out, const uint32_t* in, uint32_t* out, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* w = in + i * n_in;  // n_in, n_out: kContractWords[fn], which sized both arrays
  uint32_t* r = out + i * n_out;
  auto F = [&](int k) { return u2f(w[k]); };
  auto V = [&](int k) { return f3{u2f(w[k]), u2f(w[k + 1]), u2f(w[k + 2])}; };
  auto put3 = [&](int k, f3 v) { r[k] = f2u(v.x); r[k + 1] = f2u(v.y); r[k + 2] = f2u(v.z); };
  switch (fn) {
    case 0: r[0] = f2u(exact::dot(V(0), V(3))); break;
    case 1: put3(0, exact::cross(V(0), V(3))); break;
    case 2: r[0] = f2u(exact::length(V(0))); break;
    case 3: put3(0, exact::normalize(V(0))); break;
    case 4: r[0] = f2u(exact::powi(F(0), static_cast<int>(w[1]))); break;
    case 5: r[0] = static_cast<uint32_t>(exact::f2i(F(0))); break;
    case 6: r[0] = f2u(glsl_min(F(0), F(1))); r[1] = f2u(glsl_max(F(0), F(1))); break;
    case 7: r[0] = exact::rng_seed(w[0], w[1], w[2], w[3]); break;
    case 8: {
      uint32_t st = w[0], sk = w[0];
      const float f = exact::rng_next(st);
      exact::rng_skip(sk);
      r[0] = st; r[1] = f2u(f); r[2] = sk;
      break;
    }
    case 9: { float s, c; exact::sincos2pi(F(0), s, c); r[0] = f2u(s); r[1] = f2u(c); break; }
    case 10: r[0] = f2u(exact::log_(F(0))); break;
    case 11: r[0] = f2u(exact::exp_(F(0))); break;
    case 12: {
      float M[16];
      for (int k = 0; k < 16; k++) M[k] = F(k);
      for (int k = 0; k < 4; k++) r[k] = f2u(exact::mat_row_point(M, k, V(16)));
      break;
    }
    case 13: r[0] = f2u(exact::div_(F(0), F(1))); break;
    case 14: { float q0, q1; exact::div2_(F(0), F(1), F(2), q0, q1); r[0] = f2u(q0); r[1] = f2u(q1); break; }
    case 15: r[0] = f2u(tri_area(V(0), V(3), V(6))); break;
    case 16: put3(0, bary_coords(V(0), V(3), V(6), V(9))); break;
    case 17: put3(0, bary_coords_at(V(0), V(3), V(6), V(9), F(12))); break;
    case 18: put3(0, bary_mix(V(0), V(3), V(6), V(9))); break;
    case 19: {
      // W, H, PVprev[16], id, wp[3], the id's three lut_prev cells, x, y.  The cells stand at 3 * id of a table of four
      // triangles (id & 3: the generators stay below 4), the rest of it zero
      float M[16];
      for (int k = 0; k < 16; k++) M[k] = F(2 + k);
      const uint32_t id = w[18] & 3u;
      float4 lut[12];
      for (int k = 0; k < 12; k++) lut[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int k = 0; k < 3; k++) lut[3 * id + k] = make_float4(F(22 + 4 * k), F(23 + 4 * k), F(24 + 4 * k), F(25 + 4 * k));
      int px, py;
      reproject_pixel(static_cast<int>(w[0]), static_cast<int>(w[1]), M, id, V(19), lut, static_cast<int>(w[34]), static_cast<int>(w[35]), px, py);
      r[0] = static_cast<uint32_t>(px); r[1] = static_cast<uint32_t>(py);
      break;
    }
    case 20: { const float radius = F(9); r[0] = ray_hits_light(V(0), V(3), V(6), radius * radius) ? 1u : 0u; break; }  // r2: api_passes.hip
    case 21: put3(0, sky_color(V(0))); break;
    case 22: {
      const HitRec h{0.f, 1u, F(0), F(1), F(2)};
      float b0, b1, b2;
      hit_barycentrics<true>(h, b0, b1, b2);
      put3(0, f3{b0, b1, b2});
      hit_barycentrics<false>(h, b0, b1, b2);
      put3(3, f3{b0, b1, b2});
      break;
    }
    default: break;
  }
}

// specular.hpp's bounce, one case per thread: in = d, n, u1, u2, g; out = d', 1.0f if absorbed else 0.0f (rtpt_selftest_bounce)
__global__ void k_selftest_bounce(const float* in, float* out, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* w = in + 9 * i;
  bool absorbed;
  const f3 dn = spec::bounce(ld3(w + 3), ld3(w), w[6], w[7], w[8], &absorbed);
  out[4 * i] = dn.x; out[4 * i + 1] = dn.y; out[4 * i + 2] = dn.z;
  out[4 * i + 3] = absorbed ? 1.0f : 0.0f;
}

// dielectric.hpp's interface, one case per thread: in = d, n, u1, u2, ior; out = d', 1.0f if transmitted else 0.0f, F
// (rtpt_selftest_refract)
__global__ void k_selftest_refract(const float* in, float* out, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* w = in + 9 * i;
  bool transmitted;
  float fresnel;
  const f3 dn = diel::refract(ld3(w + 3), ld3(w), w[6], w[8], &transmitted, &fresnel);
  out[5 * i] = dn.x; out[5 * i + 1] = dn.y; out[5 * i + 2] = dn.z;
  out[5 * i + 3] = transmitted ? 1.0f : 0.0f;
  out[5 * i + 4] = fresnel;
}

// light_sample.hpp's pick and sample, one case per thread: in = v0, v1, v2, x, nf, u_l, u_a, u_b, L (19 words); out = y, wd, g,
// 1.0f if valid else 0.0f, the picked entry (9 words).  The light's normal as k_scene_prepare stores it (rtpt_selftest_light_sample)
__global__ void k_selftest_light_sample(const uint32_t* in, uint32_t* out, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* w = reinterpret_cast<const float*>(in + 19 * i);
  const f3 v0 = ld3(w), v1 = ld3(w + 3), v2 = ld3(w + 6);
  const uint32_t L = in[19 * i + 18];
  const f3 nl = exact::normalize(exact::cross(v1 - v0, v2 - v0));  // raytrace.comp.glsl:150
  const light::Sample s = light::sample(v0, v1, v2, nl, ld3(w + 9), ld3(w + 12), w[16], w[17], static_cast<float>(L));
  uint32_t* r = out + 9 * i;
  r[0] = f2u(s.y.x); r[1] = f2u(s.y.y); r[2] = f2u(s.y.z);
  r[3] = f2u(s.wd.x); r[4] = f2u(s.wd.y); r[5] = f2u(s.wd.z);
  r[6] = f2u(s.g);
  r[7] = f2u(s.valid ? 1.0f : 0.0f);
  r[8] = light::pick(w[15], L);
}

// light_sample.hpp's sphere_sample, one case per thread: in = x, nf, c, r2, u_c, u_p (12 words); out = wd, g, 1.0f if taken else
// 0.0f, 1.0f if valid else 0.0f (6 words); wd and g as 0 where the sample is not taken (rtpt_selftest_sphere_sample)
__global__ void k_selftest_sphere_sample(const uint32_t* in, uint32_t* out, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* w = reinterpret_cast<const float*>(in + 12 * i);
  const light::SphereSample s = light::sphere_sample(ld3(w), ld3(w + 3), ld3(w + 6), w[9], w[10], w[11]);
  uint32_t* r = out + 6 * i;
  r[0] = s.taken ? f2u(s.wd.x) : 0u; r[1] = s.taken ? f2u(s.wd.y) : 0u; r[2] = s.taken ? f2u(s.wd.z) : 0u;
  r[3] = s.taken ? f2u(s.g) : 0u;
  r[4] = f2u(s.taken ? 1.0f : 0.0f);
  r[5] = f2u(s.valid ? 1.0f : 0.0f);
}

// light_sample.hpp's weights of RTPT_FLAG_EXT_NEE_MIS, one case per thread, by the functions the tracing kernels call: in = v0, v1, v2
// of the hit emitter, o, d, the hit's b1, b2, cb, inv_p (19 floats of a 20-word case; word 19 is not read); out = g_hit,
// wb(g_hit), g_hit * m(g_hit).  The emitter's normal as k_scene_prepare stores it; b0 as hit_barycentrics forms it
// (rtpt_selftest_mis_weight)
__global__ void k_selftest_mis_weight(const float* in, float* out, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* w = in + 20 * i;
  const f3 v0 = ld3(w), v1 = ld3(w + 3), v2 = ld3(w + 6);
  const f3 nl = exact::normalize(exact::cross(v1 - v0, v2 - v0));  // raytrace.comp.glsl:150
  const float b1 = w[15], b2 = w[16];
  const float b0 = 1.0f - b1 - b2;
  const float g = light::hit_weight(v0, v1, v2, nl, ld3(w + 9), ld3(w + 12), b0, b1, b2, w[17], w[18]);
  out[3 * i] = g;
  out[3 * i + 1] = light::mis_bounce(g);
  out[3 * i + 2] = g * light::mis_light(g);
}

// shading_normal.hpp's rules 1 to 7 and its three side tests, one case per thread, by the functions shade_segment calls: in = 36 words,
// n0, n1, n2, (b1, b2), the three cof rows, ng, d, d', wd, ray_offset (33 floats; words 33 to 35 are not read); out = 8 words: smooth as
// 1.0f / 0.0f, ns (ng where the hit is not smooth), absorbed(d') and sample_side(wd) as 1.0f / 0.0f, the dielectric's offset, 0.
// b0 as hit_barycentrics forms it (rtpt_selftest_shading_normal)
__global__ void k_selftest_shading_normal(const float* in, float* out, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* w = in + 36 * i;
  const float b1 = w[9], b2 = w[10];
  const float b0 = 1.0f - b1 - b2;
  const f3 ng = ld3(w + 20), d = ld3(w + 23);
  f3 ns;
  const bool smooth = nrm::interpolate(ld3(w), ld3(w + 3), ld3(w + 6), b0, b1, b2, ld3(w + 11), ld3(w + 14), ld3(w + 17), &ns);
  ns = smooth ? nrm::orient(ns, ng, d) : ng;
  float* r = out + 8 * i;
  r[0] = smooth ? 1.0f : 0.0f;
  r[1] = ns.x;
  r[2] = ns.y;
  r[3] = ns.z;
  r[4] = nrm::absorbed(ld3(w + 26), ng) ? 1.0f : 0.0f;
  r[5] = nrm::sample_side(ld3(w + 29), ng) ? 1.0f : 0.0f;
  r[6] = nrm::dielectric_offset(ld3(w + 26), ng, w[32]);
  r[7] = 0.0f;
}

// rtpt_light::find (light_list_host.hpp) of k queries on the ascending list ids[0, n): the entry's index, n where the list does not
// hold the id (rtpt_selftest_light_find)
__global__ void k_selftest_light_find(const uint32_t* ids, uint32_t n, const uint32_t* queries, size_t k, uint32_t* index_out) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= k) return;
  index_out[i] = rtpt_light::find(ids, n, queries[i]);
}

template <int BVH>
__global__ __launch_bounds__(kThreads) void k_selftest_trace(SceneView sc, const float* rays, size_t n, float tmax,
                                                             uint32_t* out_id, float* out_t) {
  extern __shared__ uint32_t stack[];  // BVH: stack_depth x 256 entries (dynamic); unused otherwise
  size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  f3 o = ld3(rays + 6 * i), d = ld3(rays + 6 * i + 3);
  HitRec h{tmax, 0u, 0.f, 0.f, 1.f};
  closest_hit<BVH>(sc, o, d, h, stack, threadIdx.x);
  out_id[i] = h.id1;
  if (out_t) out_t[i] = h.id1 ? h.t : 0.0f;
}

// env::color (env.hpp) of the context's environment map at arbitrary directions (rtpt_selftest_environment)
__global__ void k_selftest_environment(EnvView envmap, const float* dirs, size_t n, float* rgb) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const f3 c = env::color(envmap, f3{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]});
  rgb[3 * i] = c.x;
  rgb[3 * i + 1] = c.y;
  rgb[3 * i + 2] = c.z;
}

// the sampler of texture.hpp at arbitrary uv (rtpt_selftest_texture)
__global__ void k_selftest_texture(const TexDesc* desc, const float4* texels, const float* uv, size_t n, float4* out) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = tex::sample(*desc, texels, uv[2 * i], uv[2 * i + 1]);
}

// the sampler at an explicit level (rtpt_selftest_texture_lod); lv: the texture's row of the level table
__global__ void k_selftest_texture_lod(const TexDesc* desc, const uint32_t* lv, const float4* texels, const float* uv, const float* lod,
                                       size_t n, float4* out) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = tex::sample_lod(*desc, lv, texels, uv[2 * i], uv[2 * i + 1], lod[i]);
}

// k_selftest_trace, then the level shade_segment would sample the hit's texture at (rtpt_selftest_texture_footprint)
template <int BVH>
__global__ __launch_bounds__(kThreads) void k_selftest_footprint(SceneView sc, TexView tex, const float* rays, size_t n, float tmax,
                                                                 uint32_t primary, float slope, int frame_h, uint32_t* out_id,
                                                                 float* out_lod) {
  extern __shared__ uint32_t stack[];
  size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  f3 o = ld3(rays + 6 * i), d = ld3(rays + 6 * i + 3);
  HitRec h{tmax, 0u, 0.f, 0.f, 1.f};
  closest_hit<BVH>(sc, o, d, h, stack, threadIdx.x);
  out_id[i] = h.id1;
  float lambda = 0.0f;
  if (h.id1 && tex.records && tex.levels) {
    const float4* tr = tex.records + 2 * static_cast<size_t>((h.id1 - 1) % sc.n_base_tris);
    const float4 t0 = tr[0], t1 = tr[1];
    const uint32_t ti = __float_as_uint(t1.z);
    if (ti) {
      const float4* s = sc.shade + 3 * static_cast<size_t>(h.id1 - 1);
      const TexDesc td = tex.desc[ti - 1];
      lambda = hit_texture_lod(td, s[0], s[1], s[2], t0, t1, h.t, d, primary != 0, slope, frame_h, tex.bounce_spread);
      uint32_t L = tex.levels[kTexLevelRow * static_cast<size_t>(ti - 1) + kTexLevelRowCount];  // the clamp of tex::sample_lod
      L = L < 1u ? 1u : (L > kTexLevelRowCount ? kTexLevelRowCount : L);
      const float top = static_cast<float>(L - 1u);
      lambda = lambda > 0.0f ? lambda : 0.0f;
      lambda = lambda < top ? lambda : top;
    }
  }
  out_lod[i] = lambda;
}

}  // namespace

void launch_selftest_math(int op, const float* in, float* out, size_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_math, dim3((n + 255) / 256), dim3(256), 0, s, op, in, out, n);
}
void launch_selftest_exhaustive(int op, unsigned long long* out, hipStream_t s) {
  hipLaunchKernelGGL(k_selftest_exhaustive, dim3((1u << 26) / 256u), dim3(256), 0, s, op, out);  // 2^26 threads x 64 patterns
}
void launch_selftest_div(int mode, uint32_t pass, unsigned long long* out, hipStream_t s) {
  if (mode == 3) {
    hipLaunchKernelGGL(k_selftest_div2, dim3((1u << 23) / 256u), dim3(256), 0, s, pass, out);
    return;
  }
  hipLaunchKernelGGL(k_selftest_div, dim3((1u << 23) / 256u), dim3(256), 0, s, mode, pass, out);
}
void launch_selftest_contract(int fn, const uint32_t* in, uint32_t* out, size_t n, hipStream_t s) {
  if (!n || fn < 0 || fn >= kContractFns) return;
  hipLaunchKernelGGL(k_selftest_contract, dim3((n + 255) / 256), dim3(256), 0, s, fn, kContractWords[fn][0], kContractWords[fn][1], in, out, n);
}
void launch_selftest_bounce(const float* in, float* out, size_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_bounce, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
}
void launch_selftest_light_sample(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_light_sample, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
}
void launch_selftest_sphere_sample(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_sphere_sample, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
}
void launch_selftest_mis_weight(const float* in, float* out, size_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_mis_weight, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
}
void launch_selftest_shading_normal(const float* in, float* out, size_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_shading_normal, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
}
void launch_selftest_light_find(const uint32_t* ids, uint32_t n, const uint32_t* queries, size_t k, uint32_t* index_out, hipStream_t s) {
  if (!k) return;
  hipLaunchKernelGGL(k_selftest_light_find, dim3(static_cast<uint32_t>((k + 255) / 256)), dim3(256), 0, s, ids, n, queries, k, index_out);
}
void launch_selftest_refract(const float* in, float* out, size_t n, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_refract, dim3((n + 255) / 256), dim3(256), 0, s, in, out, n);
}
void launch_selftest_environment(const EnvView& envmap, const float* dirs, size_t n, float* rgb_out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_environment, dim3((n + 255) / 256), dim3(256), 0, s, envmap, dirs, n, rgb_out);
}
void launch_selftest_texture(const TexDesc* desc, const float4* texels, const float* uv, size_t n, float4* out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_texture, dim3((n + 255) / 256), dim3(256), 0, s, desc, texels, uv, n, out);
}
void launch_selftest_texture_lod(const TexDesc* desc, const uint32_t* lv, const float4* texels, const float* uv, const float* lod, size_t n,
                                 float4* out, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_selftest_texture_lod, dim3((n + 255) / 256), dim3(256), 0, s, desc, lv, texels, uv, lod, n, out);
}
void launch_selftest_footprint(const SceneView& scene, const TexView& tex, const float* rays, size_t n, float tmax, bool primary, float slope,
                               int frame_h, uint32_t* out_id, float* out_lod, hipStream_t s) {
  if (!n) return;
  dim3 grid((n + kThreads - 1) / kThreads), block(kThreads);
  with_mode<3>(scene_mode(scene), [&](auto mode) {
    constexpr int M = decltype(mode)::value;
    hipLaunchKernelGGL(k_selftest_footprint<M>, grid, block, M ? scene.stack_lds * kThreads * 4 : 0, s, scene, tex, rays, n, tmax,
                       primary ? 1u : 0u, slope, frame_h, out_id, out_lod);
  });
}
void launch_selftest_trace(const SceneView& scene, const float* rays, size_t n, float tmax, uint32_t* out_id,
                           float* out_t, hipStream_t s) {
  if (!n) return;
  dim3 grid((n + kThreads - 1) / kThreads), block(kThreads);
  with_mode<3>(scene_mode(scene), [&](auto mode) {
    constexpr int M = decltype(mode)::value;
    hipLaunchKernelGGL(k_selftest_trace<M>, grid, block, M ? scene.stack_lds * kThreads * 4 : 0, s, scene, rays, n, tmax, out_id, out_t);
  });
}

}  // namespace rt
