// contract_host_check.cpp — a plain C++ program (no device) over the two statements of the numerics contract: the host half of
// rtpt_math.hpp, the text the kernels compile, against oracle/det_math.h, function by function and bit for bit (two NaNs count
// as equal: their sign and payload are the processor's).  Built with -ffp-contract=off -mfma and the address, undefined-behaviour
// and float-cast-overflow sanitizers: f2i, sincos2pi and exp_ convert floats to integers, and a conversion outside int's range
// stops the program.  Operands, per function:
//   * ordinary (magnitudes 2^-8 .. 2^8), arbitrary bits, all operands scaled by 2^-70 .. 2^-60 and by 2^60 .. 2^66,
//   * +-0, +-inf, NaN, 2^-149 and the largest finite in each operand position,
//   * equal and nearly parallel vectors and the zero vector; all 49 pairs of the specials for min/max; +-2^31 and their
//     neighbours for f2i; every exponent of the domain for sincos2pi ([0, 1]) and log_ (positive finite); the thresholds of exp_.
// `make -C csrc contract-host-check` builds and runs it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../rtpt_math.hpp"
#include "det_math.h"

using rt::f2u;
using rt::u2f;
namespace ex = rt::exact;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return static_cast<uint32_t>((g_state * 0x2545f4914f6cdd1dull) >> 32);
}
static float unit() { return static_cast<float>(rnd() >> 8) * 0x1p-24f; }  // [0, 1)
static float ordinary() {
  const float m = std::ldexp(1.0f + unit(), static_cast<int>(rnd() % 16u) - 8);
  return (rnd() & 1u) ? -m : m;
}

static const uint32_t kSpecials[7] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0x00000001u, 0x7f7fffffu};
static const char* kClass[6] = {"ordinary", "any bits", "scaled small", "scaled big", "specials", "structural"};

// k operands of item i: class i % 5 (structural operands are made by the callers); returns the class
static int operands(uint64_t i, int k, float* v) {
  const int cls = static_cast<int>(i % 5);
  const int sh = cls == 2 ? -70 + static_cast<int>(rnd() % 11u) : 60 + static_cast<int>(rnd() % 7u);
  for (int j = 0; j < k; j++) {
    if (cls == 1)
      v[j] = u2f(rnd());
    else if (cls == 2 || cls == 3)
      v[j] = std::ldexp(ordinary(), sh);
    else
      v[j] = ordinary();
  }
  if (cls == 4) {
    const uint64_t t = i / 5;
    v[t % static_cast<uint64_t>(k)] = u2f(kSpecials[(t / static_cast<uint64_t>(k)) % 7]);
  }
  return cls;
}

struct Tally {
  const char* name;
  uint64_t n = 0, bad = 0, nan = 0;
};
static uint64_t g_bad = 0;

static bool same(float a, float b, Tally& t) {
  const uint32_t x = f2u(a), y = f2u(b);
  const bool nx = (x & 0x7fffffffu) > 0x7f800000u, ny = (y & 0x7fffffffu) > 0x7f800000u;
  t.nan += ny;
  return (nx && ny) || x == y;
}
static void report(Tally& t, int cls, const float* in, int k, const float* got, const float* want, int m) {
  t.bad++;
  g_bad++;
  if (t.bad > 4) return;
  std::fprintf(stderr, "mismatch: %s (%s):", t.name, kClass[cls]);
  for (int j = 0; j < k; j++) std::fprintf(stderr, " %08x", f2u(in[j]));
  std::fprintf(stderr, " -> rtpt_math.hpp");
  for (int j = 0; j < m; j++) std::fprintf(stderr, " %08x", f2u(got[j]));
  std::fprintf(stderr, ", det_math.h");
  for (int j = 0; j < m; j++) std::fprintf(stderr, " %08x", f2u(want[j]));
  std::fprintf(stderr, "\n");
}
static void compare(Tally& t, int cls, const float* in, int k, const float* got, const float* want, int m) {
  t.n++;
  bool ok = true;
  for (int j = 0; j < m; j++) ok &= same(got[j], want[j], t);
  if (!ok) report(t, cls, in, k, got, want, m);
}
static void done(const Tally& t) {
  std::printf("contract_host_check: %-10s %9llu items, %8llu NaN words, %llu mismatches\n", t.name, static_cast<unsigned long long>(t.n),
              static_cast<unsigned long long>(t.nan), static_cast<unsigned long long>(t.bad));
}

static rt::f3 F3(const float* v) { return rt::f3{v[0], v[1], v[2]}; }
static vec3 V3(const float* v) { return v3(v[0], v[1], v[2]); }

static void check_pair(Tally& td, Tally& tc, int cls, const float* v) {
  const float gd = ex::dot(F3(v), F3(v + 3)), wd = v3_dot(V3(v), V3(v + 3));
  compare(td, cls, v, 6, &gd, &wd, 1);
  const rt::f3 c = ex::cross(F3(v), F3(v + 3));
  const vec3 o = v3_cross(V3(v), V3(v + 3));
  const float gc[3] = {c.x, c.y, c.z}, wc[3] = {o.x, o.y, o.z};
  compare(tc, cls, v, 6, gc, wc, 3);
}
static void check_single(Tally& tl, Tally& tn, int cls, const float* v) {
  const float gl = ex::length(F3(v)), wl = v3_length(V3(v));
  compare(tl, cls, v, 3, &gl, &wl, 1);
  const rt::f3 c = ex::normalize(F3(v));
  const vec3 o = v3_normalize(V3(v));
  const float gc[3] = {c.x, c.y, c.z}, wc[3] = {o.x, o.y, o.z};
  compare(tn, cls, v, 3, gc, wc, 3);
}
static void check_minmax(Tally& t, int cls, const float* v) {
  const float g[2] = {rt::glsl_min(v[0], v[1]), rt::glsl_max(v[0], v[1])}, w[2] = {dm_min(v[0], v[1]), dm_max(v[0], v[1])};
  compare(t, cls, v, 2, g, w, 2);
}
static void check_powi(Tally& t, int cls, float x) {
  static const int ns[7] = {1, 2, 3, 5, 127, 128, 255};
  for (int n : ns) {
    const float g = ex::powi(x, n), w = dm_powi(x, n);
    compare(t, cls, &x, 1, &g, &w, 1);
  }
}
static void check_f2i(Tally& t, int cls, float x) {
  const int32_t g = ex::f2i(x), w = dm_f2i(x);
  t.n++;
  if (g != w) {
    const float gf = u2f(static_cast<uint32_t>(g)), wf = u2f(static_cast<uint32_t>(w));
    report(t, cls, &x, 1, &gf, &wf, 1);
  }
}
static void check_sincos(Tally& t, int cls, float u) {  // u in [0, 1]
  float g[2], w[2];
  ex::sincos2pi(u, g[0], g[1]);
  dm_sincos2pi(u, &w[0], &w[1]);
  compare(t, cls, &u, 1, g, w, 2);
}
static void check_log(Tally& t, int cls, float x) {  // finite x > 0
  const float g = ex::log_(x), w = dm_log(x);
  compare(t, cls, &x, 1, &g, &w, 1);
}
static void check_exp(Tally& t, int cls, float x) {
  const float g = ex::exp_(x), w = dm_exp(x);
  compare(t, cls, &x, 1, &g, &w, 1);
}

int main() {
  const uint64_t N = 1u << 20;
  Tally t_dot{"dot"}, t_cross{"cross"}, t_len{"length"}, t_norm{"normalize"}, t_mm{"min/max"}, t_powi{"powi"}, t_f2i{"f2i"},
      t_sc{"sincos2pi"}, t_log{"log_"}, t_exp{"exp_"}, t_rng{"rng_skip"};
  float v[6];

  // vectors
  for (uint64_t i = 0; i < N; i++) check_pair(t_dot, t_cross, operands(i, 6, v), v);
  for (uint64_t i = 0; i < N / 4; i++) {
    operands(5 * i, 3, v);  // an ordinary a
    const int kind = static_cast<int>(i % 6);
    for (int j = 0; j < 3; j++)
      v[3 + j] = kind == 0 ? v[j] : kind == 1 ? v[j] * (1.0f + 0x1p-12f) : kind == 2 ? 0.0f : kind == 3 ? -v[j] : kind == 4 ? -0.0f : v[j] * 0x1p-75f;
    if (kind == 5)
      for (int j = 0; j < 3; j++) v[j] *= 0x1p-75f;
    check_pair(t_dot, t_cross, 5, v);
    float s[6] = {v[3], v[4], v[5], v[0], v[1], v[2]};
    check_pair(t_dot, t_cross, 5, s);
  }
  for (uint64_t i = 0; i < N; i++) check_single(t_len, t_norm, operands(i, 3, v), v);
  for (uint64_t i = 0; i < N / 4; i++) {
    operands(5 * i, 3, v);
    const int kind = static_cast<int>(i % 6);
    static const int sh[6] = {0, 0, -75, -138, 64, 56};
    for (int j = 0; j < 3; j++) v[j] = kind == 0 ? 0.0f : kind == 1 ? (j == static_cast<int>(i / 6 % 3) ? v[j] : -0.0f) : std::ldexp(v[j], sh[kind]);
    check_single(t_len, t_norm, 5, v);
  }

  // min/max: the classes, all 49 pairs of the specials, neighbours
  for (uint64_t i = 0; i < N; i++) check_minmax(t_mm, operands(i, 2, v), v);
  for (uint32_t a : kSpecials)
    for (uint32_t b : kSpecials) {
      v[0] = u2f(a), v[1] = u2f(b);
      check_minmax(t_mm, 5, v);
    }
  for (uint64_t i = 0; i < 4096; i++) {
    const uint32_t b = f2u(ordinary());
    const uint32_t other[4] = {b, b + 1u, b - 1u, b ^ 0x80000000u};
    for (uint32_t o : other) {
      v[0] = u2f(b), v[1] = u2f(o);
      check_minmax(t_mm, 5, v);
      v[0] = u2f(o), v[1] = u2f(b);
      check_minmax(t_mm, 5, v);
    }
  }

  // powi: the classes with every n, then the listed bases
  for (uint64_t i = 0; i < N / 4; i++) {
    const int cls = operands(i, 1, v);
    check_powi(t_powi, cls, v[0]);
  }
  {
    const float xs[] = {0.0f, -0.0f, 1.0f, u2f(0x3f800001u), u2f(0x3f7fffffu), -1.0f, -1.5f, -0.99f, -2.0f, 0x1p-20f, 0x1p-75f, -0x1p-75f, 1e-30f,
                        0.5f, 2.0f, 1.0000119f, 0.9999f, INFINITY, -INFINITY, NAN, 0x1p-149f, 3.4e38f, 1.4142135f, -1.4142135f};
    for (float x : xs) check_powi(t_powi, 5, x);
    for (uint64_t i = 0; i < 65536; i++) check_powi(t_powi, 5, std::ldexp((rnd() & 1u) ? -1.0f - unit() : 1.0f + unit(), static_cast<int>(rnd() % 3u) - 1));
  }

  // f2i: the classes, +-2^31 and the floats next to them, the range of int
  for (uint64_t i = 0; i < N; i++) {
    const int cls = operands(i, 1, v);
    check_f2i(t_f2i, cls, v[0]);
  }
  {
    const uint32_t p31 = 0x4f000000u;
    const uint32_t edge[] = {p31, p31 | 0x80000000u, p31 + 1u, p31 - 1u, (p31 + 1u) | 0x80000000u, (p31 - 1u) | 0x80000000u, 0x3f7fffffu, 0xbf7fffffu,
                             0x00000000u, 0x80000000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u, 0x7f800000u, 0xff800000u, 0x3f800000u, 0xbf800000u,
                             0x4b800000u, 0xcb800000u, 0x4affffffu, 0x00000001u, 0x80000001u, 0x7f7fffffu, 0xff7fffffu, 0x4f800000u, 0x5f000000u};
    for (uint32_t e : edge) check_f2i(t_f2i, 5, u2f(e));
    for (uint64_t i = 0; i < N; i++) check_f2i(t_f2i, 5, std::ldexp((rnd() & 1u) ? -1.0f - unit() : 1.0f + unit(), static_cast<int>(rnd() % 34u)));
  }

  // sincos2pi on its domain [0, 1]: uniform, any pattern of the domain, tiny, up against 1, every exponent, k/8 +- 1 ulp
  for (uint64_t i = 0; i < N; i++) {
    const int kind = static_cast<int>(i % 4);
    const float u = kind == 0 ? unit() : kind == 1 ? u2f(rnd() % 0x3f800001u) : kind == 2 ? std::ldexp(1.0f + unit(), -70 + static_cast<int>(rnd() % 11u))
                                                                                          : 1.0f - std::ldexp(unit(), -static_cast<int>(rnd() % 16u));
    check_sincos(t_sc, kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? 2 : 5, u);
  }
  for (uint32_t e = 0; e < 127; e++)
    for (uint32_t m : {0x000000u, 0x000001u, 0x400000u, 0x555555u, 0x7fffffu}) check_sincos(t_sc, 5, u2f((e << 23) | m));
  for (int k = 0; k <= 8; k++) {
    const uint32_t b = f2u(static_cast<float>(k) / 8.0f);
    check_sincos(t_sc, 5, u2f(b));
    if (k < 8) check_sincos(t_sc, 5, u2f(b + 1u));
    if (k > 0) check_sincos(t_sc, 5, u2f(b - 1u));
  }
  check_sincos(t_sc, 4, -0.0f);
  check_sincos(t_sc, 4, 0x1p-149f);

  // log_ on every positive finite pattern class: any such pattern, every exponent field
  for (uint64_t i = 0; i < N; i++) check_log(t_log, 1, u2f(rnd() % 0x7f7fffffu + 1u));
  for (uint64_t i = 0; i < N; i++) check_log(t_log, 0, std::fabs(ordinary()));
  for (uint32_t e = 0; e < 255; e++)
    for (uint32_t m : {0x000000u, 0x000001u, 0x3504f3u, 0x3504f4u, 0x400000u, 0x7fffffu})
      if ((e << 23) | m) check_log(t_log, 5, u2f((e << 23) | m));

  // exp_ on the whole line
  for (uint64_t i = 0; i < N; i++) {
    const int cls = operands(i, 1, v);
    check_exp(t_exp, cls, v[0]);
  }
  for (uint64_t i = 0; i < N; i++) check_exp(t_exp, 5, (unit() - 0.5f) * 200.0f);
  for (uint32_t b : {f2u(-87.0f), f2u(88.0f)})
    for (uint32_t d : {0u, 1u, 0xffffffffu}) check_exp(t_exp, 5, u2f(b + d));
  for (uint32_t b : kSpecials) check_exp(t_exp, 4, u2f(b));

  // rng_skip is rng_next's step of the state
  for (uint64_t i = 0; i < N; i++) {
    uint32_t a = rnd(), b = a;
    (void)ex::rng_next(a);
    ex::rng_skip(b);
    t_rng.n++;
    if (a != b) {
      t_rng.bad++;
      g_bad++;
    }
  }

  for (const Tally* t : {&t_dot, &t_cross, &t_len, &t_norm, &t_mm, &t_powi, &t_f2i, &t_sc, &t_log, &t_exp, &t_rng}) done(*t);
  if (g_bad) return 1;
  std::printf("contract_host_check: ok\n");
  return 0;
}
