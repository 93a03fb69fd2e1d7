/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.
 *
 * glsl_compat.hpp — the subset of GLSL 4.60 that the reference's three compute shaders use, as C++ over a scalar type
 * `Real`, so that the shader text itself (after prep.py's syntactic pre-pass) is compiled and executed on the CPU.
 * Nothing of the reference is in this file: it is the language the shaders are written in, not the shaders.
 *
 * Two arithmetics, selected by REFSHADER_REAL (float | double); the translation unit is compiled once per arithmetic:
 *   R32  Real = float, built with -ffp-contract=off and no fast-math.  +,-,*,/ on scalars and vectors are the literal
 *        operator-by-operator reading (unfused, left to right).  The builtins the numerics contract defines
 *        (oracle/det_math.h: dot, cross, length, normalize, sqrt, log, exp, integer pow, float->int, min/max wording,
 *        sincos(2 pi u)) use the contract's definitions.
 *   R64  Real = double with libm: the plain high-precision reading.  Floating literals keep their GLSL value (a GLSL
 *        `0.7` IS the binary32 0.7), integers stay 32-bit with wrap-around in both.
 */
#ifndef REFSHADER_GLSL_COMPAT_HPP
#define REFSHADER_GLSL_COMPAT_HPP

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

namespace dmc {  // the contract, verbatim (its C `vec3` stays inside this namespace)
#include "../det_math.h"
}

#ifndef REFSHADER_REAL
#error "compile with -DREFSHADER_REAL=float or -DREFSHADER_REAL=double"
#endif

/* the two arithmetics live in one library: every name below is in namespace glsl_f32 or glsl_f64 */
#ifndef REFSHADER_SUF
#error "compile with -DREFSHADER_SUF=f32 or -DREFSHADER_SUF=f64"
#endif
#define REFSHADER_CAT2(a, b) a##b
#define REFSHADER_CAT(a, b) REFSHADER_CAT2(a, b)
#define glsl REFSHADER_CAT(glsl_, REFSHADER_SUF)

namespace glsl {

typedef REFSHADER_REAL Real;
typedef uint32_t uint;
/* a GLSL floating literal is a 32-bit float: prep.py wraps every one as RL(<literal>) */
#define RL(x) (::glsl::Real(x##f))
#define RLF(x) (::glsl::Real(x))  // literal that already carries the f suffix

/* ---------------------------------------------------------------- scalar builtins */
inline float rs_sqrt(float x) { return dmc::dm_sqrt(x); }
inline double rs_sqrt(double x) { return std::sqrt(x); }
inline float rs_log(float x) { return dmc::dm_log(x); }
inline double rs_log(double x) { return std::log(x); }
inline float rs_exp(float x) { return dmc::dm_exp(x); }
inline double rs_exp(double x) { return std::exp(x); }
inline float rs_tan(float x) { return ::tanf(x); }
inline double rs_tan(double x) { return std::tan(x); }
/* pow: the contract defines pow(x, n) for integer n >= 1 (the only use: n = 128) */
inline float rs_pow(float x, float n) {
  if (n >= 1.0f && n <= 1024.0f && n == (float)(int)n) return dmc::dm_powi(x, (int)n);
  return ::powf(x, n);
}
inline double rs_pow(double x, double n) { return std::pow(x, n); }
inline int rs_f2i(float x) { return dmc::dm_f2i(x); }
inline int rs_f2i(double x) {
  if (x != x) return 0;
  if (x >= 2147483648.0) return 2147483647;
  if (x <= -2147483648.0) return -2147483647 - 1;
  return (int)x;
}
/* trig hook (prep.py HOOKS): theta = 2*k_pi*u.  R32 evaluates the contract's sincos(2 pi u) from u; R64 evaluates
 * cos/sin of theta as the text writes it. */
inline float rs_cos_hook(float theta, float u) { float s, c; (void)theta; dmc::dm_sincos2pi(u, &s, &c); return c; }
inline float rs_sin_hook(float theta, float u) { float s, c; (void)theta; dmc::dm_sincos2pi(u, &s, &c); return s; }
inline double rs_cos_hook(double theta, double u) { (void)u; return std::cos(theta); }
inline double rs_sin_hook(double theta, double u) { (void)u; return std::sin(theta); }

inline Real sqrt(Real x) { return rs_sqrt(x); }
inline Real log(Real x) { return rs_log(x); }
inline Real exp(Real x) { return rs_exp(x); }
inline Real tan(Real x) { return rs_tan(x); }
inline Real pow(Real x, Real n) { return rs_pow(x, n); }
/* GLSL spec wording: min(x,y) = y < x ? y : x;  max(x,y) = x < y ? y : x */
inline Real min(Real x, Real y) { return (y < x) ? y : x; }
inline Real max(Real x, Real y) { return (x < y) ? y : x; }
inline Real clamp(Real x, Real lo, Real hi) { return min(max(x, lo), hi); }
inline Real length(Real x) { return x < 0 ? -x : x; }  // |x|: length() of a one-component vector

/* ---------------------------------------------------------------- vectors */
struct ivec2;
struct uvec2 {
  uint x, y;
};
struct uvec3 {
  union {
    struct { uint x, y, z; };
    uvec2 xy;
  };
};

struct ivec2 {
  int x, y;
  ivec2() = default;
  explicit ivec2(int s) : x(s), y(s) {}
  /* mixed int/uint components convert like GLSL's constructors: modulo 2^32 */
  template <class A, class B> ivec2(A a, B b) : x((int)(uint)a), y((int)(uint)b) {}
  explicit ivec2(uvec2 u) : x((int)u.x), y((int)u.y) {}
  explicit ivec2(const struct vec2& v);
};
inline ivec2 operator-(ivec2 a, int s) { return ivec2(a.x - s, a.y - s); }
inline int clampi(int v, int lo, int hi) { int t = v < lo ? lo : v; return t > hi ? hi : t; }  // min(max(x,lo),hi)
inline ivec2 clamp(ivec2 v, ivec2 lo, ivec2 hi) { return ivec2(clampi(v.x, lo.x, hi.x), clampi(v.y, lo.y, hi.y)); }

struct vec2 {
  Real x, y;
  vec2() = default;
  explicit vec2(Real s) : x(s), y(s) {}
  vec2(Real a, Real b) : x(a), y(b) {}
  vec2(ivec2 i) : x((Real)i.x), y((Real)i.y) {}  // implicit int -> float conversion of GLSL
};
inline ivec2::ivec2(const vec2& v) : x(rs_f2i(v.x)), y(rs_f2i(v.y)) {}
inline vec2 operator+(vec2 a, vec2 b) { return vec2(a.x + b.x, a.y + b.y); }
inline vec2 operator*(vec2 a, vec2 b) { return vec2(a.x * b.x, a.y * b.y); }
inline vec2 operator*(vec2 a, Real s) { return vec2(a.x * s, a.y * s); }
inline vec2 operator*(Real s, vec2 a) { return vec2(s * a.x, s * a.y); }
inline vec2 operator+(vec2 a, Real s) { return vec2(a.x + s, a.y + s); }

struct vec3;
struct swz3 {  // .rgb / .xyz of a vec3: converts back to a vec3
  Real v[3];
  inline operator vec3() const;
};
struct vec3 {
  union {
    struct { Real x, y, z; };
    struct { Real r, g, b; };
    vec2 xy;
    swz3 rgb;
    swz3 xyz;
  };
  vec3() = default;
  explicit vec3(Real s) : x(s), y(s), z(s) {}
  vec3(Real a, Real b_, Real c) : x(a), y(b_), z(c) {}
  vec3(Real a, vec2 bc) : x(a), y(bc.x), z(bc.y) {}
  vec3& operator*=(vec3 o) { x *= o.x; y *= o.y; z *= o.z; return *this; }
  vec3& operator+=(vec3 o) { x += o.x; y += o.y; z += o.z; return *this; }
  vec3& operator+=(Real s) { x += s; y += s; z += s; return *this; }
};
inline swz3::operator vec3() const { return vec3(v[0], v[1], v[2]); }
inline vec3 operator+(vec3 a, vec3 b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(vec3 a, vec3 b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(vec3 a, vec3 b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator/(vec3 a, vec3 b) { return vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline vec3 operator*(vec3 a, Real s) { return vec3(a.x * s, a.y * s, a.z * s); }
inline vec3 operator*(Real s, vec3 a) { return vec3(s * a.x, s * a.y, s * a.z); }
inline vec3 operator/(vec3 a, Real s) { return vec3(a.x / s, a.y / s, a.z / s); }
inline vec3 operator-(vec3 a) { return vec3(-a.x, -a.y, -a.z); }

struct vec4 {
  union {
    struct { Real x, y, z, w; };
    struct { Real r, g, b, a; };
    vec3 xyz;
    vec3 rgb;
  };
  vec4() = default;
  vec4(Real a_, Real b_, Real c, Real d) : x(a_), y(b_), z(c), w(d) {}
  vec4(vec3 v, Real d) : x(v.x), y(v.y), z(v.z), w(d) {}
};

/* dot / cross / length / normalize: the contract's sequences in R32, the textbook ones in R64 */
#define REFSHADER_IS_F32 (sizeof(::glsl::Real) == 4)
inline Real dot(vec3 a, vec3 b) {
  if (REFSHADER_IS_F32) return (Real)dmc::dm_fma((float)a.z, (float)b.z, dmc::dm_fma((float)a.y, (float)b.y, (float)a.x * (float)b.x));
  return a.x * b.x + a.y * b.y + a.z * b.z;
}
inline vec3 cross(vec3 a, vec3 b) {
  if (REFSHADER_IS_F32)
    return vec3((Real)dmc::dm_fma((float)a.y, (float)b.z, -((float)a.z * (float)b.y)), (Real)dmc::dm_fma((float)a.z, (float)b.x, -((float)a.x * (float)b.z)),
                (Real)dmc::dm_fma((float)a.x, (float)b.y, -((float)a.y * (float)b.x)));
  return vec3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
inline Real length(vec3 a) { return sqrt(dot(a, a)); }
inline vec3 normalize(vec3 a) {
  if (REFSHADER_IS_F32) { Real inv = Real(1) / sqrt(dot(a, a)); return a * inv; }
  return a / sqrt(dot(a, a));
}
/* spec definitions, literally */
inline vec3 mix(vec3 x, vec3 y, Real a) { return x * (Real(1) - a) + y * a; }
inline vec3 faceforward(vec3 N, vec3 I, vec3 Nref) { return (dot(Nref, I) < Real(0)) ? N : -N; }
inline vec3 reflect(vec3 I, vec3 N) { return I - Real(2) * dot(N, I) * N; }

/* mat4, column-major; products are the spec's linear-algebra sums, left to right */
struct mat4 {
  Real c[4][4];  // c[column][row]
};
inline mat4 operator*(const mat4& A, const mat4& B) {
  mat4 R;
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 4; i++) R.c[j][i] = A.c[0][i] * B.c[j][0] + A.c[1][i] * B.c[j][1] + A.c[2][i] * B.c[j][2] + A.c[3][i] * B.c[j][3];
  return R;
}
inline vec4 operator*(const mat4& A, vec4 v) {
  Real o[4];
  for (int i = 0; i < 4; i++) o[i] = A.c[0][i] * v.x + A.c[1][i] * v.y + A.c[2][i] * v.z + A.c[3][i] * v.w;
  return vec4(o[0], o[1], o[2], o[3]);
}

/* ---------------------------------------------------------------- images */
/* One binding.  Loads read `load` (a pre-pass snapshot when the host separates them, D1), stores go to `store`.
 * Out-of-image loads return 0 and out-of-image stores are dropped (robust image access, D2).  `chan` planes of Real.
 * The host may ask for the coordinate of every load to be recorded (last_load). */
struct image2D {
  int w = 0, h = 0, chan = 4;
  const Real* load = nullptr;
  Real* store = nullptr;
  mutable ivec2 last_load = ivec2(0, 0);
  mutable int n_loads = 0;
};
inline ivec2 imageSize(const image2D& im) { return ivec2(im.w, im.h); }
inline vec4 imageLoad(const image2D& im, ivec2 p) {
  im.last_load = p;
  im.n_loads++;
  vec4 r(Real(0), Real(0), Real(0), Real(0));
  if (p.x < 0 || p.y < 0 || p.x >= im.w || p.y >= im.h || !im.load) return r;
  const Real* s = im.load + (size_t)im.chan * ((size_t)p.y * im.w + p.x);
  r.x = s[0];
  if (im.chan > 1) { r.y = s[1]; r.z = s[2]; r.w = s[3]; }
  return r;
}
inline void imageStore(image2D& im, ivec2 p, vec4 v) {
  if (p.x < 0 || p.y < 0 || p.x >= im.w || p.y >= im.h || !im.store) return;
  Real* d = im.store + (size_t)im.chan * ((size_t)p.y * im.w + p.x);
  d[0] = v.x;
  if (im.chan > 1) { d[1] = v.y; d[2] = v.z; d[3] = v.w; }
}

/* ---------------------------------------------------------------- ray query */
/* The traversal is the driver's black box, not shader text: the host supplies closest hit (D4) through `tlas`. */
struct rayQueryEXT {
  int prim = -1;  // committed primitive index, -1 = none
  Real t = 0, b1 = 0, b2 = 0;
};
struct RayRecord {
  uint32_t id;  // committed primitive id + 1, 0 = none
  Real t;
  vec3 o, d;
};
struct accelerationStructureEXT {
  const float* tris = nullptr;  // n x 9 world-space
  uint32_t n = 0;
  std::vector<RayRecord>* record = nullptr;  // one entry per query of the current invocation
  uint32_t (*closest)(const accelerationStructureEXT&, vec3 o, vec3 d, Real tmax, Real* t, Real* b1, Real* b2) = nullptr;
};
enum { gl_RayFlagsOpaqueEXT = 1, gl_RayQueryCommittedIntersectionNoneEXT = 0, gl_RayQueryCommittedIntersectionTriangleEXT = 1 };
inline void rayQueryInitializeEXT(rayQueryEXT& q, const accelerationStructureEXT& as, int flags, int mask, vec3 o, Real tmin, vec3 d, Real tmax) {
  (void)flags; (void)mask; (void)tmin;  // opaque, all instances, tmin 0: what the host's closest hit implements
  Real t = 0, b1 = 0, b2 = 0;
  uint32_t id = as.closest(as, o, d, tmax, &t, &b1, &b2);
  q.prim = (int)id - 1;
  q.t = t; q.b1 = b1; q.b2 = b2;
  if (as.record) as.record->push_back(RayRecord{id, id ? t : Real(0), o, d});
}
inline bool rayQueryProceedEXT(rayQueryEXT&) { return false; }  // opaque geometry: nothing to confirm
inline int rayQueryGetIntersectionTypeEXT(const rayQueryEXT& q, bool) { return q.prim >= 0 ? gl_RayQueryCommittedIntersectionTriangleEXT : gl_RayQueryCommittedIntersectionNoneEXT; }
inline int rayQueryGetIntersectionPrimitiveIndexEXT(const rayQueryEXT& q, bool) { return q.prim; }
inline vec2 rayQueryGetIntersectionBarycentricsEXT(const rayQueryEXT& q, bool) { return vec2(q.b1, q.b2); }

}  // namespace glsl
#endif
