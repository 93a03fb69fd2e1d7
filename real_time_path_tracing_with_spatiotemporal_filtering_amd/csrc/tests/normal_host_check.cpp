// normal_host_check.cpp — the host side of smooth shading in a program of its own under the address and undefined-behaviour
// sanitizers (make normal-host-check; runs on the CPU, needs neither hipcc nor a device): rtpt_scene_set_normals' argument checks
// and record packing (normal_host.hpp) on arrays that are allocations of exactly their length, and the cofactor function and the
// rules (shading_normal.hpp, compiled as plain C++: HIP's headers are only included) on hostile matrices and operands.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../normal_host.hpp"
#include "../shading_normal.hpp"

#define CHECK(x)                                                                 \
  do {                                                                           \
    if (!(x)) {                                                                  \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof u);
  return u;
}

static void check_arguments() {
  const float one[9] = {0, 0, 1, 0, 0, 1, 0, 0, 1};
  CHECK(rtpt_nrm::check_normals(one, 1, 1, 0) == nullptr);
  CHECK(rtpt_nrm::check_normals(one, 1, 2, 0) != nullptr);                                // not the upload's base count
  CHECK(rtpt_nrm::check_normals(one, 0, 1, 0) != nullptr);
  CHECK(rtpt_nrm::check_normals(nullptr, 1, 1, 0) != nullptr);                            // NULL with a count
  CHECK(rtpt_nrm::check_normals(one, 1, 1, RTPT_FLAG_NO_PATH_COMPACTION) != nullptr);     // that A/B flag has no smooth kernels
  CHECK(rtpt_nrm::check_normals(one, 1, 1, ~static_cast<uint32_t>(RTPT_FLAG_NO_PATH_COMPACTION)) == nullptr);
}

static void check_packing() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  for (uint32_t n : {1u, 2u, 7u, 1000u}) {
    // allocations of exactly the lengths the call reads and writes: one float or word beyond either is the sanitizer's
    std::unique_ptr<float[]> nrm(new float[9 * static_cast<size_t>(n)]);
    std::unique_ptr<uint32_t[]> smooth(new uint32_t[n]);
    std::unique_ptr<float[]> rec(new float[rtpt_nrm::kRecordFloats * static_cast<size_t>(n)]);
    for (size_t i = 0; i < 9 * static_cast<size_t>(n); i++) nrm[i] = i % 13 == 0 ? nan : (i % 17 == 0 ? -inf : (i % 5 == 0 ? -0.0f : static_cast<float>(i) * 0.25f));
    for (uint32_t t = 0; t < n; t++) smooth[t] = t % 3 == 0 ? 0u : (t % 3 == 1 ? 1u : 0xFFFFFFFFu);
    for (int pass = 0; pass < 2; pass++) {
      std::memset(rec.get(), 0x5A, rtpt_nrm::kRecordFloats * static_cast<size_t>(n) * sizeof(float));
      rtpt_nrm::pack_records(nrm.get(), pass ? nullptr : smooth.get(), n, rec.get());
      for (uint32_t t = 0; t < n; t++)
        for (int k = 0; k < 3; k++) {
          const float* r = rec.get() + 12 * static_cast<size_t>(t) + 4 * k;
          CHECK(!std::memcmp(r, nrm.get() + 9 * static_cast<size_t>(t) + 3 * k, 12));      // bit for bit, NaN and -0 included
          const uint32_t want = k == 0 ? ((pass || smooth[t]) ? 1u : 0u) : 0u;
          CHECK(bits(r[3]) == want);
        }
    }
  }
  rtpt_nrm::pack_records(nullptr, nullptr, 0, nullptr);  // nothing is read or written for no triangle
}

static double det3(const double* l) {
  return l[0] * (l[4] * l[8] - l[5] * l[7]) - l[1] * (l[3] * l[8] - l[5] * l[6]) + l[2] * (l[3] * l[7] - l[4] * l[6]);
}

static void check_cofactor() {
  const float id[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  float c[9];
  rt::nrm::cofactor(id, c);
  CHECK(!std::memcmp(c, id, sizeof id));
  const float mirror[9] = {-1, 0, 0, 0, 1, 0, 0, 0, 1}, want_mirror[9] = {1, 0, 0, 0, -1, 0, 0, 0, -1};
  rt::nrm::cofactor(mirror, c);
  for (int i = 0; i < 9; i++) CHECK(c[i] == want_mirror[i]);
  const float zero[9] = {};
  rt::nrm::cofactor(zero, c);
  for (int i = 0; i < 9; i++) CHECK(c[i] == 0.0f);
  // C^T L = det(L) I in double from the float entries, for seeded matrices over twelve decades, singular ones among them
  uint32_t s = 12345u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return static_cast<float>(static_cast<int32_t>(s >> 8) % 2001 - 1000) * 1e-3f;
  };
  for (int it = 0; it < 2000; it++) {
    float l[9];
    const float scale = std::pow(10.0f, static_cast<float>(it % 13 - 6));
    for (float& v : l) v = rnd() * scale;
    if (it % 7 == 0) std::memcpy(l + 6, l, 12);  // two equal rows
    rt::nrm::cofactor(l, c);
    double ld[9], big = 0;
    for (int i = 0; i < 9; i++) ld[i] = l[i], big = std::fmax(big, std::fabs(ld[i]));
    const double det = det3(ld);
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) {
        double sum = 0;
        for (int k = 0; k < 3; k++) sum += static_cast<double>(c[3 * k + a]) * ld[3 * k + b];
        // each cofactor is within 2^-23 of its two products' magnitudes: 3 of them times an entry
        CHECK(std::fabs(sum - (a == b ? det : 0.0)) <= 3 * 2 * 1.2e-7 * big * big * big + 1e-300);
      }
  }
  // the rows as the device table holds them, with and without a transform; the model is column-major, the transform row-major
  float model[16] = {}, rows[12], rows2[12];
  for (int i = 0; i < 4; i++) model[5 * i] = 1.0f;
  rt::nrm::cof_rows(model, nullptr, rows);
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 4; k++) CHECK(rows[4 * r + k] == (r == k ? 1.0f : 0.0f));
  const float xf[12] = {2, 0, 0, 5, 0, 3, 0, 6, 0, 0, 4, 7};  // a scale with a translation: C = diag(12, 8, 6), the translation unread
  rt::nrm::cof_rows(model, xf, rows);
  const float want[12] = {12, 0, 0, 0, 0, 8, 0, 0, 0, 0, 6, 0};
  for (int i = 0; i < 12; i++) CHECK(rows[i] == want[i]);
  model[0] = 0.0f, model[1] = 1.0f, model[4] = -1.0f, model[5] = 0.0f;  // a quarter turn about z, column-major: x -> y, y -> -x
  float l[9];
  rt::nrm::linear_part(model, xf, l);
  const float want_l[9] = {0, -3, 0, 2, 0, 0, 0, 0, 4};
  for (int i = 0; i < 9; i++) CHECK(l[i] == want_l[i]);
  rt::nrm::cof_rows(model, xf, rows2);
  CHECK(rows2[1] == -8.0f && rows2[4] == 12.0f && rows2[10] == 6.0f && rows2[3] == 0.0f && rows2[7] == 0.0f && rows2[11] == 0.0f);
}

static void check_rules() {
  using rt::f3;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const f3 x{1, 0, 0}, y{0, 1, 0}, z{0, 0, 1};
  f3 ns;
  CHECK(rt::nrm::interpolate(z, z, z, 0.25f, 0.25f, 0.5f, x, y, z, &ns) && ns.x == 0.0f && ns.y == 0.0f && ns.z == 1.0f);
  CHECK(!rt::nrm::interpolate(f3{0, 0, 0}, f3{0, 0, 0}, f3{0, 0, 0}, 0.25f, 0.25f, 0.5f, x, y, z, &ns));   // zero: rule 4
  CHECK(!rt::nrm::interpolate(z, f3{nan, 0, 0}, z, 0.25f, 0.25f, 0.5f, x, y, z, &ns));                      // NaN
  CHECK(!rt::nrm::interpolate(z, f3{0, 0, -1}, x, 0.5f, 0.5f, 0.0f, x, y, z, &ns));                         // n0 = -n1 on their edge
  CHECK(!rt::nrm::interpolate(z, z, z, 0.25f, 0.25f, 0.5f, f3{0, 0, 0}, f3{0, 0, 0}, f3{0, 0, 0}, &ns));    // a singular pose
  CHECK(rt::nrm::interpolate(f3{0, 0, 1e15f}, f3{0, 0, 1e15f}, f3{0, 0, 1e15f}, 0.25f, 0.25f, 0.5f, x, y, z, &ns) && ns.z == 1.0f);  // any length
  const f3 d{0, 0, -1};
  f3 o = rt::nrm::orient(f3{0, 0, -1}, z, d);  // rule 6: turned to ng's side
  CHECK(o.z == 1.0f);
  o = rt::nrm::orient(f3{1, 0, 0}, z, d);      // rule 7: perpendicular to d does not face it
  CHECK(o.x == 0.0f && o.z == 1.0f);
  o = rt::nrm::orient(f3{nan, 0, 0}, z, d);    // (not reached behind rule 4; still ng)
  CHECK(o.z == 1.0f);
  CHECK(rt::nrm::absorbed(f3{1, 0, 0}, z) && rt::nrm::absorbed(f3{0, 0, -1}, z) && !rt::nrm::absorbed(f3{0, 0, 1e-30f}, z) && rt::nrm::absorbed(f3{nan, 0, 0}, z));
  CHECK(!rt::nrm::sample_side(f3{1, 0, 0}, z) && rt::nrm::sample_side(f3{0, 0, 1}, z) && !rt::nrm::sample_side(f3{nan, 0, 0}, z));
  CHECK(rt::nrm::dielectric_offset(f3{0, 0, -1}, z, 1e-4f) == -1e-4f && rt::nrm::dielectric_offset(f3{0, 0, 1}, z, 1e-4f) == 1e-4f);
  CHECK(rt::nrm::dielectric_offset(f3{1, 0, 0}, z, 1e-4f) == 1e-4f && rt::nrm::dielectric_offset(f3{nan, 0, 0}, z, 1e-4f) == 1e-4f);
}

int main() {
  check_arguments();
  check_packing();
  check_cofactor();
  check_rules();
  std::puts("normal_host_check: ok");
  return 0;
}
