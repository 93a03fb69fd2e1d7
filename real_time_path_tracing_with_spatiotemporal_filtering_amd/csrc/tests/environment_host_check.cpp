// environment_host_check.cpp — the host-only code of the environment map (env_host.hpp: the argument checks of rtpt_set_environment,
// the decode and the lat-long conversion of rtpt_util_environment_from_latlong) in a program of its own, built with the address and
// undefined-behaviour sanitizers (make environment-host-check).  Every array is an allocation of exactly its length, so a read or a
// write one element outside is a report.  No device, no HIP.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../env_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static std::vector<float> map_of(uint32_t n, float value) { return std::vector<float>(4 * static_cast<size_t>(n) * n, value); }

static void check_refusals() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, one[3] = {1, 1, 1};
  for (uint32_t n : {1u, 2u, 3u, 8u, 64u}) {
    std::vector<float> m = map_of(n, 0.5f);
    CHECK(!rtpt_env::check_environment(m.data(), n, 0, nullptr, nullptr, 0));
    CHECK(!rtpt_env::check_environment(m.data(), n, RTPT_TEX_NEAREST, eye, one, 0));
    CHECK(!rtpt_env::check_environment(m.data(), n, 0, eye, one, RTPT_FLAG_FORCE_BVH));
    CHECK(rtpt_env::check_environment(m.data(), n, 0, eye, one, RTPT_FLAG_NO_PATH_COMPACTION));
    for (uint32_t flags : {0x2u, 0x10u, 0x20u, 0x11u, 0x80000000u}) CHECK(rtpt_env::check_environment(m.data(), n, flags, eye, one, 0));
    for (float bad : {inf, -inf, nan}) {
      for (size_t at : {static_cast<size_t>(0), m.size() / 2, m.size() - 1}) {  // first, middle and last float, alpha included
        std::vector<float> t = m;
        t[at] = bad;
        CHECK(rtpt_env::check_environment(t.data(), n, 0, nullptr, nullptr, 0));
      }
      for (int k = 0; k < 9; k++) {
        float r[9];
        for (int i = 0; i < 9; i++) r[i] = i == k ? bad : eye[i];
        CHECK(rtpt_env::check_environment(m.data(), n, 0, r, nullptr, 0));
      }
      for (int k = 0; k < 3; k++) {
        float s[3] = {1, 1, 1};
        s[k] = bad;
        CHECK(rtpt_env::check_environment(m.data(), n, 0, nullptr, s, 0));
      }
    }
    // values are not a reason while they are finite: HDR, negative, denormal, the largest float
    std::vector<float> t = m;
    t[0] = 1e4f, t[1] = -3.0f, t[2] = 1e-45f, t[3] = std::numeric_limits<float>::max();
    CHECK(!rtpt_env::check_environment(t.data(), n, 0, nullptr, nullptr, 0));
  }
  // the size is refused before a texel is read: one float stands for a map it would not fit
  float lone = 0.0f;
  CHECK(rtpt_env::check_environment(&lone, 4097, 0, nullptr, nullptr, 0));
  CHECK(rtpt_env::check_environment(&lone, 0xFFFFFFFFu, 0, nullptr, nullptr, 0));
}

static void check_decode() {
  // the centre of the square is +y, its corners -y, the middles of its edges the horizontal axes; every direction has unit length
  double d[3];
  rtpt_env::decode(0.5, 0.5, d);
  CHECK(d[0] == 0.0 && d[1] == 1.0 && d[2] == 0.0);
  for (double U : {0.0, 1.0})
    for (double V : {0.0, 1.0}) {
      rtpt_env::decode(U, V, d);
      CHECK(std::fabs(d[0]) == 0.0 && d[1] == -1.0 && std::fabs(d[2]) == 0.0);
    }
  rtpt_env::decode(1.0, 0.5, d);
  CHECK(d[0] == 1.0 && std::fabs(d[1]) == 0.0 && d[2] == 0.0);
  rtpt_env::decode(0.5, 0.0, d);
  CHECK(d[0] == 0.0 && std::fabs(d[1]) == 0.0 && d[2] == -1.0);
  for (int i = 0; i <= 64; i++)
    for (int j = 0; j <= 64; j++) {
      rtpt_env::decode(i / 64.0, j / 64.0, d);
      CHECK(std::fabs(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - 1.0) < 1e-14);
      // and back: the L1 projection of the direction is the point
      const double s = std::fabs(d[0]) + std::fabs(d[1]) + std::fabs(d[2]);
      double u = d[0] / s, v = d[2] / s;
      if (d[1] < 0.0) {
        const double p = u, q = v;
        u = std::copysign(1.0 - std::fabs(q), p);
        v = std::copysign(1.0 - std::fabs(p), q);
      }
      const bool edge = i == 0 || i == 64 || j == 0 || j == 64 || i + j == 32 || i + j == 96 || i - j == 32 || j - i == 32;  // folds: either sheet
      if (!edge) CHECK(std::fabs(0.5 * u + 0.5 - i / 64.0) < 1e-14 && std::fabs(0.5 * v + 0.5 - j / 64.0) < 1e-14);
    }
}

static void check_latlong() {
  // refusals first, with nothing read or written
  float px[3] = {1, 2, 3}, out4[4] = {0, 0, 0, 0};
  CHECK(rtpt_env::from_latlong(nullptr, 1, 1, 1, out4));
  CHECK(rtpt_env::from_latlong(px, 1, 1, 1, nullptr));
  CHECK(rtpt_env::from_latlong(px, 0, 1, 1, out4));
  CHECK(rtpt_env::from_latlong(px, 1, 0, 1, out4));
  CHECK(rtpt_env::from_latlong(px, 65537, 1, 1, out4));
  CHECK(rtpt_env::from_latlong(px, 1, 1, 0, out4));
  CHECK(rtpt_env::from_latlong(px, 1, 1, 4097, out4));
  CHECK(out4[0] == 0.0f && out4[3] == 0.0f);
  // a one-pixel image is a constant map of any size
  for (uint32_t n : {1u, 2u, 3u, 8u, 64u}) {
    std::vector<float> out = map_of(n, -1.0f);
    CHECK(!rtpt_env::from_latlong(px, 1, 1, n, out.data()));
    for (size_t t = 0; t < out.size() / 4; t++) CHECK(out[4 * t] == 1.0f && out[4 * t + 1] == 2.0f && out[4 * t + 2] == 3.0f && out[4 * t + 3] == 1.0f);
  }
  // images of odd and even sizes, one row, one column: every index stays inside (the sanitizer's business), a constant image stays
  // constant, and an image that depends on its row only gives texels that depend on the direction's y only
  for (uint32_t w : {1u, 2u, 5u, 16u})
    for (uint32_t h : {1u, 2u, 7u, 16u}) {
      std::vector<float> flat(3 * static_cast<size_t>(w) * h, 0.25f), rows(3 * static_cast<size_t>(w) * h);
      for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++)
          for (int c = 0; c < 3; c++) rows[3 * (static_cast<size_t>(y) * w + x) + c] = static_cast<float>(y + 1) * (c + 1);
      for (uint32_t n : {1u, 3u, 8u}) {
        std::vector<float> a = map_of(n, -1.0f), b = map_of(n, -1.0f);
        CHECK(!rtpt_env::from_latlong(flat.data(), w, h, n, a.data()));
        CHECK(!rtpt_env::from_latlong(rows.data(), w, h, n, b.data()));
        for (uint32_t j = 0; j < n; j++)
          for (uint32_t i = 0; i < n; i++) {
            const size_t t = 4 * (static_cast<size_t>(j) * n + i);
            CHECK(a[t] == 0.25f && a[t + 1] == 0.25f && a[t + 2] == 0.25f && a[t + 3] == 1.0f);
            double d[3];
            rtpt_env::decode((i + 0.5) / n, (j + 0.5) / n, d);
            const double y = std::acos(d[1]) / 3.14159265358979323846 * h - 0.5;
            const double lo = std::floor(y) < 0 ? 0 : std::floor(y), hi = std::floor(y) + 1 > h - 1 ? h - 1 : std::floor(y) + 1;
            const double want = (lo + 1) + (y - std::floor(y)) * (hi - lo);
            CHECK(std::fabs(b[t] - want) <= 1e-6 * want && std::fabs(b[t + 1] - 2 * want) <= 2e-6 * want);
          }
      }
    }
  // a NaN pixel is not refused here (rtpt_set_environment refuses the map)
  float bad[3] = {std::numeric_limits<float>::quiet_NaN(), 1, 1};
  CHECK(!rtpt_env::from_latlong(bad, 1, 1, 1, out4));
  CHECK(std::isnan(out4[0]) && rtpt_env::check_environment(out4, 1, 0, nullptr, nullptr, 0));
}

int main() {
  check_refusals();
  check_decode();
  check_latlong();
  if (failures) {
    std::printf("environment_host_check: %d FAILED\n", failures);
    return 1;
  }
  std::printf("environment_host_check: ok\n");
  return 0;
}
