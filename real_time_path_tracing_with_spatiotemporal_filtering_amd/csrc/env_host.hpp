// env_host.hpp — the host side of the environment map (rtpt_set_environment, rtpt_util_environment_from_latlong), free of HIP so
// that a plain C++ program can exercise it under a sanitizer (csrc/tests/environment_host_check.cpp): the checks the call applies
// before anything reaches the device, and the conversion of a lat-long image to the octahedral map.  The lookup's rules E1 to E6 are
// env.hpp's.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rtpt.h"

namespace rtpt_env {

constexpr uint32_t kMaxSize = 4096;  // n x n texels of 16 bytes: at most 256 MB, and an index times n far below 2^32

// Everything rtpt_set_environment refuses, decided on arguments alone.  NULL: the arguments are fine.  Not for the dropping call
// (texels NULL or n 0).  No kernel can index outside the map: that is decided here.
inline const char* check_environment(const float* texels_rgba, uint32_t n, uint32_t flags, const float* rotation, const float* scale,
                                     uint32_t ctx_flags) {
  if (ctx_flags & RTPT_FLAG_NO_PATH_COMPACTION) return "a context with RTPT_FLAG_NO_PATH_COMPACTION has no kernels that read an environment map";
  if (n > kMaxSize) return "an environment map is at most 4096 x 4096 texels";
  if (flags & ~static_cast<uint32_t>(RTPT_TEX_NEAREST)) return "unknown environment flag (RTPT_TEX_NEAREST is the only one)";
  if (rotation)
    for (int i = 0; i < 9; i++)
      if (!std::isfinite(rotation[i])) return "a rotation entry is not finite";
  if (scale)
    for (int i = 0; i < 3; i++)
      if (!std::isfinite(scale[i])) return "a scale is not finite";
  const size_t count = 4 * static_cast<size_t>(n) * n;
  for (size_t i = 0; i < count; i++)
    if (!std::isfinite(texels_rgba[i])) return "a texel is not finite";
  return nullptr;
}

// The direction of the point (U, V) of the octahedral square, E5, E4 and E3 inverted in double and normalised: u = 2U - 1, v = 2V - 1;
// |u| + |v| <= 1 is the upper sheet, (p, q) = (u, v); else the lower one, |p| = 1 - |v| with u's sign, |q| = 1 - |u| with v's;
// e = (p, +-(1 - |p| - |q|), q) / its length.
inline void decode(double U, double V, double d[3]) {
  const double u = 2.0 * U - 1.0, v = 2.0 * V - 1.0;
  double p = u, q = v, y = 1.0 - std::fabs(u) - std::fabs(v);
  if (y < 0.0) {
    p = std::copysign(1.0 - std::fabs(v), u);
    q = std::copysign(1.0 - std::fabs(u), v);
    y = -(1.0 - std::fabs(p) - std::fabs(q));
  }
  const double len = std::sqrt(p * p + y * y + q * q);
  d[0] = p / len;
  d[1] = y / len;
  d[2] = q / len;
}

// Texel (i, j) of the n x n map from the width x height lat-long image `rgb` (3 floats a pixel, row 0 at +y): the direction of the
// texel's centre, column fraction atan2(d.x, -d.z) / (2 pi) + 0.5 (the image's centre is -z), row fraction acos(d.y) / pi, ONE
// bilinear sample (x = fraction * size - 0.5; wrapped horizontally, clamped vertically), in double, rounded to binary32; alpha 1.
// Known limit: one sample per texel, no prefiltering when n is much smaller than the image.
inline void latlong_texel(const float* rgb, uint32_t width, uint32_t height, uint32_t n, uint32_t i, uint32_t j, float out[4]) {
  const double kPi = 3.14159265358979323846;
  double d[3];
  decode((i + 0.5) / n, (j + 0.5) / n, d);
  const double cf = std::atan2(d[0], -d[2]) / (2.0 * kPi) + 0.5;
  const double dy = d[1] > 1.0 ? 1.0 : (d[1] < -1.0 ? -1.0 : d[1]);
  const double rf = std::acos(dy) / kPi;
  const double x = cf * width - 0.5, y = rf * height - 0.5;
  const double x0 = std::floor(x), y0 = std::floor(y);
  const double fx = x - x0, fy = y - y0;
  const long long w = width, h = height;
  const long long i0 = ((static_cast<long long>(x0) % w) + w) % w, i1 = (i0 + 1) % w;
  long long j0 = static_cast<long long>(y0), j1 = j0 + 1;
  j0 = j0 < 0 ? 0 : (j0 > h - 1 ? h - 1 : j0);
  j1 = j1 < 0 ? 0 : (j1 > h - 1 ? h - 1 : j1);
  for (int c = 0; c < 3; c++) {
    const double a = rgb[3 * (j0 * w + i0) + c], b = rgb[3 * (j0 * w + i1) + c];
    const double e = rgb[3 * (j1 * w + i0) + c], g = rgb[3 * (j1 * w + i1) + c];
    const double top = a + fx * (b - a), bot = e + fx * (g - e);
    out[c] = static_cast<float>(top + fy * (bot - top));
  }
  out[3] = 1.0f;
}

// NULL: converted.  The image's values are not a reason (a NaN pixel gives NaN texels, which rtpt_set_environment then refuses).
inline const char* from_latlong(const float* rgb, uint32_t width, uint32_t height, uint32_t n, float* texels_rgba_out) {
  if (!rgb || !texels_rgba_out) return "NULL argument";
  if (!width || !height || width > 65536u || height > 65536u) return "a lat-long image is between 1 x 1 and 65536 x 65536 pixels";
  if (!n || n > kMaxSize) return "an environment map is between 1 x 1 and 4096 x 4096 texels";
  for (uint32_t j = 0; j < n; j++)
    for (uint32_t i = 0; i < n; i++) latlong_texel(rgb, width, height, n, i, j, texels_rgba_out + 4 * (static_cast<size_t>(j) * n + i));
  return nullptr;
}

}  // namespace rtpt_env
