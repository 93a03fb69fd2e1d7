// texture.hpp — the albedo-texture sampler (rtpt_scene_set_textures).  ONE definition, used by every kernel that shades a hit
// (kernels.hip: shade_segment) and by the sampler self test (rtpt_selftest_texture).  Not reference behaviour: the reference
// has no textures.  No image instructions, no LDS: plain 16-byte global loads of RGBA32F texels.
//
// The arithmetic, stated so that numpy float32 reproduces it bit for bit (the build has -ffp-contract=off: only the fmas
// written here fuse; tests/texture_scenes.py restates it):
//   uv from barycentrics   uv = fmaf(b2, uv2, fmaf(b1, uv1, b0 * uv0))               per component
//   repeat wrap            s = u - floorf(u)                                          in [0, 1]: 1.0 for a tiny negative u
//   nearest                i = min((int)floorf(s * W), W - 1)                         (s == 1.0 belongs to the last texel)
//   bilinear               x = s * W - 0.5f, x0 = floorf(x), f = x - x0; taps (int)x0 and (int)x0 + 1 wrapped into [0, W);
//                          rows likewise; lerp(a, b, f) = a + f * (b - a), along x for both rows, then along y.
//                          Equal taps return the tap exactly (b - a == 0).
// Bounds: every index below is in [0, W) x [0, H) for ANY bit pattern of (u, v) — a NaN takes s = 0 — and the host refuses
// every descriptor whose rectangle [first_texel, first_texel + W * H) leaves the atlas (api_scene.hip), so no lane can read
// outside it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

struct TexDesc {  // == rtpt_texture
  uint32_t width, height, first_texel, flags;
};
constexpr uint32_t kTexNearest = 0x1u;  // RTPT_TEX_NEAREST

// The per-triangle record of the BASE mesh, two float4 (instance i, triangle t reads record t, like the materials):
//   t0 = (u0, v0, u1, v1)   t1 = (u2, v2, texture index + 1 as bits or 0: untextured, spare)
namespace tex {

__device__ __forceinline__ float wrap01(float u) {
  const float s = u - __builtin_floorf(u);
  return s >= 0.0f ? s : 0.0f;  // s is in [0, 1] for every finite u; NaN (an infinite u) reads texel 0
}

__device__ __forceinline__ float interp_uv(float b0, float b1, float b2, float c0, float c1, float c2) {
  return __builtin_fmaf(b2, c2, __builtin_fmaf(b1, c1, b0 * c0));
}

__device__ __forceinline__ float lerp(float a, float b, float f) { return a + f * (b - a); }
__device__ __forceinline__ float4 lerp4(float4 a, float4 b, float f) {
  return make_float4(lerp(a.x, b.x, f), lerp(a.y, b.y, f), lerp(a.z, b.z, f), lerp(a.w, b.w, f));
}

// the two taps of one axis of the bilinear filter and the weight of the second
__device__ __forceinline__ void taps(float s, int n, int& i0, int& i1, float& f) {
  const float x = s * static_cast<float>(n) - 0.5f;  // in [-0.5, n - 0.5]
  const float x0 = __builtin_floorf(x);              // in [-1, n - 1]
  f = x - x0;
  const int k = static_cast<int>(x0);
  i0 = k < 0 ? n - 1 : (k > n - 1 ? n - 1 : k);  // the second test never fires; it bounds the index whatever x is
  i1 = k + 1 > n - 1 ? 0 : (k + 1 < 0 ? 0 : k + 1);
}

__device__ __forceinline__ float4 sample(const TexDesc d, const float4* __restrict__ texels, float u, float v) {
  const int W = static_cast<int>(d.width), H = static_cast<int>(d.height);
  const float4* t = texels + d.first_texel;
  const float su = wrap01(u), sv = wrap01(v);
  if (d.flags & kTexNearest) {
    int i = static_cast<int>(__builtin_floorf(su * static_cast<float>(W)));
    int j = static_cast<int>(__builtin_floorf(sv * static_cast<float>(H)));
    i = i > W - 1 ? W - 1 : (i < 0 ? 0 : i);
    j = j > H - 1 ? H - 1 : (j < 0 ? 0 : j);
    return t[static_cast<uint32_t>(j) * d.width + static_cast<uint32_t>(i)];
  }
  int i0, i1, j0, j1;
  float fx, fy;
  taps(su, W, i0, i1, fx);
  taps(sv, H, j0, j1, fy);
  const uint32_t r0 = static_cast<uint32_t>(j0) * d.width, r1 = static_cast<uint32_t>(j1) * d.width;
  const float4 a = t[r0 + static_cast<uint32_t>(i0)], b = t[r0 + static_cast<uint32_t>(i1)];
  const float4 c = t[r1 + static_cast<uint32_t>(i0)], e = t[r1 + static_cast<uint32_t>(i1)];
  return lerp4(lerp4(a, b, fx), lerp4(c, e, fx), fy);
}

}  // namespace tex
}  // namespace rt
