// texture.hpp — the albedo-texture sampler (rtpt_scene_set_textures).  ONE definition, used by every kernel that shades a hit
// (shade_segment.hpp: shade_segment) and by the sampler self test (rtpt_selftest_texture).  Not reference behaviour: the reference
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
//
// Mip-mapping (RTPT_TEX_MIPMAP; the chain's geometry is stated in texture_host.hpp), the level a hit reads, in this order:
//   footprint width        w = t * pix, pix = (2.0f * slope) / (float)H      at segment 0 (H the FULL frame's height)
//                          w = t * kTexBounceSpread                           at every later segment (t: this segment's length)
//   world area (twice)     e1 = p1 - p0, e2 = p2 - p0, c = (e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z,
//                          e1.x * e2.y - e1.y * e2.x), aw = sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z)    p: the shade record
//   texel area (twice)     at = fabsf(((u1 - u0) * (v2 - v0) - (u2 - u0) * (v1 - v0)) * ((float)W * (float)H))
//   density                D = at / aw,   rho2 = ((w * w) * D) / (nd * nd),   nd = n . d of the unit normal and the unit ray
//   level                  lambda = 0.5f * plog2(rho2), plog2(x) = (float)(exponent of x) + (float)(mantissa bits) * 2^-23:
//                          the piecewise-linear log2, exact at powers of two, at most 0.0861 below log2 elsewhere, no
//                          transcendental instruction; lambda = 0 unless D and rho2 are positive and finite
//   clamp                  lambda = lambda > 0 ? lambda : 0 (a NaN too), then lambda < L - 1 ? lambda : L - 1
//   bilinear               l0 = (int)floorf(lambda), f = lambda - (float)l0; f == 0: the bilinear sample of level l0 alone (the
//                          other level is not loaded); else lerp4(bilinear(l0), bilinear(min(l0 + 1, L - 1)), f)
//   nearest                the nearest texel of level (int)floorf(lambda + 0.5f)
// each level sampled by `sample` itself, as a texture of its own dimensions max(1, W >> l), max(1, H >> l).  Bounds: l is clamped to
// [0, L - 1] and L to [1, 17] whatever lambda's bits are, and the host's level table (texture_host.hpp: build_level_table)
// holds, for every l < L, an offset whose level lies inside the atlas.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {

struct TexDesc {  // == rtpt_texture
  uint32_t width, height, first_texel, flags;
};
constexpr uint32_t kTexNearest = 0x1u;  // RTPT_TEX_NEAREST
constexpr uint32_t kTexMipmap = 0x10u;  // RTPT_TEX_MIPMAP
// the level table, one row per texture (texture_host.hpp: kLevelRow): [l] first texel of level l, [17] number of levels
constexpr uint32_t kTexLevelRow = 20u, kTexLevelRowCount = 17u;
// footprint growth per unit length of a bounce segment: a definition (a cone of 1/8 radian), not a measurement
constexpr float kTexBounceSpread = 0.125f;

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

// piecewise-linear log2 of a positive finite binary32: exponent + mantissa fraction
__device__ __forceinline__ float plog2(float x) {
  const uint32_t b = __float_as_uint(x);
  return static_cast<float>(static_cast<int>(b >> 23) - 127) + static_cast<float>(b & 0x7FFFFFu) * 0x1p-23f;
}

// The level a hit reads, before the clamp to the chain.  w: the footprint width at the hit; nd: n . d; p: the three posed
// vertices of the hit's shade record; t0, t1: its uv record; W x H: level 0 of its texture.
__device__ __forceinline__ float footprint_lod(float w, float nd, float4 p0, float4 p1, float4 p2, float4 t0, float4 t1, uint32_t W, uint32_t H) {
  const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z;
  const float e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
  const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  const float aw = __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
  const float at = __builtin_fabsf(((t0.z - t0.x) * (t1.y - t0.y) - (t1.x - t0.x) * (t0.w - t0.y)) * (static_cast<float>(W) * static_cast<float>(H)));
  const float D = at / aw;
  const float rho2 = ((w * w) * D) / (nd * nd);
  const float inf = __builtin_inff();
  return (D > 0.0f && D < inf && rho2 > 0.0f && rho2 < inf) ? 0.5f * plog2(rho2) : 0.0f;
}

// the texture at level lambda (any bit pattern); lv: this texture's row of the level table
__device__ __forceinline__ float4 sample_lod(const TexDesc d, const uint32_t* __restrict__ lv, const float4* __restrict__ texels, float u,
                                             float v, float lambda) {
  uint32_t L = lv[kTexLevelRowCount];
  L = L < 1u ? 1u : (L > kTexLevelRowCount ? kTexLevelRowCount : L);
  const float top = static_cast<float>(L - 1u);
  lambda = lambda > 0.0f ? lambda : 0.0f;
  lambda = lambda < top ? lambda : top;
  const bool nearest = (d.flags & kTexNearest) != 0;
  auto level = [&](uint32_t l) {  // l < L: `sample` of the level's own rectangle
    const uint32_t w = d.width >> l, h = d.height >> l;
    return sample(TexDesc{w ? w : 1u, h ? h : 1u, lv[l], d.flags}, texels, u, v);
  };
  const int li = static_cast<int>(__builtin_floorf(nearest ? lambda + 0.5f : lambda));
  const uint32_t l0 = li < 0 ? 0u : (static_cast<uint32_t>(li) > L - 1u ? L - 1u : static_cast<uint32_t>(li));
  const float4 a = level(l0);
  if (nearest) return a;
  const float f = lambda - static_cast<float>(l0);
  if (!(f > 0.0f)) return a;
  return lerp4(a, level(l0 + 1u > L - 1u ? L - 1u : l0 + 1u), f);
}

}  // namespace tex
}  // namespace rt
