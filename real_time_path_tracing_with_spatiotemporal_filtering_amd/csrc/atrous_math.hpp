// atrous_math.hpp — K3's per-pixel arithmetic (temporalFiltering.comp.glsl:118-155 the filter, :213-263 reprojection and
// temporal blend), stated once.  k_atrous, k_atrous_ext, k_atrous_comb_sh (atrous.hip), k_atrous_chain (atrous_chain.hip)
// and k_atrous_chain_sw (experiments/chain_sliding_window.inc) call these and keep what is theirs: staging, addressing,
// work lists, barriers and stores.  The reprojection itself is device_common.hpp's reproject_pixel().  Everything here is
// force-inlined and takes its inputs by value (see EdgeStop).
#pragma once

#include "device_common.hpp"

namespace rt {
namespace {

// x^n for the normal weight (temporalFiltering.comp.glsl:62).  The reference's exponent is 128: seven squarings,
// written straight-line — exact::powi's square-and-multiply LOOP yields the same products in the same order but
// runs its control flow on the CU's single scalar unit, which made per-tap use of it SALU-bound.
__device__ __forceinline__ float pow_sigma(float x, int n) {
  if (n == 128) {
    const float x2 = x * x, x4 = x2 * x2, x8 = x4 * x4, x16 = x8 * x8, x32 = x16 * x16, x64 = x32 * x32;
    return x64 * x64;
  }
  return exact::powi(x, n);
}

__device__ __forceinline__ float luminance(f3 c) { return fmaf_(0.0722f, c.z, fmaf_(0.7152f, c.y, 0.2126f * c.x)); }

// gaussianKernel2D (temporalFiltering.comp.glsl:93-99; the reference declares it and never uses it), offsets -2..2; the
// tap's h is gauss5(i, j) / 273 (RTPT_FLAG_EXT_GAUSS5)
__device__ __forceinline__ float gauss5(int i, int j) {
  constexpr float k[5][5] = {{1, 4, 7, 4, 1}, {4, 16, 26, 16, 4}, {7, 26, 41, 26, 7}, {4, 16, 26, 16, 4}, {1, 4, 7, 4, 1}};
  return k[i + 2][j + 2];
}

// Variance guidance (RTPT_FLAG_EXT_VARIANCE, extension): the colour term of a tap's weight compares luminances, scaled by
// the centre pixel's own standard deviation instead of sigma_l.  `var` is that pixel's (prefiltered) variance.
struct VarGuide {
  float lum_p, lum_scale, cl_var;  // cl_var = -log2(e) / lum_scale: the fast path's exponent scale
};
__device__ __forceinline__ VarGuide var_guide(float sigma_l, f3 cp, bool use_var, float var) {
  VarGuide v;
  v.lum_p = luminance(cp);
  v.lum_scale = use_var ? fmaf_(sigma_l, exact::sqrt_(glsl_max(var, 0.0f)), 1e-4f) : 1.0f;
  v.cl_var = -1.44269504088896341f * fast::rcp_(v.lum_scale);
  return v;
}

// what the weight needs of AtrousArgs, by value: a helper that takes the kernel's argument struct by reference keeps the
// optimiser from treating its pointers as kernel arguments until late, and the instructions change
struct EdgeStop {
  float sigma_z, sigma_l, cz, cl;  // cz / cl = -log2(e) / sigma, set by the launch
};
// The edge-stopping weight of tap q against the centre p, given the normal weight wn (:62, from the id-pair table, the
// per-id self weight or pow_sigma): wn * exp(-|dz| / sigma_z) * exp(-|dc| / sigma_l)  (:67-68, :73, :77).
// EXACT: the contract's arithmetic, three factors.  Otherwise the two exponentials are one exp2:
// exp(-|dz|/sz) * exp(-|dc|/sl) = exp2(|dz| * cz + |dc| * cl).
// use_var: the colour term is the variance-guided one (extension family only).
template <bool EXACT>
__device__ __forceinline__ float edge_weight(EdgeStop s, float wn, f3 cp, f3 cq, float dp, float dq, bool use_var = false,
                                             VarGuide v = VarGuide{0.0f, 1.0f, 0.0f}) {
  const f3 dc = cp - cq;
  if (EXACT) {
    const float wd = exact::exp_(-__builtin_fabsf(dp - dq) / s.sigma_z);  // :67-68
    const float wl = use_var ? exact::exp_(-__builtin_fabsf(v.lum_p - luminance(cq)) / v.lum_scale)
                             : exact::exp_(-exact::length(dc) / s.sigma_l);  // :73
    return (wn * wd) * wl;                                                // :77
  }
  const float dl = use_var ? __builtin_fabsf(v.lum_p - luminance(cq)) * v.cl_var : fast::sqrt_(exact::dot(dc, dc)) * s.cl;
  const float e = fmaf_(__builtin_fabsf(dp - dq), s.cz, dl);
  return wn * __builtin_amdgcn_exp2f(e);
}

// The centre tap (q == p) of the plain 3x3 filter: cp - cp and dp - dp are 0, both exponentials exactly 1 and the weight is the
// id's self weight — while colour and depth are finite.  A channel or a depth that is Inf or NaN makes Inf - Inf = NaN in the
// reference's own arithmetic (:67-77, the loop treats the centre like any tap), and the NaN weight turns the whole pixel NaN.
// x * 0 is +-0 for a finite x and NaN otherwise, so the sum below leaves wself (>= +0) bit for bit or makes it NaN.
__device__ __forceinline__ float centre_weight(float wself, f3 cp, float dp) {
  return wself + fmaf_(cp.x, 0.0f, fmaf_(cp.y, 0.0f, fmaf_(cp.z, 0.0f, dp * 0.0f)));
}

// :146-147, one tap into the sums; hw = h * w with the tap's own h (:145: 1/9, or gauss5 / 273).  The extension family
// calls this form.
__device__ __forceinline__ void tap_add_h(f3& num, float& den, float hw, f3 cq) {
  num = f3{fmaf_(hw, cq.x, num.x), fmaf_(hw, cq.y, num.y), fmaf_(hw, cq.z, num.z)};  // :146
  den = den + hw;                                                                    // :147
}
// The plain 3x3 filter: h = 1/9 (:145) scales numerator and denominator alike, so the fast path drops it.
template <bool EXACT>
__device__ __forceinline__ void tap_add(f3& num, float& den, float w, f3 cq) {
  tap_add_h(num, den, EXACT ? (1.0f / 9.0f) * w : w, cq);
}

// :150.  EXACT (and the whole extension family): correctly-rounded divisions; otherwise one reciprocal.
template <bool EXACT>
__device__ __forceinline__ f3 normalise(f3 num, float den) {
  if (EXACT) return f3{num.x / den, num.y / den, num.z / den};
  return num * fast::rcp_(den);
}

// :253 the history colour at the reprojected pixel; D2: 0 outside the image.  The plane holds frame rows [y0, y1), stored
// from row_base on.
__device__ __forceinline__ f3 history_at(int ppx, int ppy, int W, int y0, int y1, const float4* history, int row_base) {
  f3 hc{0.f, 0.f, 0.f};
  if (ppx >= 0 && ppx < W && ppy >= y0 && ppy < y1) hc = xyz(history[static_cast<size_t>(ppy - row_base) * W + ppx]);
  return hc;
}

// :254
__device__ __forceinline__ f3 temporal_blend(f3 filtered, f3 hc, float alpha) {
  const float oma = 1.0f - alpha;
  return f3{fmaf_(filtered.x, alpha, hc.x * oma), fmaf_(filtered.y, alpha, hc.y * oma), fmaf_(filtered.z, alpha, hc.z * oma)};
}

// The final pass of the extension modes, in front of the blend.  RTPT_FLAG_EXT_DISOCCLUSION keeps the history only where
// previousVisibilityBuffer (main.cpp:1367: copied every frame, never read) holds the same primitive at the reprojected
// pixel; the plane holds frame rows [y0, y1) from row_base on, and rows this context does not hold count as disoccluded.
__device__ __forceinline__ bool same_primitive_at(const uint32_t* prev_vis, int W, int H, int row_base, int y0, int y1, int ppx, int ppy,
                                                  uint32_t idp) {
  const bool inside = ppx >= 0 && ppx < W && ppy >= 0 && ppy < H;
  return inside && ppy >= y0 && ppy < y1 && prev_vis[static_cast<size_t>(ppy - row_base) * W + ppx] == idp;
}
// RTPT_FLAG_EXT_ADAPTIVE_ALPHA, :247-248 (commented out in the reference); g: the pixel's temporal gradient
__device__ __forceinline__ float adaptive_alpha(float alpha, float g) { return fmaf_(1.0f - g, alpha, g); }

// main.cpp:1338-1361 vkCmdBlitImage image (RGBA32F) -> swapchain image (B8G8R8A8_UNORM): the float -> UNORM
// conversion clamps to [0,1] and quantises; defined here as trunc(x*255 + 0.5) with separate multiply and add (the
// files are compiled -ffp-contract=off), NaN -> 0 (max(NaN, 0) = 0), which is what output.to_unorm8 / the oracle compute.
__device__ __forceinline__ uint32_t unorm8(float x) {
  const float c = fminf(fmaxf(x, 0.0f), 1.0f);
  return static_cast<uint32_t>(c * 255.0f + 0.5f);
}
__device__ __forceinline__ uint32_t pack_bgra8(f3 c, float alpha) {
  return unorm8(c.z) | (unorm8(c.y) << 8) | (unorm8(c.x) << 16) | (unorm8(alpha) << 24);
}

}  // namespace
}  // namespace rt
