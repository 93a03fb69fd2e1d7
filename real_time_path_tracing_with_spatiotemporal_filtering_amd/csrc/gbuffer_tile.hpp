// gbuffer_tile.hpp — K0 (the G-buffer as pixel-centre primary rays) and K1 (the temporal gradient) for one pixel and for one 64 x 4
// tile, stated once: k_gbuffer and k_gradient run them as launches of their own, the fused K0 + K1 + K2 launch
// (gbuffer_pathtrace_body, pathtrace_tile.hpp) as the workgroups behind its tracing tiles.  Everything here is force-inlined; the
// caller owns the dynamic LDS of the node stack.
#pragma once

#include "closest_hit.hpp"
#include "shading_normal.hpp"

namespace rt {
namespace {

// ------------------------------------------------------------------------------------------
// K1 temporal gradient
// ------------------------------------------------------------------------------------------
// temporalGradient.comp.glsl:71-101
__device__ __forceinline__ f3 phong(f3 p, f3 n, f3 cam, f3 lpos, f3 lcol) {
  f3 ldir = exact::normalize(lpos - p);
  f3 ambient = lcol * 0.1f;
  float diff = glsl_max(exact::dot(n, ldir), 0.0f);
  f3 diffuse = lcol * diff;
  f3 vdir = exact::normalize(cam - p);
  f3 I = -ldir;
  float two_ndi = 2.0f * exact::dot(n, I);
  f3 rdir{fmaf_(-two_ndi, n.x, I.x), fmaf_(-two_ndi, n.y, I.y), fmaf_(-two_ndi, n.z, I.z)};
  float spec = exact::powi(glsl_max(exact::dot(vdir, rdir), 0.0f), 128);
  f3 specular = lcol * (0.5f * spec);
  return ((ambient + diffuse) + specular) * 0.7f;
}

// temporalGradient.comp.glsl:128-167 for one pixel: relative change of the Phong shade of the visible surface point between
// the previous and the current light (and pose)
__device__ __forceinline__ float gradient_lambda(uint32_t id, f3 wp, const float4* lut, const float4* lut_prev, const float4* normal_tab,
                                                 const float4* area_tab, f3 cam, f3 light, f3 light_prev, f3 color, f3 color_prev) {
  if (id == 0) return 0.0f;  // :128-131
  f3 va = xyz(lut[3 * id]), vb = xyz(lut[3 * id + 1]), vc = xyz(lut[3 * id + 2]);
  // :142 normalize(cross(vb - va, vc - va)) — k_lut computed exactly that from exactly these vertices, once per triangle
  // (normal_tab[id]); per pixel it is 36 VALU of a VALU-bound kernel
  f3 nrm = xyz(normal_tab[id]);
  // :143; the whole triangle's area (:60) comes from k_lut's table: same vertices, same arithmetic, once per triangle
  f3 bc = bary_coords_at(wp, va, vb, vc, area_tab[id].x);
  f3 pa = xyz(lut_prev[3 * id]), pb = xyz(lut_prev[3 * id + 1]), pc = xyz(lut_prev[3 * id + 2]);
  f3 wpp = bary_mix(bc, pa, pb, pc);                          // :153
  f3 cur = phong(wp, nrm, cam, light, color);                 // :158
  f3 prv = phong(wpp, nrm, cam, light_prev, color_prev);      // :161 (current normal!)
  f3 tg = cur - prv;
  float delta = glsl_max(exact::length(cur), exact::length(prv));  // :166
  // (hipcc's division on purpose: with the light at rest the numerator is +0 for every pixel, which exact::div_ would hand
  // to the long path after paying for the short one)
  return glsl_min(1.0f, exact::length(tg) / delta);                // :167
}

__device__ __forceinline__ void store_gradient(float4* grad, size_t i, float lam) {
  // nothing on the reference's path reads the gradient again (its consumer is commented out,
  // temporalFiltering.comp.glsl:247-248): keep the 133 MB out of the caches the filter passes need
  typedef float v4f_ __attribute__((ext_vector_type(4)));
  v4f_ g4 = {lam, lam, lam, 0.0f};
  __builtin_nontemporal_store(g4, reinterpret_cast<v4f_*>(grad + i));
}

// ------------------------------------------------------------------------------------------
// K0 G-buffer
// ------------------------------------------------------------------------------------------
// RTPT_FLAG_EXT_SMOOTH_GUIDE: the cell of the per-pixel normal plane at a hit with id1 > 0, the guide normal of shading_normal.hpp
// (G1-G5) from K0's own barycentrics; normal_tab[id1] where G4 says so.  The matrix is loaded only behind a smooth record.
__device__ __forceinline__ float4 guide_cell(const NormalView& nv, const float4* normal_tab, uint32_t id1, uint32_t n_base, float b0, float b1, float b2) {
  const float4 tab = normal_tab[id1];
  const uint32_t t = (id1 - 1) % n_base, i = (id1 - 1) / n_base;
  const float4* r = nv.records + 3 * static_cast<size_t>(t);
  const float4 r0 = r[0];
  if (__float_as_uint(r0.w) == 0u) return tab;
  const float4 r1 = r[1], r2 = r[2];
  const float4* c = nv.cof + 3 * static_cast<size_t>(i);
  const float4 c0 = c[0], c1 = c[1], c2 = c[2];
  f3 ns;
  if (!nrm::guide(xyz(r0), xyz(r1), xyz(r2), b0, b1, b2, xyz(c0), xyz(c1), xyz(c2), xyz(tab), &ns)) return tab;
  return make_float4(ns.x, ns.y, ns.z, nrm::guide_self_weight(ns, nv.sigma_n));
}

// K0 (+ K1 when a.grad_on) for pixel (x, y), which must lie inside the frame and inside a's rows; `cand` = span_candidates of
// the pixel's wave (brute force with culling only).  alpha_image != NULL (the fused K0 + K1 + K2 launch): the depth also goes
// into the alpha of that image's pixel for rows [ay0, ay1) — the traced image is "rgbd" (atrous.hip) and the tracing
// workgroups of that launch store the colour's 12 bytes only.
// NV: nothing, or the scene's NormalView (kernels.hpp: the NRM axis).  With one, and while its `guide` word is set, the pixel's cell
// of a.normals is guide_cell's; every other instantiation, and every launch without the switch, stores normal_tab[id1].
template <int BVH, class... NV>
__device__ __forceinline__ void gbuffer_pixel(const GbufferArgs& a, int x, int y, unsigned long long cand, uint32_t* stack, int tid, int nt,
                                              float4* alpha_image = nullptr, int ay0 = 0, int ay1 = 0, const NV&... nv) {
  static_assert(sizeof...(NV) == 0 || (sizeof...(NV) == 1 && pack_nrm<NV...>()), "a NormalView or nothing");
  // view-space direction of the pixel-centre ray: (ndc.x / P00, ndc.y / P11, -1) with ndc = (2 (x + .5) - W) / W.  Each
  // component is a function of the column or of the row alone: k_ray_tables evaluates the two divisions per column / row
  // once (same operands, same correctly-rounded operations), K0 reads them back — 4 divisions less per pixel
  f3 dv{a.dvx[x], a.dvy[y], -1.0f};
  f3 c0 = ld3(a.c0), c1 = ld3(a.c1), c2 = ld3(a.c2);
  f3 d = exact::normalize(f3{exact::dot(c0, dv), exact::dot(c1, dv), exact::dot(c2, dv)});
  f3 o = ld3(a.org);
  HitRec h{a.tmax, 0u, 0.f, 0.f, 1.f};
  if (!BVH && a.cull)
    closest_hit_brute_set(a.scene, cand, o, d, h);
  else
    closest_hit<BVH>(a.scene, o, d, h, stack, tid, nt);
  const size_t i = static_cast<size_t>(y - a.g.row_base) * a.g.W + x;
  a.vis[i] = h.id1;  // visibility.frag.glsl:23
  bool guide = false;  // the cell is written below, behind the barycentrics
  if constexpr (sizeof...(NV) != 0) guide = a.normals && pack_get<NormalView>(nv...).guide != 0u && h.id1 != 0u;
  if (a.normals && !guide) a.normals[i] = a.normal_tab[h.id1];
  f3 wp{0.f, 0.f, 0.f};
  float dep = 1.0f;  // clear depth  main.cpp:1421
  if (h.id1) {
    float b1 = RTPT_DIV_SH(-h.u, h.ad), b2 = RTPT_DIV_SH(h.v, h.ad);
    float b0 = 1.0f - b1 - b2;
    if constexpr (sizeof...(NV) != 0) {
      if (guide) a.normals[i] = guide_cell(pack_get<NormalView>(nv...), a.normal_tab, h.id1, a.scene.n_base_tris, b0, b1, b2);
    }
    const float4* s = a.scene.shade + 3 * static_cast<size_t>(h.id1 - 1);
    wp = bary_point(xyz(s[0]), xyz(s[1]), xyz(s[2]), b0, b1, b2);
    a.worldpos[i] = make_float4(wp.x, wp.y, wp.z, 1.0f);
    float cz = exact::mat_row_point(a.PV, 2, wp), cw = exact::mat_row_point(a.PV, 3, wp);
    dep = exact::div_(cz, cw);
  } else {
    a.worldpos[i] = make_float4(0.f, 0.f, 0.f, 1.0f);  // clear colour main.cpp:1420
  }
  a.depth[i] = dep;
  if (alpha_image && y >= ay0 && y < ay1) reinterpret_cast<float*>(alpha_image + i)[3] = dep;
  if (a.grad_on && y >= a.grad_y0 && y < a.grad_y1) {
    // K1 (temporalGradient.comp.glsl:104-172) on the values K0 just stored — the same bits it would load back (the world
    // position is computed ONCE: the stores above may alias the vertex records as far as the compiler knows, so a
    // second evaluation was a second evaluation)
    store_gradient(a.grad, i, gradient_lambda(h.id1, wp, a.lut, a.lut_prev, a.normal_tab, a.area_tab, ld3(a.g_cam), ld3(a.g_light), ld3(a.g_light_prev),
                                              ld3(a.g_color), ld3(a.g_color_prev)));
  }
}

// the 64 x 4-pixel tile (bx, by) of a's rows (k_gbuffer's workgroup, and the G-buffer workgroups of the fused launch)
template <int BVH, class... NV>
__device__ __forceinline__ void gbuffer_tile(const GbufferArgs& a, uint32_t bx, uint32_t by, uint32_t* stack, float4* alpha_image = nullptr, int ay0 = 0,
                                             int ay1 = 0, const NV&... nv) {
  const int tid = threadIdx.y * kBlockX + threadIdx.x;
  const uint32_t tp = tile_pixel(static_cast<int>(threadIdx.y), threadIdx.x);
  const int x = static_cast<int>(bx) * kBlockX + static_cast<int>(tp & 63u);
  const int y = a.g.y0 + static_cast<int>(by) * kBlockY + static_cast<int>(tp >> 6);
  unsigned long long cand = 0;
  if (!BVH && a.cull)
    cand = span_candidates(a.bounds, a.scene.n_tris, static_cast<int>(bx) * kBlockX + wave_x0(static_cast<int>(threadIdx.y)),
                           a.g.y0 + static_cast<int>(by) * kBlockY);
  if (x >= a.g.W || y >= a.g.y1) return;
  gbuffer_pixel<BVH>(a, x, y, cand, stack, tid, kThreads, alpha_image, ay0, ay1, nv...);
}

}  // namespace
}  // namespace rt
