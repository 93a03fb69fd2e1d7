// kernels.hpp — launch interface between the C-ABI layer (api_*.hip) and the gfx950 kernels
// (kernels.hip, selftest_kernels.hip).  Plain structs passed by value as kernel arguments.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <tuple>
#include <type_traits>

#include "bvh.hpp"
#include "texture.hpp"

namespace rt {

// Device view of the scene.  Records are float4 triples:
//   isect record  r0 = (v0.x, v0.y, v0.z, e1.x)  r1 = (e1.y, e1.z, e2.x, e2.y)  r2 = (e2.z, n.x, n.y, n.z)   n = e1 x e2
//   shade record  s0 = (v0.xyz, n.x)  s1 = (v1.xyz, n.y)  s2 = (v2.xyz, n.z)     n = unit geometric normal
struct SceneView {
  const float4* isect_id;    // id order  (small-scene wave-uniform brute force)
  // BVH leaf order.  leaf_pairs == 0: one 48-byte isect record per leaf slot.  leaf_pairs != 0: one 80-byte record per PAIR
  // of slots (2q, 2q + 1) — the two fan triangles share v0 and the edge e2_A == e1_B, and their ids ride in the record:
  //   p0 = (v0.xyz, e1.x)  p1 = (e1.yz, e2.xy)  p2 = (e2.z, n.xyz)  p3 = (e2_B.xyz, n_B.x)  p4 = (n_B.yz, id_A, id_B as bits)
  // five 16-byte loads per pair test instead of five + two id loads (the traversal is bound by its vector-memory requests)
  const float4* isect_leaf;
  const uint32_t* leaf_ids;  // triangle id of each leaf slot
  const float4* shade;       // id order
  const BvhNodeQ* nodes;     // 32-byte child-pair nodes, boxes on a 16-bit grid (bvh.hpp)
  const float* bvh_grid;  // device: origin xyz, cell xyz of the nodes' 16-bit grid (rewritten by a device-side refit)
  uint32_t n_tris;
  uint32_t use_bvh;  // 0: brute force over isect_id, 1: BVH traversal
  uint32_t paired;   // brute force only: triangles (2q, 2q+1) share v0 and the edge v2_A == v1_B bitwise (fan-triangulated faces)
  uint32_t leaf_pairs;  // BVH: built over such pairs (bvh.hpp): every leaf holds whole pairs, A right before B
  uint32_t stack_depth;  // BVH traversal stack entries per lane (tree depth + 2)
  // The first stack_lds entries of a lane's stack live in LDS (what sets the workgroups per CU: the 1.15M-triangle
  // tree is 28 deep, 30 KB per workgroup = 5 per CU, and its trace is that sensitive to occupancy: 2 / 3 / 4 / 5
  // workgroups per CU 5.75 / 4.74 / 4.07 / 3.62 ms); deeper entries, which few rays ever reach, go to stack_spill in
  // global memory: [entry - stack_lds][workgroup of the launch][thread]
  uint32_t stack_lds;
  uint32_t* stack_spill;
  // optional per-triangle materials of the BASE mesh (.mtl Kd / Ke; instance i, triangle t reads record t):
  //   m0 = (Kd.rgb, 0)  m1 = (Ke.rgb, 1 if emissive else 0).  NULL: the reference's normal-keyed colours
  //   a specular material (rtpt_scene_set_materials_ext): m0 = (Ks.rgb, -roughness), -0.0f for the mirror (specular.hpp)
  //   a dielectric one: m0 = (colour, ior), m1 = (1 / ior, R0, 0, 0) (dielectric.hpp)
  const float4* materials;
  uint32_t n_base_tris;
};

// Optional albedo textures of the BASE mesh (rtpt_scene_set_textures; texture.hpp): two float4 per triangle (corner uvs and the
// texture index), the descriptors, and the RGBA32F atlas they index.  All NULL without textures.  It travels as the LAST
// parameter of the path-trace kernels, not inside SceneView: as three more pointers there it moved every later field of
// PathtraceArgs / GbufferArgs by 24 bytes, and the 1,152,000-triangle frame measured 0.1 % slower with textures off.  Behind
// the other arguments it leaves every existing offset, and so the code of the TEX = false instantiations, as it was.
// levels: the per-texture table of level offsets (texture.hpp: kTexLevelRow dwords a texture), non-NULL exactly when some texture
// has RTPT_TEX_MIPMAP — what selects the mip instantiations; bounce_spread: kTexBounceSpread unless the environment overrides it.
struct TexView {
  const float4* records;
  const TexDesc* desc;
  const float4* texels;
  const uint32_t* levels;
  float bounce_spread;
};

// The light list of next-event estimation (RTPT_FLAG_EXT_NEE; light_sample.hpp, light_list_host.hpp): ids[i] = id + 1 of a posed
// emissive triangle, ascending; n in [1, 2^24] where a kernel reads it.  It travels as a parameter of its own behind TexView, and
// only of the instantiations that sample lights (kernels.hip: the tile kernels' trailing parameter pack), for TexView's reason:
// inside SceneView the pointer would move every later field of PathtraceArgs / GbufferArgs, and as a field of TexView it would
// change the argument segment of every tracing kernel.  The instantiations that sample the sphere light too
// (RTPT_FLAG_EXT_NEE_SPHERE) take it the same way; there ids may be NULL and n 0: no triangle is sampled.
struct LightView {
  const uint32_t* ids;
  uint32_t n;
};
// The light list with the cumulative table of RTPT_FLAG_EXT_NEE_POWER behind it (light_sample.hpp: pick_power; light_table.hip
// builds it): cdf[i] = the sum of the quantised weights of entries 0..i, cdf[n - 1] = S.  A sibling of LightView, not a field of
// it: the instantiations that pick by weight take this one, the others that sample lights a LightView — its first two fields —
// so that their argument segments and their code are those of a build without the table.  ids, cdf non-NULL and n in [1, 2^24]
// wherever a kernel takes it.  The host carries the list in this form (launch_pathtrace), cdf NULL where there is no table.
struct LightTableView {
  const uint32_t* ids;
  uint32_t n;
  const uint64_t* cdf;
};

// THE SPEC AXIS of shade_segment and the tile kernels, and launch_pathtrace's `specular`.  0, 1, 2 are the material modes
// (Scene::materials_specular): every material diffuse, some specular, some dielectric.  The values above them sample lights and
// include the specular and dielectric bounces:
//   kSpecNee             RTPT_FLAG_EXT_NEE on a scene whose light list has entries: the triangles of the list, picked uniformly
//   kSpecNeeSphere       a context with RTPT_FLAG_EXT_NEE_SPHERE, whatever the scene's materials or light list: the analytic
//                        sphere light, and the triangles where the list has entries
//   kSpecNeePower        RTPT_FLAG_EXT_NEE and RTPT_FLAG_EXT_NEE_POWER on a list with entries: kSpecNee with the weighted pick
//   kSpecNeeSpherePower  ... and RTPT_FLAG_EXT_NEE_SPHERE besides: kSpecNeeSphere with it (with an empty list 0x60000 launches
//                        kSpecNeeSphere)
//   kSpecNeeMis, kSpecNeeSphereMis, kSpecNeePowerMis, kSpecNeeSpherePowerMis
//                        RTPT_FLAG_EXT_NEE_MIS on top of RTPT_FLAG_EXT_NEE on a list with entries: the four above with the light
//                        sample and the bounce that meets an emitter weighed against each other (light_sample.hpp: MULTIPLE
//                        IMPORTANCE SAMPLING).  Such an instantiation always has a list with entries: with the sphere flag on an
//                        empty list 0xA0000 launches kSpecNeeSphere.  The sphere sample is not weighed.
// Nothing outside this block compares a SPEC with a number: it asks the predicates.
constexpr int kSpecNee = 3;
constexpr int kSpecNeeSphere = 4;
constexpr int kSpecNeePower = 5;
constexpr int kSpecNeeSpherePower = 6;
constexpr int kSpecNeeMis = 7;
constexpr int kSpecNeeSphereMis = 8;
constexpr int kSpecNeePowerMis = 9;
constexpr int kSpecNeeSpherePowerMis = 10;
constexpr int kSpecModes = 11;  // SPEC lies in [0, kSpecModes)
constexpr bool spec_lights(int spec) { return spec >= kSpecNee; }                                        // samples lights
constexpr bool spec_mis(int spec) { return spec >= kSpecNeeMis; }                                        // ... and weighs them (MIS)
constexpr int spec_unweighed(int spec) { return spec_mis(spec) ? spec - (kSpecNeeMis - kSpecNee) : spec; }  // the value without MIS
constexpr bool spec_sphere(int spec) {                                                                   // ... the sphere light
  return spec_unweighed(spec) == kSpecNeeSphere || spec_unweighed(spec) == kSpecNeeSpherePower;
}
constexpr bool spec_power(int spec) {                                                                    // ... picks by weight
  return spec_unweighed(spec) == kSpecNeePower || spec_unweighed(spec) == kSpecNeeSpherePower;
}
constexpr bool spec_may_be_empty(int spec) { return spec_sphere(spec) && !spec_power(spec) && !spec_mis(spec); }  // ... maybe from no list
constexpr int spec_material(int spec) { return spec_lights(spec) ? 2 : spec; }                           // its material mode
// what an instantiation takes behind TexView: nothing (void), the list, or the list with its table
template <int SPEC>
using spec_lights_t = std::conditional_t<spec_power(SPEC), LightTableView, std::conditional_t<spec_lights(SPEC), LightView, void>>;
// ... as a trailing parameter pack LV: empty, or that one type
template <int SPEC, class... LV>
constexpr bool spec_takes() {
  return sizeof...(LV) == (spec_lights(SPEC) ? 1u : 0u) && (std::is_same<LV, spec_lights_t<SPEC>>::value && ...);
}

// Smooth shading (rtpt_scene_set_normals; shading_normal.hpp states the two arrays and the rules): the corner normals of the BASE
// mesh and the cofactor matrix of every instance's pose.  It travels as the LAST parameter of the tracing kernels that shade with
// it, behind TexView and the light argument, and of those instantiations only — TexView's reason: inside SceneView it would move
// every later argument offset and change every existing kernel.  THE NRM AXIS of shade_segment and the tracing kernels is whether
// an instantiation's trailing parameter pack ends in a NormalView (pack_nrm): the instantiations without one keep their names,
// their argument segments and their code.  Instantiated where a scene with normals can be launched: the BVH scene modes (such a
// scene is traced through its tree), the fused launch and the unfused compacting one, the queue kernels; no
// RTPT_FLAG_NO_PATH_COMPACTION form, no brute-force form.
// RTPT_FLAG_EXT_SMOOTH_GUIDE rides here too, for the same reason: `guide` != 0 while the switch is active, and K0 of these
// instantiations (gbuffer_tile.hpp; k_gbuffer's two with a NormalView, the G-buffer workgroups of the fused launch) then writes the
// guide normal of shading_normal.hpp (G1-G5) into the per-pixel plane, its self weight formed with `sigma_n` (k_lut's formula).
// With guide == 0 they store normal_tab[id], like every instantiation without a NormalView.
struct NormalView {
  const float4* records;  // 3 per base triangle
  const float4* cof;      // 3 per instance
  uint32_t guide;         // RTPT_FLAG_EXT_SMOOTH_GUIDE is active
  int32_t sigma_n;        // rtpt_config::sigma_n, read only while guide != 0
};
// The environment map (rtpt_set_environment; env.hpp states the rules E1 to E6): n x n RGBA32F texels of an octahedral map, the rows
// of its rotation and its scale.  It travels as the LAST parameter of the tracing kernels that read it, behind TexView, the light
// argument and the NormalView, and of those instantiations only — NormalView's reason.  THE ENV AXIS of shade_segment and the tile
// kernels is whether an instantiation's trailing parameter pack ends in an EnvView (pack_env): there a path that meets nothing is
// multiplied by env::color(d), everywhere else by sky_color(d), and the instantiations without one keep their names, their argument
// segments and their code.  An environment launch has the limits of a launch that samples lights: every segment runs in the tile
// kernel (no queue kernels) and the launch carries no final pass.  Instantiated for the fused launch and the unfused compacting
// one, in every scene mode, with and without a NormalView; no RTPT_FLAG_NO_PATH_COMPACTION form (rtpt_set_environment refuses such
// a context).  n in [1, 4096] and texels non-NULL wherever a kernel takes it.
struct EnvView {
  const float4* texels;
  uint32_t n, flags;  // flags: RTPT_TEX_NEAREST (kTexNearest) or 0
  float4 r0, r1, r2;  // rows of the rotation, .w spare
  float4 scale;       // rgb, .w spare
};
template <class... P>
struct pack_last {
  using type = void;
};
template <class A>
struct pack_last<A> {
  using type = A;
};
template <class A, class B, class... P>
struct pack_last<A, B, P...> {
  using type = typename pack_last<B, P...>::type;
};
// ... and the one in front of the last
template <class... P>
struct pack_last2 {
  using type = void;
};
template <class A, class B>
struct pack_last2<A, B> {
  using type = A;
};
template <class A, class B, class C, class... P>
struct pack_last2<A, B, C, P...> {
  using type = typename pack_last2<B, C, P...>::type;
};
template <class... P>
constexpr bool pack_env() {
  return std::is_same<typename pack_last<P...>::type, EnvView>::value;
}
template <class... P>
constexpr bool pack_nrm() {
  return std::is_same<typename pack_last<P...>::type, NormalView>::value ||
         (pack_env<P...>() && std::is_same<typename pack_last2<P...>::type, NormalView>::value);
}
// a tracing kernel's pack: the light argument of its SPEC (spec_takes), then a NormalView or nothing, then an EnvView or nothing
template <int SPEC, class... P>
constexpr bool pack_takes() {
  constexpr size_t want = (spec_lights(SPEC) ? 1u : 0u) + (pack_nrm<P...>() ? 1u : 0u) + (pack_env<P...>() ? 1u : 0u);
  if constexpr (sizeof...(P) != want) return false;
  else if constexpr (spec_lights(SPEC)) return std::is_same<std::tuple_element_t<0, std::tuple<P...>>, spec_lights_t<SPEC>>::value;
  else return true;
}
// the first argument of a pack, and its first argument of type T
template <class A, class... P>
constexpr const A& pack_first(const A& a, const P&...) {
  return a;
}
template <class T, class A, class... P>
constexpr const T& pack_get(const A& a, const P&... p) {
  if constexpr (std::is_same<A, T>::value) return a;
  else return pack_get<T>(p...);
}

// Texel (x, y) of level l + 1 of a mip chain = ((a + b) + (c + d)) * 0.25f of the texels (2x, 2y), (min(2x + 1, sw - 1), 2y)
// and the same columns of row min(2y + 1, sh - 1) of level l (texture_mips.hip): one launch per level.  src and dst are texel
// offsets into `atlas`; dw = max(1, sw >> 1), dh = max(1, sh >> 1).
void launch_mip_downsample(float4* atlas, uint32_t src, uint32_t sw, uint32_t sh, uint32_t dst, hipStream_t s);

// Screen-space bounds of every triangle of a small scene (<= 64), computed on the host per call and
// passed in the kernel-argument segment (scalar loads).  A wave covers 64 pixels of one row; a
// triangle whose padded bounds miss that span cannot be hit by any of the wave's PRIMARY rays, so the
// wave skips it with a scalar branch.  Conservative by construction => results are unchanged.
struct TriBounds {
  int16_t x0, y0, x1, y1;  // inclusive pixel bounds, already padded; x0 > x1 marks "never"
};
constexpr int kCullMaxTris = 64;

struct FrameGeom {
  int32_t W, H;      // full frame
  int32_t row_base;  // first frame row stored in the planes of this context
  int32_t y0, y1;    // rows to compute (frame coordinates)
};

struct GbufferArgs {
  FrameGeom g;
  SceneView scene;
  float org[3];          // camera origin = -R^T t
  float c0[3], c1[3], c2[3];  // columns of the view rotation
  float p00, p11;        // proj[0][0], proj[1][1]
  const float* dvx;      // [W] view-space ray direction x per column, [H] y per frame row (launch_ray_tables)
  const float* dvy;
  float PV[16];          // proj * view (host product, fixed order)
  float tmax;
  uint32_t* vis;
  float4* worldpos;
  float* depth;
  float4* normals;            // nullable: per-pixel normal_tab[id] for the LDS-staged filter of large scenes
  const float4* normal_tab;   // per-id (n.xyz, self weight), built by k_lut
  const float4* area_tab;     // per-id (area of LUT[id], 0, 0, 0), built by k_lut (K1 in the same launch)
  int32_t cull;                      // 1: bounds[] is valid
  // K1 in the same launch (rtpt_temporal_gradient arrived right behind rtpt_gbuffer): the pixel's id and world position
  // are still in registers, so the gradient costs its 16 B/px store and none of its 20 B/px of loads
  int32_t grad_on;
  int32_t grad_y0, grad_y1;          // rows the gradient was asked for
  float g_cam[3], g_light[3], g_light_prev[3], g_color[3], g_color_prev[3];
  const float4* lut;
  const float4* lut_prev;
  float4* grad;
  TriBounds bounds[kCullMaxTris];
};

struct LutArgs {
  uint32_t n_tris;
  const float4* shade;  // world-space vertices
  float model[16];
  float4* lut;          // (n+1) x 3 float4 (stride 48 B)
  float4* normal_tab;   // (n+1) float4: xyz = unit normal of LUT[id] (id 0: (0,0,1)), w = self weight
  float4* area_tab;     // (n+1) float4: x = tri_area(LUT[id]) — the denominator of the area-ratio barycentrics
                        // (temporalGradient.comp.glsl:60), a per-triangle value K1 used to recompute per pixel
  float* pair_tab;      // (n+1)^2 pow(max(0,dot(n_p,n_q)),sigma_n), NULL when n+1 > 64
  int32_t sigma_n;
};

struct GradientArgs {
  FrameGeom g;
  float cam[3], light[3], light_prev[3], color[3], color_prev[3];
  const uint32_t* vis;
  const float4* worldpos;
  const float4* lut;
  const float4* lut_prev;
  const float4* normal_tab;  // per-id normals of the current LUT (k_lut)
  const float4* area_tab;    // per-id triangle areas of the current LUT (k_lut)
  float4* grad;
};

struct PathtraceArgs {
  FrameGeom g;
  SceneView scene;
  uint32_t frame, batch;
  uint32_t max_segments, spp;
  float cam[3];
  float light_c[3];
  float light_col[3];        // currentCameraColor * intensity
  float light_col_first[3];  // light_col / first_hit_light_divisor
  float light_r2;            // radius * radius
  float slope, jitter, ray_offset, tmax;
  float4* image;        // written as (rgb, depth): see atrous.hip "rgbd"
  const float* depth;   // G-buffer depth of the same pixels
  uint32_t* hit_id;  // nullable
  float4* albedo;    // nullable.  RTPT_FLAG_EXT_DEMODULATE: segment 0 stores (albedo of the hit, 0) here — (1, 1, 1, 0) when the path
                     // ends at that query — instead of multiplying it into the throughput
  unsigned long long* raycount;
  int32_t count_y0, count_y1;  // rows whose queries are counted
  int32_t compact;             // 1: compact surviving paths to the front of the block after every segment
  int32_t cull;                // 1: bounds[] is valid for the primary segment
  int32_t n_cu;                // compute units of the context's device (persistent queue-kernel grid)
  uint32_t multi_off;          // dword offset of the spp > 1 accumulators in dynamic LDS (set by launch_pathtrace)
  uint32_t tiles_y;            // rows of tiles of the traced rows (set by launch_pathtrace; the fused launch's grid is taller)
  void* pool_slab;             // path-pool form of the tile kernel (kernels.hip: k_pathtrace_pool): pathtrace_pool_bytes() of
                               // scratch owned by the context, or NULL
  // long paths (spp == 1, max_segments > 4): a launch covers the segment window [seg_begin, seg_end) and hands the
  // unfinished paths to the next one through a queue of 48-byte records (set by launch_pathtrace)
  uint32_t seg_begin, seg_end;
  uint32_t first_window;       // segments the tile kernel runs before it hands the survivors to the queue kernels (0: pt_first_window())
  void* q_out;                 // records written by this launch
  uint32_t* q_out_count;
  const void* q_in;            // records read by k_pathtrace_queue
  const uint32_t* q_in_count;
  // queue storage owned by the context: two buffers of `queue_capacity` records and two counters, or NULL
  void* queue[2];
  uint32_t* queue_count;       // [2][kPathQueues]
  uint32_t queue_region;       // records per region (a queue buffer holds kPathQueues regions)
  TriBounds bounds[kCullMaxTris];
};

struct AtrousArgs {
  FrameGeom g;
  int32_t k;             // tap stride = waveletIteration
  int32_t exact;         // 1: contract arithmetic for the weights (RTPT_FLAG_EXACT_FILTER)
  int32_t direct;        // 1: force the direct-load kernel (no LDS staging)
  int32_t rows_stored;   // rows held by the planes (row_base .. row_base+rows_stored-1)
  int32_t cwp;           // comb kernel: staged row length in cells (set by launch_atrous)
  int32_t n_cu;          // compute units of the context's device (persistent grid size)
  int32_t alpha_zero;    // 1: a k < N launch writes alpha 0 instead of the depth (last iteration of an even N)
  int32_t n_strips, n_segs, seg_rows;  // chained iterations (atrous_chain.hip): column strips x row segments (set by launch_atrous_chain)
  int32_t strip_w;       // chained iterations: columns a strip stores (set by launch_atrous_chain; at most 128 - 2 * sum of the later strides)
  const float* pair_tab; // (n_tris+1)^2 id-pair normal weights, NULL when the scene is too large
  const float4* normals; // per-pixel (n.xyz, self weight) plane written by k_gbuffer for such scenes, NULL otherwise
  uint32_t n_tris;       // normal_tab has n_tris + 1 entries
  int32_t sigma_n;
  float cz, cl;          // fast path: -log2(e)/sigma_z, -log2(e)/sigma_l (set by launch_atrous)
  int32_t tiles_x, tiles_y;  // 64x4 tiles covering [y0,y1) (set by launch_atrous)
  float sigma_z, sigma_l;
  const float4* in;
  float4* out;
  const uint32_t* vis;
  const float4* normal_tab;
  // final pass only
  uint32_t frame;
  float alpha;
  const float4* worldpos;
  const float4* history;
  const float4* lut_prev;
  float PVprev[16];
  int2* prev_pixel;      // nullable
  int32_t hist_row_base;          // first frame row stored by the history plane
  int32_t hist_y0, hist_y1;       // frame rows of the history plane that hold a valid previous frame
  // extension modes (RTPT_FLAG_EXT_*; 0 = the reference's filter).  Any bit routes to k_atrous_ext.
  uint32_t ext;
  int32_t stride;                 // tap stride (k, or 2^(k-1) with RTPT_FLAG_EXT_POW2_STRIDE)
  const float4* gradient;         // K1 output (adaptive alpha)
  const uint32_t* prev_vis;       // previous frame's id plane, rows [pvis_y0,pvis_y1) valid, stored from pvis_row_base
  int32_t pvis_y0, pvis_y1, pvis_row_base;
  // final pass only, optional: the swapchain blit (main.cpp:1338-1361) fused into the pass — rows [present_y0, present_y1)
  // of the blended frame are also written as B8G8R8A8_UNORM to present (first byte = pixel (0, present_y0)); rtpt_present_target
  uint32_t* present;
  int32_t present_y0, present_y1;
  const float* var_scale;         // RTPT_FLAG_EXT_SVGF_VARIANCE: the 3x3-prefiltered variance that scales the luminance weight of
                                  // the centre pixel (k_var_prefilter of var_in); NULL: var_in's own value
  const float* var_in;            // RTPT_FLAG_EXT_VARIANCE: per-pixel luminance variance read by this iteration
  float* var_out;                 //                         ... and the filtered variance it writes
  // final pass of the plain comb kernel only (atrous_final_plain_comb): the reprojected pixel of every output pixel, packed
  // ppy << 16 | ppx, 0xFFFFFFFF when it lies outside the frame (history_at reads 0 there either way); indexed like every plane.
  // reproj_out: the pass also stores it; reproj_in: the pass reads it INSTEAD of reprojecting (never both)
  uint32_t* reproj_out;
  const uint32_t* reproj_in;
};

// RTPT_FLAG_EXT_VARIANCE: temporal accumulation of the luminance moments before the first filter iteration
struct MomentsArgs {
  FrameGeom g;
  uint32_t frame;
  float alpha;
  const float4* traced;
  const uint32_t* vis;
  const float4* worldpos;
  const float4* lut_prev;
  float PVprev[16];
  const uint32_t* prev_vis;     // previous frame's ids and moments: frame rows [hist_y0, hist_y1), stored from hist_row_base
  const float4* moments_prev;
  int32_t hist_row_base, hist_y0, hist_y1;
  int32_t svgf;         // RTPT_FLAG_EXT_SVGF_VARIANCE: spatial estimate for histories shorter than 4 frames
  int32_t rows_stored;  // rows the planes hold from g.row_base on: the 7x7 estimate never reads beyond them (strips trace 3
                        // rows more than their filter needs, so every variance that is consumed saw its whole window)
  float4* moments_out;  // (m1, m2, n, var)
  float* var_out;
};
void launch_moments(const MomentsArgs& a, hipStream_t s);
// RTPT_FLAG_EXT_SVGF_VARIANCE: out = 3x3 Gaussian (1 2 1 / 2 4 2 / 1 2 1) / 16 of var, frame-clamped, rows [g.y0, g.y1)
void launch_var_prefilter(const FrameGeom& g, int rows_stored, const float* var, float* out, hipStream_t s);

// Long paths: segments handled by the tile kernel before the survivors are queued; every later window is twice as
// long.  Swept at 4K on the Cornell box (k_pathtrace, 8 / 16 / 32 segments; single launch 969 / 1627 / 2843 us):
// 2: 1028 / 1376 / 1622, 3: 893 / 1246 / 1489, 4: 836 / 1186 / 1421, 6: 891 / 1238 / 1494.  BVH scenes use twice the
// window: the queue order is the order of arrival, not of the image, and the lost ray coherence costs the traversal
// more than the denser waves win (1.15M triangles, 8 segments: 3.65 -> 3.80 ms with a window of 4).  Windows shorter
// than the BASELINE configs' 4 segments lose everywhere, also on the 270-row strip of an 8-rank job (k_pathtrace
// 89 us in one launch, 108 / 115 us with windows of 3 / 2): the hand-over costs more than the drain tail it removes.
constexpr uint32_t kPtPhase0 = 4, kPtBvhMult = 2;
inline uint32_t pt_first_window(bool use_bvh) { return use_bvh ? kPtBvhMult * kPtPhase0 : kPtPhase0; }
// regions (and counters) per queue buffer.  1 / 8 / 16 / 64 regions: reference frame 352 / 403 / 421 / 418 us, 4K 32 segments
// 1421 / 1434 / 1441 / 1429
constexpr uint32_t kPathQueues = 1;

constexpr uint32_t kRayCounters = 256;  // RAYCOUNT is kept as this many partial sums (power of two), added up at readback

constexpr uint32_t kExtAdaptiveAlpha = 0x10u, kExtGauss5 = 0x20u, kExtPow2Stride = 0x40u, kExtDisocclusion = 0x80u;
constexpr uint32_t kExtVariance = 0x100u;
constexpr uint32_t kExtSvgfVariance = 0x800u;  // with kExtVariance: spatial estimate for short histories + 3x3 prefilter
constexpr uint32_t kExtMask = 0x9F0u;

struct ScenePrepArgs {
  uint32_t n_tris;
  const float* tris;  // n x 9 world-space floats
  const uint32_t* leaf_order;
  float4* isect_id;
  float4* isect_leaf;
  float4* shade;
  uint32_t leaf_pairs;  // the BVH was built over fan pairs: isect_leaf holds one 80-byte record per pair (SceneView::isect_leaf)
};

void launch_scene_prepare(const ScenePrepArgs& a, hipStream_t s);

// device-side re-pose + BVH refit (refit.hip)
struct RefitModel {
  float m[16];       // column-major model matrix (rtpt_ubo::model)
  int32_t identity;  // 1: copy the vertices
};
struct RefitArgs {
  const float* tris;           // posed triangles, n x 9
  const uint32_t* leaf_order;  // leaf slot -> triangle id
  const uint32_t* order;       // node indices sorted by height (children before parents)
  BvhNodeQ* nodes;             // device nodes: references are read, boxes rewritten
  float* fbox;                 // n_nodes x 12 floats: unpadded binary32 child boxes (scratch)
  float* grid;                 // 8 floats: origin xyz, cell xyz, pad, 0
};
void launch_pose(uint32_t n_verts, const float* src, float* dst, const RefitModel& m, hipStream_t s);
// the cofactor table of smooth shading (shading_normal.hpp: cof_rows; NormalView::cof), three float4 per instance, from the model
// and the instance transforms as they stand on the stream (xf: n_instances x 12 floats on the device, or NULL: one instance, the
// model's own linear part); no synchronisation
void launch_normal_cof(uint32_t n_instances, const float* xf, const RefitModel& m, float4* cof, hipStream_t s);
// level_first[h] .. level_first[h + 1]: the slice of `order` holding the nodes of height h (n_levels + 1 entries)
void launch_refit(const RefitArgs& a, const uint32_t* level_first, int n_levels, uint32_t n_nodes, float pad_rel, hipStream_t s);
// device-side flatten + fan-pair test (scene_flatten.hip): mesh x instance transforms -> the un-posed triangles
struct FlattenArgs {
  uint32_t n_tris;       // triangles of the mesh
  uint32_t n_out_verts;  // 3 x n_tris x instances
  const float* xyz;      // mesh vertices
  const uint32_t* idx;   // 3 x n_tris vertex indices, each below the vertex count
  const float* xf;       // instances x 12 floats (3x4 row-major), or NULL: one identity instance, the vertices are copied
  float* out;            // n_out_verts x 3 floats, triangle id = instance * n_tris + t
};
void launch_flatten(const FlattenArgs& a, hipStream_t s);
// *all_paired (preset to 1 by the caller) is cleared when some (2q, 2q + 1), q < n_pairs, is not a fan pair bit for bit
void launch_fan_pairs(uint32_t n_pairs, const float* tris, uint32_t* all_paired, hipStream_t s);
// device-side LBVH build (bvh_build.hip): the topology only — launch_refit + launch_scene_prepare fill boxes, grid and records
constexpr uint32_t kLbvhMaxLevels = 128;                  // heights the histogram distinguishes (63 + 32 key bits: at most 95)
constexpr uint32_t kLbvhHeaderWords = 2 + kLbvhMaxLevels;  // [0] depth, [1] nodes, [2 + h] nodes of height h: ONE readback
struct LbvhArgs {
  uint32_t n_prims;       // primitives: fan pairs (2q, 2q + 1) when prim_w == 2, triangles when 1
  uint32_t prim_w;
  const float* tris;      // n_prims x prim_w x 9 world-space floats
  BvhNodeQ* nodes;        // max(n_prims - 1, 1) nodes: references set, boxes zero
  uint32_t* leaf_order;   // n_prims x prim_w
  uint32_t* refit_order;  // the nodes sorted by height
  uint32_t* header;       // kLbvhHeaderWords
  uint32_t by_height;     // A/B: number the nodes by descending height instead of pre-order (RTPT_LBVH_ORDER=height)
};
size_t lbvh_scratch_bytes(uint32_t n_prims, bool by_height);  // 0: the sort's size query failed
hipError_t launch_lbvh_build(const LbvhArgs& a, void* scratch, size_t scratch_bytes, hipStream_t s);
// device-side SAH build (bvh_build_sah.hip): the host builder's tree, node for node; the same outputs in the same formats
// (nodes: at most n_prims - 1 are written, header[1] says how many; by_height is ignored).  Synchronises the stream once at
// the start and one to three times per level of the tree (three while a level still has segments larger than a workgroup).
size_t sah_scratch_bytes(uint32_t n_prims);  // 0: the sort's size query failed
hipError_t launch_sah_build(const LbvhArgs& a, void* scratch, size_t scratch_bytes, hipStream_t s);
// gather isect records into class order: out[t] = isect_id[ids[t]] (3 float4 each), n entries
void launch_lut(const LutArgs& a, hipStream_t s);
// normals.guide != 0 (RTPT_FLAG_EXT_SMOOTH_GUIDE is active: the scene holds normals, so it traces through its tree, and a.normals is
// the per-pixel plane): the BVH-mode instantiation with a NormalView, which writes the guide normal there.  Every other launch is the
// kernel without one.
void launch_gbuffer(const GbufferArgs& a, hipStream_t s, const NormalView& normals = NormalView{nullptr, nullptr, 0u, 0});
void launch_ray_tables(int W, int H, float p00, float p11, float* dvx, float* dvy, hipStream_t s);
void launch_gradient(const GradientArgs& a, hipStream_t s);
// gb != NULL: K0 (+ K1) of gb's rows run inside the tile kernel's launch, behind the tracing tiles (pathtrace_fuses_gbuffer says
// whether they can; pathtrace_grid_blocks = the workgroups of that launch, what the BVH stack's spill area is sized for)
// specular: the launch's SPEC (the block of kSpecNee above) — what selects the SPEC instantiations; it travels beside the kernel
// arguments, not in them, so that every existing argument offset stays.  A launch that samples lights (spec_lights) runs every
// segment in the tile kernel (no queue kernels) and carries no final pass.
// lights: the light list in its host form, handed to a kernel as spec_lights_t<SPEC> says: not at all, as a LightView (its first
// two fields) or whole.  It has entries where the launch samples the list's triangles (with spec_sphere alone it may be empty),
// and a table (cdf) where it picks by weight (spec_power).
// normals: the scene's vertex normals (rtpt_scene_set_normals), records NULL without: with them the scene traces through its BVH, the
// unfused launch compacts, and the launch carries no final pass.
// envmap: the context's environment (rtpt_set_environment), texels NULL without: with it the launch is fused or compacts, runs every
// segment in the tile kernel and carries no final pass (the ENV axis above).
// fin != NULL (then gb == NULL and pol != NULL): the launch also holds the workgroups of the final filter pass `fin`, which
// atrous_final_role finished — in front of and behind the tracing tiles as pol says (kernels.hip: k_pathtrace_final).
// pathtrace_takes_final says whether the launch can carry one: the brute-force tile kernel, one sample, no albedo plane, no
// textures, no specular bounce
// run_info (optional, 3 words): the tile columns the launch serves as ordinary tiles, its run workgroups and the tiles those serve
// (final_split.hpp; a launch without runs: every column, 0, 0)
struct FilterPolicy;
void launch_pathtrace(const PathtraceArgs& a, const GbufferArgs* gb, const TexView& tex, int specular, hipStream_t s, const AtrousArgs* fin = nullptr,
                      const FilterPolicy* pol = nullptr, uint32_t* run_info = nullptr,
                      const LightTableView& lights = LightTableView{nullptr, 0u, nullptr},
                      const NormalView& normals = NormalView{nullptr, nullptr, 0u, 0}, const EnvView& envmap = EnvView{});
// the instantiations of the ENV axis (kernels_env.hip), in five parts so that they compile side by side: scene mode 0; mode 1
// without and with a NormalView; mode 2 without and with one.  launch_pathtrace finishes the arguments (b: tiles_y, multi_off and
// the segment window set; spec: the launch's SPEC; dyn: its dynamic LDS) and calls the part of its scene; nothing else does.
#define RTPT_ENV_PART_DECL(p)                                                                                                          \
  void launch_pathtrace_env_p##p(const PathtraceArgs& b, const GbufferArgs* gb, const TexView& tex, int spec, dim3 grid, dim3 block, \
                                 size_t dyn, hipStream_t s, const LightTableView& lights, const NormalView& normals, const EnvView& envmap)
RTPT_ENV_PART_DECL(0);
RTPT_ENV_PART_DECL(1);
RTPT_ENV_PART_DECL(2);
RTPT_ENV_PART_DECL(3);
RTPT_ENV_PART_DECL(4);
bool pathtrace_takes_final(const PathtraceArgs& a, const TexView& tex, int specular);
bool pathtrace_fuses_gbuffer(const PathtraceArgs& a, const GbufferArgs& g);
uint32_t pathtrace_grid_blocks(const PathtraceArgs& a, const GbufferArgs* gb);
bool pathtrace_uses_pool(const PathtraceArgs& a);
size_t pathtrace_pool_bytes(int W, int rows);
// px_normals (RTPT_FLAG_EXT_SMOOTH_GUIDE is active and a.normals covers the rows read; then a.pair_tab is NULL): the normals of a
// tap are the two pixels' cells of a.normals in every kernel — the comb kernel's NRM form, or the per-pixel instantiation of the
// two direct-load kernels where today's launch reads normal_tab by id.  It travels beside the arguments, like launch_pathtrace's
// `specular`: AtrousArgs and the argument segment of every filter kernel stay what they were.
void launch_atrous(const AtrousArgs& a, bool final_pass, hipStream_t s, bool px_normals = false);
bool atrous_final_fuses_present(const AtrousArgs& a);
// true when a launch of `a` runs in the plain comb kernel (no extension mode, not forced direct, 1 <= k <= 16, id-pair table
// or per-pixel normals): the only kernel whose final pass takes reproj_out / reproj_in
bool atrous_final_plain_comb(const AtrousArgs& a);
// The final pass `a` as workgroups of a tracing launch (launch_pathtrace's fin): true when the comb body is instantiated for it
// there — id-pair table, the fast weights, a stride whose halo fits that launch's LDS (atrous_comb.hpp: kFinalRoleMaxK), the
// reprojected pixels loaded (reproj_in), neither prev_pixel nor present — and then the members a launch sets (cz, cl, tiles)
// are filled in
bool atrous_final_role(AtrousArgs& a);
// `levels` consecutive iterations k, k+1, .. in one launch, intermediates in LDS (atrous_chain.hip): a.k = the first
// stride, a.in / a.out = input of the first and output of the last iteration (distinct buffers), final_pass = the last
// level is the frame's FINAL pass (reprojection + blend)
// launch policy switches of the filter kernels, read from the environment ONCE per context (rtpt_create) — A/B runs and the
// tests that pin a variant set them before creating the context; 0 = the shipped choice
// FilterPolicy::empty_run, the built-in R.  4K frame at rest, one job, ms per frame / us of the tracing launch
// (profiles/r20_empty_runs_ab.txt): parent 0.5876, 0.5895 / 409.2, 411.2; R = 0 0.5874 / 409.5; 2 0.5717 / 393.5; 4 0.5709,
// 0.5726 / 392.7, 393.7; 8 0.5713, 0.5722 / 392.7, 393.7; 16 0.5731, 0.5743 / 394.6, 395.9; 32 0.5806 / 401.9.  4 and 8 do not
// differ; 8 has half the workgroups, and on a frame of nothing but sky 8 tiles per workgroup run 2.9 times as fast as one.
constexpr int kEmptyRunTiles = 8;
struct FilterPolicy {
  int chain_g_pin = 0;      // RTPT_CHAIN_G1: rows per level and step of a chained pair (2, 3, 4)
  int chain_generic = 0;    // RTPT_CHAIN_GENERIC: the instantiation that reads its strides instead of having them compiled in
  int chain_wg_per_cu = 0;  // RTPT_CHAIN_WG_PER_CU: workgroups per CU the row segments are sized for
  int chain_sw = 0;         // RTPT_CHAIN_SW: the sliding-window form of the pair (round 3, slower)
  int chain_sw_g1 = 0, chain_sw_g3 = 0;  // RTPT_CHAIN_SW_G1 / _G3: its rows per step
  // RTPT_CHAIN_SKEW: percent by which the row segments of a chained launch differ with the age of their workgroups on a CU
  // (atrous_chain.hip: chain_segments), "a" or "a,b": a for four workgroups per CU, b for two or three; -1 = the built-in values
  int chain_skew = -1, chain_skew2 = -1;
  int chain_bw = 0;         // RTPT_CHAIN_BW: columns a strip of the pair (1,2) stores (A/B; 0 = the widest, 124)
  // RTPT_FINAL_FRONT=<front>[,<percent of the work list>]: the filter workgroups of a tracing launch
  // that carries the previous frame's final pass (kernels.hip: k_pathtrace_final; final_split.hpp has the layout).  <front>: the
  // group dispatched in FRONT of the tiles, 1 .. 7 workgroups per CU or, from 8 on, a total number of workgroups (a multiple of
  // 8); 0 = none.  The second field is the percent of the list the front group owns; the rest runs behind the tiles, where its
  // workgroups start when the launch is all but over.  Left out (-1): the whole list on a frame as large as 4K, 75 % on one
  // as small as 1080p (final_split.hpp: kFinalWholeListItems).  Built-in: 1 per CU.  4K frame at rest, one job
  // (profiles/r19_final_place_ab.txt): parent (1 per CU, 75 %) 0.5935-0.5945 ms; whole list with 128 / 192 / 256 / 512
  // workgroups in front 0.678 / 0.586 / 0.587 / 0.587 (128 workgroups outlast the tiles; 192 and 256 differ by less than the
  // spread of a setting, and 256 leaves the group 160 us of the launch to spare where 192 leaves 85); 90 / 80 / 70 % in front
  // of 256 with the rest behind the tiles 0.590 / 0.595 / 0.600.  1080p: parent 0.1705-0.1712; 100 / 90 / 80 / 75 % 0.1728 /
  // 0.1722 / 0.1711 / 0.1712.  A third group in front of the sky tiles (the last three eighths dispatched) recovered 3-5 us of
  // what the tail loses at 4K and stayed behind the whole list in front; it was removed.
  int final_front = 1, final_front_share = -1;
  // RTPT_EMPTY_RUN=<R>: in that launch, the tile columns at the end of the dispatch order that no triangle's screen bounds reach
  // are served R vertically consecutive tiles per workgroup (final_split.hpp, pathtrace_tile.hpp: pathtrace_empty_run); 0 = one
  // workgroup per tile, as every other column.  kEmptyRunTiles has the sweep.
  int empty_run = kEmptyRunTiles;
};
void launch_atrous_chain(const AtrousArgs& a, int levels, bool final_pass, const FilterPolicy& pol, hipStream_t s);
bool atrous_chain_supported(int k0, int levels, uint32_t n_tris);
hipError_t prepare_device_atrous_chain();
hipError_t prepare_device_atrous();  // per device, from rtpt_create: raises the dynamic-LDS limit of the staged filter kernels
void launch_stamp_depth(const FrameGeom& g, float4* color, const float* depth, hipStream_t s);
// swapchain blit (main.cpp:1338-1361): rows [g.y0,g.y1) of `image` -> B8G8R8A8_UNORM at dst (first byte = pixel (0, g.y0))
// albedo != NULL (RTPT_FLAG_EXT_DEMODULATE): the bytes are the conversion of (image.rgb * albedo.rgb, 0), each product rounded to
// binary32 first
void launch_present(const FrameGeom& g, const float4* image, const float4* albedo, uint32_t* dst, hipStream_t s);
// RTPT_FLAG_EXT_DEMODULATE: shaded = (image.rgb * albedo.rgb, 0) over rows [g.y0,g.y1)
void launch_modulate(const FrameGeom& g, const float4* image, const float4* albedo, float4* shaded, hipStream_t s);
void launch_selftest_math(int op, const float* in, float* out, size_t n, hipStream_t s);
void launch_selftest_exhaustive(int op, unsigned long long* out, hipStream_t s);
void launch_selftest_div(int mode, uint32_t pass, unsigned long long* out, hipStream_t s);
void launch_selftest_trace(const SceneView& scene, const float* rays, size_t n, float tmax, uint32_t* out_id,
                           float* out_t, hipStream_t s);
// rtpt_selftest_contract: {input words, output words} per item of every fn (the table of include/rtpt.h, in its order)
constexpr int kContractFns = 23;
constexpr uint32_t kContractWords[kContractFns][2] = {
    {6, 1},  {6, 3},  {3, 1},  {3, 3},  {2, 1},  {1, 1},  {2, 2},  {4, 1},  {1, 3},  {1, 2},  {1, 1},  {1, 1},
    {19, 4}, {2, 1},  {3, 2},  {9, 1},  {12, 3}, {13, 3}, {12, 3}, {36, 2}, {10, 1}, {3, 3},  {3, 6}};
void launch_selftest_contract(int fn, const uint32_t* in, uint32_t* out, size_t n, hipStream_t s);
// spec::bounce (specular.hpp) on n cases of 9 floats (d, n, u1, u2, g): out = n x (d', absorbed as 1.0f / 0.0f)
void launch_selftest_bounce(const float* in, float* out, size_t n, hipStream_t s);
// diel::refract (dielectric.hpp) on n cases of 9 floats (d, n, u1, u2, ior): out = n x (d', transmitted as 1.0f / 0.0f, F)
void launch_selftest_refract(const float* in, float* out, size_t n, hipStream_t s);
// light::pick and light::sample (light_sample.hpp) on n cases of 19 words (v0, v1, v2, x, nf, u_l, u_a, u_b, L): out = n x (y, wd,
// g, valid as 1.0f / 0.0f, the picked entry)
void launch_selftest_light_sample(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s);
// light::sphere_sample on n cases of 12 words (x, nf, c, r2, u_c, u_p): out = n x (wd, g, taken, valid), 6 words
void launch_selftest_sphere_sample(const uint32_t* in, uint32_t* out, size_t n, hipStream_t s);
// light::hit_weight, light::mis_bounce and light::mis_light (light_sample.hpp: RTPT_FLAG_EXT_NEE_MIS) on n cases of 20 words (v0, v1,
// v2, o, d, b1, b2, cb, inv_p, one word not read): out = n x (g_hit, wb(g_hit), g_hit * m(g_hit))
void launch_selftest_mis_weight(const float* in, float* out, size_t n, hipStream_t s);
// shading_normal.hpp's rules and side tests on n cases of 36 words (n0, n1, n2, b1, b2, the cof rows, ng, d, d', wd, ray_offset, three
// words not read): out = n x (smooth as 1.0f / 0.0f, ns, absorbed, sample_side, the dielectric's offset, 0)
void launch_selftest_shading_normal(const float* in, float* out, size_t n, hipStream_t s);
// env::color (env.hpp) of n directions of 3 floats: rgb_out = n x 3 (rtpt_selftest_environment)
void launch_selftest_environment(const EnvView& envmap, const float* dirs, size_t n, float* rgb_out, hipStream_t s);
// rtpt_light::find (light_list_host.hpp) of k queries on the ascending list ids[0, n): index_out[j], n where the id is not in it
void launch_selftest_light_find(const uint32_t* ids, uint32_t n, const uint32_t* queries, size_t k, uint32_t* index_out, hipStream_t s);

// The cumulative table of RTPT_FLAG_EXT_NEE_POWER (light_table.hip; light_sample.hpp states the arithmetic): everything on stream
// s, no synchronisation, no readback.  kLightTableBlock entries per workgroup; light_table_scratch_bytes(n) = what the builder
// needs beside the table for n entries: the maximum's word (8 bytes), the sums of the workgroups of every level of the scan
// (8 bytes each: ceil(n / 1024), ceil(that / 1024), ... down to one workgroup) and the weights (4 n).
constexpr uint32_t kLightTableBlock = 1024;
size_t light_table_scratch_bytes(size_t n);
// ... of the light list ids[0, n) of a scene: the weights come from the shade records and the material records
struct LightTableArgs {
  const uint32_t* ids;
  uint32_t n;
  const float4* shade;
  const float4* materials;
  uint32_t n_base_tris;
  uint64_t* cdf;  // n entries
  void* scratch;  // light_table_scratch_bytes(n)
};
void launch_light_table(const LightTableArgs& a, hipStream_t s);
// ... of n given weights w (a device pointer): rtpt_selftest_light_table
void launch_light_table_weights(const float* w, size_t n, uint64_t* cdf, void* scratch, hipStream_t s);
// light::pick_power on k draws u_l of the table cdf[0, n): index_out[j], inv_p_out[j] (rtpt_selftest_light_pick)
void launch_selftest_light_pick(const uint64_t* cdf, uint32_t n, const float* u_l, size_t k, uint32_t* index_out, float* inv_p_out, hipStream_t s);
// tex::sample of descriptor `desc` (a device pointer) at n uv pairs: out[i] = the RGBA the kernels would read
void launch_selftest_texture(const TexDesc* desc, const float4* texels, const float* uv, size_t n, float4* out, hipStream_t s);
// tex::sample_lod of descriptor `desc` and its level-table row `lv` (device pointers) at n (uv, lod) pairs
void launch_selftest_texture_lod(const TexDesc* desc, const uint32_t* lv, const float4* texels, const float* uv, const float* lod, size_t n,
                                 float4* out, hipStream_t s);
// launch_selftest_trace, returning instead of t the level hit_texture_lod gives the hit, clamped to its chain (0 without one)
void launch_selftest_footprint(const SceneView& scene, const TexView& tex, const float* rays, size_t n, float tmax, bool primary, float slope,
                               int frame_h, uint32_t* out_id, float* out_lod, hipStream_t s);

}  // namespace rt
