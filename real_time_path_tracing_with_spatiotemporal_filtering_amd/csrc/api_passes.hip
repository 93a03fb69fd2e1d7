// api_passes.hip — one entry point per reference dispatch (K0 rtpt_gbuffer, K1 rtpt_temporal_gradient, K2 rtpt_raytrace,
// K3 rtpt_temporal_filter, K4 rtpt_end_frame, the swapchain blit rtpt_present) and what they record: K0 / K1 until K2 arrives,
// the filter iterations until the last one arrives (api_internal.hpp: FLUSH_FILTER).
#include "api_internal.hpp"

namespace rtpt_impl {
void reuse_invalidate(rtpt_ctx* c, const Buf* b) {
  auto kill = [&](auto& tag, const Buf* of) {
    if ((!b || b == of) && tag.valid) {
      tag.valid = false;
      c->reuse_info[3]++;
    }
  };
  kill(c->tag_vis[0], &c->vis[0]);
  kill(c->tag_vis[1], &c->vis[1]);
  kill(c->tag_worldpos, &c->worldpos);
  kill(c->tag_depth, &c->depth);
  kill(c->tag_normals, &c->normals);
  kill(c->tag_gradient, &c->gradient);
  // K1 reads both LUT buffers, and their version does not see a write through a pointer handed out
  const bool lut = b == &c->scene.lut[0] || b == &c->scene.lut[1];
  if (lut) kill(c->tag_gradient, b);
  // the cached reprojection was computed from the world positions, the ids and a LUT: it dies with any of them (its own
  // counter: rtpt_debug_reproj_info), and the next final pass starts a new run of equal keys
  if (!b || lut || b == &c->worldpos || b == &c->vis[0] || b == &c->vis[1]) {
    if (c->tag_reproj.valid) c->reproj_info[2]++;
    c->tag_reproj.valid = false;
    c->reproj_last.valid = false;
  }
}
}  // namespace rtpt_impl

namespace rtpt_impl {
// k_lut (+ k_pair_weights): the LUT of the current frame and the per-id tables (normals, self weights, areas, id-pair
// weights) of the posed scene.  The device triangles are already posed, so the kernel's own model is the identity.
// rtpt_gbuffer calls this when the pose changed; rtpt_temporal_filter when it arrives first (it reads the tables).
void build_tables(rtpt_ctx* c) {
  Timer tm(c, RTPT_K_LUT);
  rt::LutArgs la;
  la.n_tris = c->scene.n_tris;
  la.shade = static_cast<const float4*>(c->scene.shade.ptr);
  for (int i = 0; i < 16; i++) la.model[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  la.lut = static_cast<float4*>(c->scene.lut[c->lut_cur].ptr);
  la.normal_tab = static_cast<float4*>(c->scene.normal_tab.ptr);
  la.area_tab = la.normal_tab + (c->scene.n_tris + 1);
  la.pair_tab = static_cast<float*>(c->scene.pair_tab.ptr);
  la.sigma_n = c->cfg.sigma_n;
  rt::launch_lut(la, c->stream);
  c->scene.lut_version[c->lut_cur] = c->scene.model_version;
  c->tables_valid = true;
}

// D3: visibilityLUTprevious is read during frame 0 (K1, the final filter pass) before anything wrote it; define it as LUT
static int seed_lut_prev(rtpt_ctx* c) {
  if (c->scene.lut_prev_valid) return RTPT_OK;
  HIP_TRY(hipMemcpyAsync(c->scene.lut[c->lut_cur ^ 1].ptr, c->scene.lut[c->lut_cur].ptr, c->scene.lut[c->lut_cur].bytes, hipMemcpyDeviceToDevice,
                         c->stream));
  c->scene.lut_prev_valid = true;
  c->scene.lut_version[c->lut_cur ^ 1] = c->scene.model_version;
  return RTPT_OK;
}

// the tables and LUT of the current pose (when `stale`), then the LUTprevious: rtpt_gbuffer's and ensure_tables's common path
static int refresh_tables(rtpt_ctx* c, bool stale) {
  if (stale) build_tables(c);
  int rc = launch_check("lut");
  return rc ? rc : seed_lut_prev(c);
}

// A pass that reads the per-id tables (normals, areas, id-pair weights) without rtpt_gbuffer in front of it — rtpt_temporal_filter
// or the stand-alone rtpt_temporal_gradient as the first pass after rtpt_scene_upload or rtpt_scene_set_instances (a changed
// ubo.model arrives only with rtpt_gbuffer, which rebuilds them in the same call) — builds them here, with the LUT of the
// current pose
int ensure_tables(rtpt_ctx* c) {
  if (c->tables_valid) return RTPT_OK;
  FLUSH_FILTER(c);
  HIP_TRY(hipSetDevice(c->device));
  return refresh_tables(c, true);
}
}  // namespace rtpt_impl

namespace {

// the key of the K0 call `a` was built for (api_internal.hpp: K0Key)
K0Key gbuffer_key(const rtpt_ctx* c, const rt::GbufferArgs& a) {
  K0Key k = new_key<K0Key>();
  std::memcpy(k.org, a.org, sizeof k.org);
  std::memcpy(k.c0, a.c0, sizeof k.c0);
  std::memcpy(k.c1, a.c1, sizeof k.c1);
  std::memcpy(k.c2, a.c2, sizeof k.c2);
  std::memcpy(k.PV, a.PV, sizeof k.PV);
  k.p00 = a.p00;
  k.p11 = a.p11;
  k.tmax = a.tmax;
  k.W = a.g.W;
  k.H = a.g.H;
  k.row_base = a.g.row_base;
  k.y0 = a.g.y0;
  k.y1 = a.g.y1;
  k.normals_on = a.normals ? 1 : 0;
  k.guide = (a.normals && guide_active(c)) ? 1 : 0;  // (the normals themselves: rtpt_scene_set_normals drops the plane's tag)
  k.guide_sigma_n = k.guide ? c->cfg.sigma_n : 0;
  k.model_version = c->scene.model_version;
  k.scene_gen = c->scene_gen;
  return k;
}

// the planes K0 (+ K1 when a.grad_on) of `a` writes now carry `key`; NULL, or a plane the context does not own (its owner can
// write it unseen): they carry nothing
void tag_outputs(rtpt_ctx* c, const rt::GbufferArgs& a, const K1Key* key) {
  auto set = [&](auto& tag, const Buf& b, const auto* k) {
    if (tag.valid) c->reuse_info[3] += (!k || !b.owned) ? 1 : 0;
    tag.valid = k && b.owned && c->frame_reuse;
    if (tag.valid) tag.key = *k;
  };
  const K0Key* k0 = key ? &key->k0 : nullptr;
  for (int i = 0; i < 2; i++)
    if (a.vis == c->vis[i].ptr) set(c->tag_vis[i], c->vis[i], k0);
  set(c->tag_worldpos, c->worldpos, k0);
  set(c->tag_depth, c->depth, k0);
  if (a.normals) set(c->tag_normals, c->normals, k0);
  if (a.grad_on) set(c->tag_gradient, c->gradient, key);
}

// would the recorded K0 + K1 rewrite every plane with the bytes it holds?  All or nothing: one plane that does not carry the
// key of its pass and both passes run
bool reuse_covers(const rtpt_ctx* c) {
  const rt::GbufferArgs& a = c->pending_gb;
  const K1Key& k = c->pending_key;
  if (!c->frame_reuse || !a.grad_on) return false;
  if (k.lut_version[0] == ~0ull || k.lut_version[1] == ~0ull) return false;  // injected LUT content
  const int v = a.vis == c->vis[0].ptr ? 0 : 1;
  if (a.vis != c->vis[v].ptr || !c->tag_vis[v].holds(k.k0)) return false;
  if (!c->tag_worldpos.holds(k.k0) || !c->tag_depth.holds(k.k0) || !c->tag_gradient.holds(k)) return false;
  return !a.normals || c->tag_normals.holds(k.k0);
}

// the five push-constant vectors K1 reads, to where GbufferArgs (g_*), GradientArgs or K1Key keep them
void gradient_inputs(const rtpt_push_constants* pc, float* cam, float* light, float* light_prev, float* color, float* color_prev) {
  const float* src[5] = {pc->cameraPos, pc->lightPos, pc->lightPosPrev, pc->currentCameraColor, pc->previousCameraColor};
  float* dst[5] = {cam, light, light_prev, color, color_prev};
  for (int i = 0; i < 5; i++) std::memcpy(dst[i], src[i], 3 * sizeof(float));
}

// launch_pathtrace's `specular`: rt::kSpecNee when the launch samples lights — the context has RTPT_FLAG_EXT_NEE and the scene's
// light list has entries (then it has material records too: the list is built beside them and dropped with them) — else what
// the materials ask for.  Without the flag, or with an empty list, every choice below is the one of a context without the flag.
// A context with RTPT_FLAG_EXT_NEE_SPHERE samples the analytic sphere light, whatever the scene's materials or light list:
// rt::kSpecNeeSphere, the kernels that sample both kinds (the triangles where the list has entries).  Such a launch has a
// sampling launch's limits (every segment in the tile kernel, no queue kernels, no path pool, no deferred final pass)
// RTPT_FLAG_EXT_NEE_POWER on top of a launch that samples the triangles of a list (both bits, entries, and the cumulative table
// that join_materials built beside the list): rt::kSpecNeePower / rt::kSpecNeeSpherePower, the kernels that pick by weight.
// Alone, with only RTPT_FLAG_EXT_NEE_SPHERE, or with an empty list the bit changes nothing
// RTPT_FLAG_EXT_NEE_MIS on top of a launch that samples the triangles of a list (the NEE bit, the MIS bit and entries): the MIS
// form of whichever of the four values the other bits choose.  Alone, with only RTPT_FLAG_EXT_NEE_SPHERE, or with an empty list
// the bit changes nothing: 0xA0000 on an empty list launches rt::kSpecNeeSphere
int trace_material_mode(const rtpt_ctx* c) {
  const bool nee = (c->cfg.flags & RTPT_FLAG_EXT_NEE) && c->scene.n_lights > 0 && c->scene.lights.ptr && c->scene.materials.ptr;
  const bool power = nee && (c->cfg.flags & RTPT_FLAG_EXT_NEE_POWER) && c->scene.light_table.cdf.ptr;
  const bool mis = nee && (c->cfg.flags & RTPT_FLAG_EXT_NEE_MIS);
  if (c->cfg.flags & RTPT_FLAG_EXT_NEE_SPHERE)
    return power ? (mis ? rt::kSpecNeeSpherePowerMis : rt::kSpecNeeSpherePower) : (mis ? rt::kSpecNeeSphereMis : rt::kSpecNeeSphere);
  if (!nee) return c->scene.materials_specular;
  return power ? (mis ? rt::kSpecNeePowerMis : rt::kSpecNeePower) : (mis ? rt::kSpecNeeMis : rt::kSpecNee);
}

// K2 of scenes whose BVH is built over fan pairs as the path-pool kernel (rtpt_ctx::trace_pool): the workgroups' slabs
int ensure_path_pool(rtpt_ctx* c, rt::PathtraceArgs& a) {
  a.pool_slab = nullptr;
  if (!(c->trace_pool && c->scene.use_bvh && c->scene.tree.leaf_pairs && a.compact && a.spp == 1 && !a.albedo && !c->scene.textures.records.ptr &&
        !trace_material_mode(c) && !c->scene.normals.records.ptr && !c->envmap.texels.ptr))
    return RTPT_OK;  // (the pool form stores no albedo, samples no texture, bounces diffusely about the triangle's normal: such frames take the tile kernel)
  const size_t need = rt::pathtrace_pool_bytes(static_cast<int>(c->cfg.width), static_cast<int>(c->rows()));  // 0: not built in
  if (need && c->path_pool.bytes < need)
    if (int rc = alloc_buf(c->path_pool, need)) return rc;
  a.pool_slab = need ? c->path_pool.ptr : nullptr;
  return RTPT_OK;
}

// the queues that hand the survivors of the first `window` segments to the queue kernels.  A region holds the survivors of
// ceil(workgroups / kPathQueues) workgroups of 256 paths (pathtrace_tile.hpp: enqueue_paths); the second buffer is only needed when a third segment
// window exists
int ensure_path_queues(rtpt_ctx* c, rt::PathtraceArgs& a, uint32_t window) {
  a.queue[0] = a.queue[1] = nullptr;
  a.queue_count = nullptr;
  a.queue_region = 0;
  if (!(a.compact && a.spp == 1 && a.max_segments > window && !(c->cfg.flags & RTPT_FLAG_SINGLE_LAUNCH_PATHS))) return RTPT_OK;
  if (rt::spec_lights(trace_material_mode(c))) return RTPT_OK;  // every segment runs in the tile kernel: the queue kernels sample no light
  if (c->envmap.texels.ptr) return RTPT_OK;                      // ... and read no environment map (kernels.hpp: the ENV axis)
  const size_t blocks = ((static_cast<size_t>(c->cfg.width) + 63) / 64) * ((c->rows() + 3) / 4);
  const size_t region = ((blocks + rt::kPathQueues - 1) / rt::kPathQueues) * 256;
  const size_t cap = region * rt::kPathQueues;
  int rc;
  if (!c->path_queue_count.ptr && (rc = alloc_buf(c->path_queue_count, 2 * rt::kPathQueues * sizeof(uint32_t)))) return rc;
  if (!c->path_queue[0].ptr && (rc = alloc_buf(c->path_queue[0], cap * 48))) return rc;
  if (a.max_segments > 2u * window && !c->path_queue[1].ptr && (rc = alloc_buf(c->path_queue[1], cap * 48))) return rc;
  a.queue[0] = c->path_queue[0].ptr;
  a.queue[1] = c->path_queue[1].ptr;
  a.queue_count = static_cast<uint32_t*>(c->path_queue_count.ptr);
  a.queue_region = static_cast<uint32_t>(region);
  return RTPT_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------ K0
int rtpt_gbuffer(rtpt_ctx* c, const rtpt_ubo* ubo, uint32_t y0, uint32_t y1) {
  if (!c || !ubo) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  int rc = check_rows(c, y0, y1);
  if (rc) return rc;
  if ((rc = gbuffer_flush(c)) || (rc = filter_flush(c, false))) return rc;
  // A deferred final pass stays deferred through a call that only records (the next rtpt_raytrace may take it): one that
  // launches or allocates anything, or changes what the pass reads (the pose and its LUTs), sends it out first
  if (c->deferred_valid &&
      ((c->cfg.flags & RTPT_FLAG_NO_FILTER_FUSION) || std::memcmp(ubo->model, c->scene.model, sizeof c->scene.model) != 0 ||
       c->scene.lut_version[c->lut_cur] != c->scene.model_version || !c->tables_valid || !c->scene.lut_prev_valid || !c->ray_tab.ptr ||
       c->ray_tab_p00 != ubo->proj[0] || c->ray_tab_p11 != ubo->proj[5] || c->ray_tab_w != c->cfg.width || c->ray_tab_h != c->cfg.height ||
       (no_pair_table(c) && !c->normals.ptr)) &&
      (rc = final_flush(c)))
    return rc;
  {
    // an affine model only (last row 0 0 0 1): the posed vertex is the xyz of model * (v, 1), visibility.vert.glsl:24
    const float* m = ubo->model;
    if (!(m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f))
      return fail(RTPT_E_INVALID, "ubo.model must be affine (bottom row 0 0 0 1)");
    float det = m[0] * (m[5] * m[10] - m[9] * m[6]) - m[4] * (m[1] * m[10] - m[9] * m[2]) + m[8] * (m[1] * m[6] - m[5] * m[2]);
    if (!(det != 0.0f) || det != det) return fail(RTPT_E_INVALID, "ubo.model is singular");
  }
  HIP_TRY(hipSetDevice(c->device));
  if (std::memcmp(ubo->model, c->scene.model, sizeof c->scene.model) != 0) {
    int rcm = apply_model(c, ubo->model);
    if (rcm) return rcm;
  }
  // The LUT is a function of the posed scene: the geometry stage's per-frame rewrite (visibility.geom.glsl:57-59)
  // produces the same bytes every frame while the model rests, so only a buffer that does not hold the current
  // pose yet is rebuilt (after rtpt_scene_upload / a model change / rtpt_set_plane).
  if ((rc = refresh_tables(c, c->scene.lut_version[c->lut_cur] != c->scene.model_version || !c->tables_valid))) return rc;
  rt::GbufferArgs a;
  a.g = geom(c, y0, y1);
  if ((rc = ensure_stack_spill(c, frame_blocks(c)))) return rc;
  a.scene = scene_view(c);
  const float* V = ubo->view;
  rt::f3 tcol{V[12], V[13], V[14]};
  rt::f3 c0{V[0], V[1], V[2]}, c1{V[4], V[5], V[6]}, c2{V[8], V[9], V[10]};
  a.org[0] = -rt::exact::dot(c0, tcol);
  a.org[1] = -rt::exact::dot(c1, tcol);
  a.org[2] = -rt::exact::dot(c2, tcol);
  a.c0[0] = c0.x; a.c0[1] = c0.y; a.c0[2] = c0.z;
  a.c1[0] = c1.x; a.c1[1] = c1.y; a.c1[2] = c1.z;
  a.c2[0] = c2.x; a.c2[1] = c2.y; a.c2[2] = c2.z;
  a.p00 = ubo->proj[0];
  a.p11 = ubo->proj[5];
  // per-column / per-row view-space ray directions (kernels.hip k_ray_tables): rebuilt when the projection or the frame
  // size they were built for changes (the reference's projection is constant after start-up, main.cpp:1471)
  if (!c->ray_tab.ptr || c->ray_tab_p00 != a.p00 || c->ray_tab_p11 != a.p11 || c->ray_tab_w != c->cfg.width || c->ray_tab_h != c->cfg.height) {
    int rct = alloc_buf(c->ray_tab, (static_cast<size_t>(c->cfg.width) + c->cfg.height) * sizeof(float));
    if (rct) return rct;
    rt::launch_ray_tables(static_cast<int>(c->cfg.width), static_cast<int>(c->cfg.height), a.p00, a.p11, static_cast<float*>(c->ray_tab.ptr),
                          static_cast<float*>(c->ray_tab.ptr) + c->cfg.width, c->stream);
    c->ray_tab_p00 = a.p00;
    c->ray_tab_p11 = a.p11;
    c->ray_tab_w = c->cfg.width;
    c->ray_tab_h = c->cfg.height;
  }
  a.dvx = static_cast<const float*>(c->ray_tab.ptr);
  a.dvy = a.dvx + c->cfg.width;
  rt::exact::mat_mul(ubo->proj, ubo->view, a.PV);
  a.tmax = c->cfg.ray_tmax;
  {
    const double org[3] = {a.org[0], a.org[1], a.org[2]};
    const double d0[3] = {c0.x, c0.y, c0.z}, d1[3] = {c1.x, c1.y, c1.z}, d2[3] = {c2.x, c2.y, c2.z};
    // view-space axis i of a world vector r is dot(row i of R, r); the columns c0,c1,c2 of the view
    // matrix's rotation hold R^T's rows, i.e. x_view = (c0.x, c1.x, c2.x) . r
    const double rx[3] = {d0[0], d1[0], d2[0]}, ry[3] = {d0[1], d1[1], d2[1]}, rz[3] = {d0[2], d1[2], d2[2]};
    a.cull = (!c->scene.use_bvh && c->width_fits_i16() && screen_bounds(c, org, rx, ry, rz, a.p00, a.p11, 0.0, a.bounds)) ? 1 : 0;
  }
  a.vis = static_cast<uint32_t*>(c->vis[c->frame.vis_cur].ptr);
  a.worldpos = static_cast<float4*>(c->worldpos.ptr);
  a.depth = static_cast<float*>(c->depth.ptr);
  a.normals = nullptr;
  a.normal_tab = static_cast<const float4*>(c->scene.normal_tab.ptr);
  a.area_tab = a.normal_tab + (c->scene.n_tris + 1);
  // more than 63 triangles: the filter stages per-pixel normals instead of ids.  RTPT_FLAG_EXT_SMOOTH_GUIDE, while active: any
  // triangle count, and the cells are guide normals (launch_gbuffer / launch_pathtrace take the switch in their NormalView)
  if (no_pair_table(c)) {
    if (!c->normals.ptr) {
      int rc2 = alloc_buf(c->normals, c->pixels() * 16);
      if (rc2) return rc2;
      c->frame.normals = Rows();
      reuse_invalidate(c, &c->normals);
    }
    a.normals = static_cast<float4*>(c->normals.ptr);
    // rows written so far this frame (strips call the pass once per range; a new frame starts a new range)
    const bool continues = c->frame.normals.y1 == static_cast<int>(y0) && c->frame.normals_frame == c->frames_ended;
    c->frame.normals = Rows(continues ? c->frame.normals.y0 : static_cast<int>(y0), y1);
    c->frame.normals_frame = c->frames_ended;
  }
  a.grad_on = 0;
  a.grad_y0 = a.grad_y1 = 0;
  a.lut = a.lut_prev = nullptr;
  a.grad = nullptr;
  for (int i = 0; i < 3; i++) a.g_cam[i] = a.g_light[i] = a.g_light_prev[i] = a.g_color[i] = a.g_color_prev[i] = 0.0f;
  if (!(c->cfg.flags & RTPT_FLAG_NO_FILTER_FUSION)) {
    // recorded: rtpt_temporal_gradient normally follows at once (main.cpp:1105-1106) and the two run as one launch;
    // any other entry point launches it first
    c->pending_gb = a;
    c->pending_gb_valid = true;
    c->pending_key = new_key<K1Key>();
    c->pending_key.k0 = gbuffer_key(c, a);
    return RTPT_OK;
  }
  tag_outputs(c, a, nullptr);  // launched unrecorded: the planes are rewritten, nothing keeps track of with what
  {
    Timer tm(c, RTPT_K_GBUFFER);
    rt::launch_gbuffer(a, c->stream, normal_view(c));
  }
  return launch_check("gbuffer");
}

}  // extern "C"

namespace rtpt_impl {
int final_flush(rtpt_ctx* c) {
  if (!c->deferred_valid) return RTPT_OK;
  c->deferred_valid = false;
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  {
    Timer tm(c, c->deferred.kernel);
    rt::launch_atrous(c->deferred.args, true, c->stream);
  }
  c->defer_info[2]++;
  return launch_check("temporal_filter");
}

int gbuffer_flush(rtpt_ctx* c) {
  if (!c->pending_gb_valid) return RTPT_OK;
  c->pending_gb_valid = false;
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  if (reuse_covers(c)) {  // every plane already holds what this launch would store
    c->reuse_info[0]++;
    return RTPT_OK;
  }
  if (int rc = final_flush(c)) return rc;  // (it reads the planes this launch rewrites)
  tag_outputs(c, c->pending_gb, &c->pending_key);
  {
    Timer tm(c, c->pending_gb.grad_on ? RTPT_K_GBUFFER_GRADIENT : RTPT_K_GBUFFER);
    rt::launch_gbuffer(c->pending_gb, c->stream, normal_view(c));
  }
  return launch_check(c->pending_gb.grad_on ? "gbuffer + temporal_gradient" : "gbuffer");
}
}  // namespace rtpt_impl

extern "C" {

// ------------------------------------------------------------------------------------------ K1
int rtpt_temporal_gradient(rtpt_ctx* c, const rtpt_push_constants* pc, uint32_t y0, uint32_t y1) {
  if (!c || !pc) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  int rc = check_rows(c, y0, y1);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (c->pending_gb_valid && static_cast<int32_t>(y0) >= c->pending_gb.g.y0 && static_cast<int32_t>(y1) <= c->pending_gb.g.y1) {
    // K0 + K1 in one launch: K1's inputs (id, world position) are K0's outputs for the same pixel
    rt::GbufferArgs& g = c->pending_gb;
    g.grad_on = 1;
    g.grad_y0 = static_cast<int32_t>(y0);
    g.grad_y1 = static_cast<int32_t>(y1);
    gradient_inputs(pc, g.g_cam, g.g_light, g.g_light_prev, g.g_color, g.g_color_prev);
    g.lut = static_cast<const float4*>(c->scene.lut[c->lut_cur].ptr);
    g.lut_prev = static_cast<const float4*>(c->scene.lut[c->lut_cur ^ 1].ptr);
    g.grad = static_cast<float4*>(c->gradient.ptr);
    K1Key& k = c->pending_key;
    gradient_inputs(pc, k.cam, k.light, k.light_prev, k.color, k.color_prev);
    k.y0 = g.grad_y0;
    k.y1 = g.grad_y1;
    k.lut_version[0] = c->scene.lut_version[c->lut_cur];
    k.lut_version[1] = c->scene.lut_version[c->lut_cur ^ 1];
    int rcq = filter_flush(c, false);
    if (rcq) return rcq;
    // stays recorded: rtpt_raytrace normally follows at once (main.cpp:1107) and takes both passes into its launch; any other
    // entry point launches them first (FLUSH_FILTER)
    if (c->fuse_trace) return RTPT_OK;
    return gbuffer_flush(c);
  }
  FLUSH_FILTER(c);
  if ((rc = ensure_tables(c))) return rc;  // K1 first after an upload or moved instances: the tables and LUTs it reads
  rt::GradientArgs a;
  a.g = geom(c, y0, y1);
  gradient_inputs(pc, a.cam, a.light, a.light_prev, a.color, a.color_prev);
  a.vis = static_cast<const uint32_t*>(c->vis[c->frame.vis_cur].ptr);
  a.worldpos = static_cast<const float4*>(c->worldpos.ptr);
  a.lut = static_cast<const float4*>(c->scene.lut[c->lut_cur].ptr);
  a.lut_prev = static_cast<const float4*>(c->scene.lut[c->lut_cur ^ 1].ptr);
  a.normal_tab = static_cast<const float4*>(c->scene.normal_tab.ptr);
  a.area_tab = a.normal_tab + (c->scene.n_tris + 1);
  a.grad = static_cast<float4*>(c->gradient.ptr);
  reuse_invalidate(c, &c->gradient);  // launched unrecorded
  {
    Timer tm(c, RTPT_K_GRADIENT);
    rt::launch_gradient(a, c->stream);
  }
  return launch_check("temporal_gradient");
}

// ------------------------------------------------------------------------------------------ K2
int rtpt_raytrace(rtpt_ctx* c, const rtpt_push_constants* pc, uint32_t y0, uint32_t y1) {
  if (!c || !pc) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  int rc = check_rows(c, y0, y1);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = filter_flush(c, false))) return rc;  // a recorded K0 (+ K1) stays recorded: it may join this launch (below)
  rt::PathtraceArgs a;
  a.g = geom(c, y0, y1);
  a.scene = scene_view(c);
  a.frame = pc->frameNumber;
  a.batch = pc->sample_batch;
  a.max_segments = c->cfg.max_segments;
  a.spp = c->cfg.samples_per_pixel;
  for (int i = 0; i < 3; i++) {
    a.cam[i] = pc->cameraPos[i];
    a.light_c[i] = pc->lightPos[i];                                          // raytrace.comp.glsl:279
    a.light_col[i] = pc->currentCameraColor[i] * c->cfg.light_intensity;     // :281
    a.light_col_first[i] = a.light_col[i] / c->cfg.first_hit_light_divisor;  // :229
  }
  a.light_r2 = c->cfg.light_radius * c->cfg.light_radius;  // :173
  a.slope = c->cfg.fov_slope;
  a.jitter = c->cfg.pixel_jitter;
  a.ray_offset = c->cfg.ray_offset;
  a.tmax = c->cfg.ray_tmax;
  a.image = nullptr;  // (below: a launch that carries a deferred final pass traces into the spare buffer)
  a.depth = static_cast<const float*>(c->depth.ptr);
  a.hit_id = (c->debug_mask & RTPT_DEBUG_HIT_ID) ? static_cast<uint32_t*>(c->hit_id.ptr) : nullptr;
  a.albedo = (c->cfg.flags & RTPT_FLAG_EXT_DEMODULATE) ? static_cast<float4*>(c->albedo.ptr) : nullptr;
  a.raycount = static_cast<unsigned long long*>(c->raycount.ptr);
  a.count_y0 = c->frame.count.y0;
  a.count_y1 = c->frame.count.y1;
  a.compact = (c->cfg.flags & RTPT_FLAG_NO_PATH_COMPACTION) ? 0 : 1;
  a.n_cu = c->n_cu;
  if ((rc = ensure_path_pool(c, a))) return rc;
  a.first_window = c->trace_window ? c->trace_window : rt::pt_first_window(c->scene.use_bvh);
  if ((rc = ensure_path_queues(c, a, a.first_window))) return rc;
  a.cull = 0;
  if (!c->scene.use_bvh && c->width_fits_i16()) {
    // K2 camera (raytrace.comp.glsl:314-320): at cameraPos, looking down -z, d = (slope*ux, slope*uy, -1) with
    // ux = (2cx - W)/H, uy = -(2cy - H)/H.  The Gaussian jitter is 0.375 * sqrt(-2 ln u1) <= 0.375 * 13.3 px
    // (u1 >= 1e-38, :87).
    const double org[3] = {pc->cameraPos[0], pc->cameraPos[1], pc->cameraPos[2]};
    const double ex[3] = {1, 0, 0}, ey[3] = {0, 1, 0}, ez[3] = {0, 0, 1};
    const double slope = c->cfg.fov_slope, W = c->cfg.width, H = c->cfg.height;
    if (slope > 0)
      a.cull = screen_bounds(c, org, ex, ey, ez, H / (W * slope), -1.0 / slope, std::fabs(c->cfg.pixel_jitter) * 13.3, a.bounds) ? 1 : 0;
  }
  c->frame.final_swapped = false;
  c->frame.image_alias = false;
  // K0 (+ K1) recorded right before this call run inside this launch, behind the tracing tiles (kernels.hip: k_gbuffer_pathtrace)
  const bool joined = c->pending_gb_valid && c->fuse_trace && rt::pathtrace_fuses_gbuffer(a, c->pending_gb);
  if (!joined && (rc = gbuffer_flush(c))) return rc;
  // frame reuse: the planes hold what the recorded passes would store, so the launch carries the tracing tiles only — the
  // un-fused kernel, which takes the depth for the traced image's alpha from the depth plane.  It is still timed as the launch
  // that serves K0 + K1 + K2
  const bool reused = joined && reuse_covers(c);
  const bool fused = joined && !reused;
  // The deferred final pass of the frame before joins this launch when only tracing tiles are in it, the tile kernel can carry
  // it and the trace covers every stored row (so that the spare buffer it writes then holds what IMAGE would).  The pass reads
  // the buffer IMAGE names now (the old history), so the trace goes to the buffer no role names and the two change places.
  // Every other call sends the pass out first.
  // (a context with an environment map has no tile kernel that carries a final pass: kernels.hpp, the ENV axis)
  const bool take = c->deferred_valid && !fused && !c->envmap.texels.ptr && rt::pathtrace_takes_final(a, tex_view(c), trace_material_mode(c)) &&
                    a.g.y0 == static_cast<int32_t>(c->cfg.row_begin) && a.g.y1 == static_cast<int32_t>(c->cfg.row_end);
  if (!take && (rc = final_flush(c))) return rc;
  if (take) {
    FrameState& fr = c->frame;
    if (!c->color[fr.color_spare].ptr) {
      if ((rc = alloc_buf(c->color[fr.color_spare], c->pixels() * 16))) return rc;
      HIP_TRY(hipMemsetAsync(c->color[fr.color_spare].ptr, 0, c->pixels() * 16, c->stream));
    }
    std::swap(fr.color_of_role[ROLE_IMAGE], fr.color_spare);
  }
  a.image = static_cast<float4*>(c->color[c->frame.color_of_role[ROLE_IMAGE]].ptr);
  c->frame.alpha_depth[c->frame.color_of_role[ROLE_IMAGE]] = true;
  if ((rc = ensure_stack_spill(c, std::max<size_t>(frame_blocks(c), rt::pathtrace_grid_blocks(a, fused ? &c->pending_gb : nullptr))))) return rc;
  a.scene = scene_view(c);
  if (joined) {
    c->pending_gb.scene = a.scene;  // the spill area may have moved since the G-buffer call was recorded
    c->pending_gb_valid = false;
    if (reused)
      c->reuse_info[0]++;
    else
      tag_outputs(c, c->pending_gb, &c->pending_key);
  }
  {
    Timer tm(c, joined ? RTPT_K_GBUFFER_PATHTRACE : RTPT_K_PATHTRACE);
    rt::launch_pathtrace(a, fused ? &c->pending_gb : nullptr, tex_view(c), trace_material_mode(c), c->stream,
                         take ? &c->deferred.args : nullptr, &c->filter_policy, c->empty_run_info, light_view(c), normal_view(c), env_view(c));
  }
  if (take) {
    c->deferred_valid = false;
    c->defer_info[1]++;
  }
  return launch_check(fused ? "gbuffer + temporal_gradient + raytrace" : "raytrace");
}

// ------------------------------------------------------------------------------------------ K3
// rtpt_temporal_filter keeps the reference's shape — one call per iteration of applyTemporalFiltering's loop
// (main.cpp:1259-1305) — but the calls of a frame are RECORDED and launched when the last iteration arrives, the way the
// reference records its dispatches into command buffers: consecutive iterations then run as one chained launch
// (atrous_chain.hip) whose intermediate image never leaves LDS.  Any call that observes or changes what an iteration
// reads or writes (readback, plane pointers, sync, another pass, ...) first runs the recorded iterations one by one, so
// between iterations every plane holds exactly what the separate dispatches would have left there.
}  // extern "C"

namespace {

// main.cpp:1264-1281: odd k reads `image`, writes `filteredImageBuffer`; even k the reverse.  An even last iteration blends
// into a buffer nothing reads (main.cpp:55 "must be an odd number"), so only an odd last iteration is the FINAL pass.
bool is_final(int k, int max_it) { return k == max_it && (k & 1); }

// the tap spacing of iteration k and how far its taps reach from their centre
struct Reach {
  int stride;
  int64_t reach;
};
Reach filter_reach(uint32_t ext, int k) {
  const int stride = (ext & rt::kExtPow2Stride) ? (1 << (k - 1)) : k;
  return {stride, static_cast<int64_t>(stride) * ((ext & rt::kExtGauss5) ? 2 : 1)};
}
// the rows an iteration over [y0, y1) reads: y +- reach, clamped to the frame (temporalFiltering.comp.glsl:135-136)
Rows rows_read(const rtpt_ctx* c, uint32_t y0, uint32_t y1, int64_t reach) {
  return Rows(std::max<int64_t>(0, static_cast<int64_t>(y0) - reach), std::min<int64_t>(c->cfg.height, static_cast<int64_t>(y1) + reach));
}

// does rtpt_temporal_filter record its calls in this context (to launch consecutive iterations as one chain)?
bool records_filter_calls(const rtpt_ctx* c) {
  return !(c->cfg.flags & (RTPT_FLAG_NO_FILTER_FUSION | RTPT_FLAG_DIRECT_FILTER)) && !(c->cfg.flags & rt::kExtMask) && !no_pair_table(c) &&
         c->chain_max > 1;  // (the chained kernel and the deferred final pass need the id-pair table)
}

int filter_validate(rtpt_ctx* c, const rtpt_push_constants* pc, const rtpt_ubo* ubo, uint32_t& y0, uint32_t& y1) {
  int rc = check_rows(c, y0, y1);
  if (rc) return rc;
  const int k = pc->waveletIteration, max_it = pc->maxWaveletIteration;
  if (k < 1 || max_it < 1 || k > max_it) return fail(RTPT_E_INVALID, "need 1 <= waveletIteration <= maxWaveletIteration");
  const uint32_t ext = c->cfg.flags & rt::kExtMask;
  if ((ext & rt::kExtPow2Stride) && k > 24) return fail(RTPT_E_INVALID, "RTPT_FLAG_EXT_POW2_STRIDE supports at most 24 iterations");
  const int64_t reach = filter_reach(ext, k).reach;
  const Rows read = rows_read(c, y0, y1, reach);  // they must be stored here
  if (y1 > y0 && !c->stored_rows().covers(read.y0, read.y1))
    return fail(RTPT_E_INVALID, "filter taps reaching " + std::to_string(reach) + " rows leave the stored rows (missing halo)");
  if (is_final(k, max_it) && !ubo) return fail(RTPT_E_INVALID, "the final pass needs the UBO (viewPrev/projPrev)");
  if ((ext & rt::kExtVariance) && !ubo)
    return fail(RTPT_E_INVALID, "RTPT_FLAG_EXT_VARIANCE needs the UBO (viewPrev/projPrev) on every iteration");
  return RTPT_OK;
}

// The previous frame as the final pass and the moment accumulation read it: the context's own planes, or the ones gathered
// across strips that rtpt_set_external_history / rtpt_set_external_guides registered.  `rows` hold a previous frame; the
// plane stores frame rows from row_base on.
struct PrevPlane {
  const void* ptr;
  const void* moments;  // prev_guides only
  Rows rows;
  int row_base;
};
PrevPlane prev_history(const rtpt_ctx* c) {
  const FrameState& fr = c->frame;
  if (fr.ext_history) return {fr.ext_history, nullptr, fr.ext_hist, fr.ext_hist.y0};
  return {c->color[fr.color_of_role[ROLE_PREVIOUS]].ptr, nullptr, fr.hist, static_cast<int>(c->cfg.row_begin)};
}
// with_moments: the reader needs the moments next to the ids, so registered ids alone do not serve it
PrevPlane prev_guides(const rtpt_ctx* c, bool with_moments) {
  const FrameState& fr = c->frame;
  if (fr.ext_prev_vis && (fr.ext_moments || !with_moments)) return {fr.ext_prev_vis, fr.ext_moments, fr.ext_guides, fr.ext_guides.y0};
  return {c->vis[fr.vis_cur ^ 1].ptr, c->moments[fr.moments_cur ^ 1].ptr, fr.guides, static_cast<int>(c->cfg.row_begin)};
}

// Reprojection reuse (api_internal.hpp: ReprojKey), for the single-launch final pass `a` of the plain comb kernel over rows
// [y0, y1): sets a.reproj_in when the plane holds this pass's reprojected pixels, a.reproj_out when this pass is to store them
// (its key equals the previous frame's final pass's; the plane is allocated here, at the first store), neither otherwise.
// store->valid: the plane carries *store once the launch is out (commit_filter).
int reproj_policy(rtpt_ctx* c, rt::AtrousArgs& a, uint32_t y0, uint32_t y1, PlaneTag<ReprojKey>* store) {
  const PlaneTag<K0Key>& wp = c->tag_worldpos;
  const uint64_t lut_version = c->scene.lut_version[c->lut_cur ^ 1];
  const bool eligible = c->frame_reuse && c->reproj_reuse && !(c->debug_mask & RTPT_DEBUG_PREV_PIXEL) &&  // (that plane wants the raw integers)
                        c->cfg.width <= 65535 && c->cfg.height <= 65535 && wp.valid && c->tag_vis[c->frame.vis_cur].holds(wp.key) &&
                        wp.key.y0 <= static_cast<int32_t>(y0) && wp.key.y1 >= static_cast<int32_t>(y1) && lut_version != ~0ull;
  if (!eligible) {
    c->reproj_last.valid = false;
    return RTPT_OK;
  }
  ReprojKey k = new_key<ReprojKey>();
  k.k0 = wp.key;
  k.lut_version = lut_version;
  std::memcpy(k.PVprev, a.PVprev, sizeof k.PVprev);
  k.y0 = static_cast<int32_t>(y0);
  k.y1 = static_cast<int32_t>(y1);
  if (c->tag_reproj.holds(k) && c->reproj.ptr) {
    a.reproj_in = static_cast<const uint32_t*>(c->reproj.ptr);
    c->reproj_info[1]++;
  } else if (c->reproj_last.holds(k)) {
    if (c->reproj.bytes != c->pixels() * 4) {
      int rc = alloc_buf(c->reproj, c->pixels() * 4);
      if (rc) return rc;
    }
    if (c->tag_reproj.valid) c->reproj_info[2]++;
    c->tag_reproj.valid = false;  // until the store is out
    a.reproj_out = static_cast<uint32_t*>(c->reproj.ptr);
    store->valid = true;
    store->key = k;
    c->reproj_info[0]++;
  }
  c->reproj_last.valid = true;
  c->reproj_last.key = k;
  return RTPT_OK;
}

// What one launch does: iteration f.pc.waveletIteration — or, with levels > 1, that iteration and the levels - 1 after it as
// one chain, over the rows of the chain's LAST iteration (f.y0, f.y1).  A function of the context and the call.
struct FilterPlan {
  int k, k_last, max_it, levels;
  Reach tap;
  bool final_pass;    // k_last is the FINAL pass ...
  bool second_range;  // ... of a frame that already had one: another row range of the same pass
  bool alpha_zero;    // the last iteration of an even N writes `image` and nothing filters it again: alpha 0 like the reference's
                      // vec4(rgb, 0) (temporalFiltering.comp.glsl:152), so a device-side consumer of IMAGE never sees the depth
  int in_buf, out_buf;  // of rtpt_ctx::color.  A chain reads its first iteration's input and writes the OTHER buffer, whatever
                        // the parity of its length
  int result_role;      // the role the separate passes would have left the result in
  int kernel;           // for the timer
};
FilterPlan plan_filter(const rtpt_ctx* c, const FilterCall& f, int levels) {
  FilterPlan p;
  p.k = f.pc.waveletIteration;
  p.max_it = f.pc.maxWaveletIteration;
  p.levels = levels;
  p.k_last = p.k + levels - 1;
  p.tap = filter_reach(c->cfg.flags & rt::kExtMask, p.k);
  p.final_pass = is_final(p.k_last, p.max_it);
  p.second_range = levels == 1 && p.final_pass && c->frame.final_swapped;
  p.alpha_zero = p.k_last == p.max_it && !p.final_pass;
  const bool from_image = ((p.k & 1) != 0) != p.second_range;  // (the first range swapped the two roles)
  p.in_buf = c->frame.color_of_role[from_image ? ROLE_IMAGE : ROLE_FILTERED];
  p.out_buf = c->frame.color_of_role[from_image ? ROLE_FILTERED : ROLE_IMAGE];
  p.result_role = (p.final_pass || !(p.k_last & 1)) ? ROLE_IMAGE : ROLE_FILTERED;  // D1: the blend becomes `image`
  p.kernel = levels > 1 ? (p.final_pass ? RTPT_K_ATROUS_CHAIN_FINAL : RTPT_K_ATROUS_CHAIN) : (p.final_pass ? RTPT_K_ATROUS_FINAL : RTPT_K_ATROUS);
  return p;
}

// the launches that must precede the pass: the depth channel of an injected input, the moments, the variance prefilter
void filter_prelaunch(rtpt_ctx* c, const FilterPlan& p, const FilterCall& f) {
  FrameState& fr = c->frame;
  const uint32_t ext = c->cfg.flags & rt::kExtMask;
  if (!fr.alpha_depth[p.in_buf]) {  // rtpt_set_plane / rtpt_bind_plane
    rt::launch_stamp_depth(geom(c, c->cfg.row_begin, c->cfg.row_end), static_cast<float4*>(c->color[p.in_buf].ptr),
                           static_cast<const float*>(c->depth.ptr), c->stream);
    fr.alpha_depth[p.in_buf] = true;
  }
  if (!(ext & rt::kExtVariance)) return;
  if (p.k == 1) {  // temporal accumulation of the luminance moments of the traced image (this iteration's input)
    const PrevPlane guides = prev_guides(c, true);
    rt::MomentsArgs m;
    std::memset(&m, 0, sizeof m);
    m.g = geom(c, c->cfg.row_begin, c->cfg.row_end);
    m.frame = f.pc.frameNumber;
    m.alpha = c->cfg.alpha;
    m.traced = static_cast<const float4*>(c->color[p.in_buf].ptr);
    m.vis = static_cast<const uint32_t*>(c->vis[fr.vis_cur].ptr);
    m.worldpos = static_cast<const float4*>(c->worldpos.ptr);
    m.lut_prev = static_cast<const float4*>(c->scene.lut[c->lut_cur ^ 1].ptr);
    rt::exact::mat_mul(f.ubo.projPrev, f.ubo.viewPrev, m.PVprev);
    m.prev_vis = static_cast<const uint32_t*>(guides.ptr);
    m.moments_prev = static_cast<const float4*>(guides.moments);
    m.hist_row_base = guides.row_base;
    m.hist_y0 = guides.rows.y0;
    m.hist_y1 = guides.rows.y1;
    m.svgf = (ext & rt::kExtSvgfVariance) ? 1 : 0;
    m.rows_stored = static_cast<int32_t>(c->rows());
    m.moments_out = static_cast<float4*>(c->moments[fr.moments_cur].ptr);
    m.var_out = static_cast<float*>(c->variance[0].ptr);
    rt::launch_moments(m, c->stream);
    fr.variance_last = 0;
  }
  if ((ext & rt::kExtSvgfVariance) && c->var_scale.ptr)  // SVGF's variance prefilter: the centre's scale only
    rt::launch_var_prefilter(geom(c, f.y0, f.y1), static_cast<int>(c->rows()), static_cast<const float*>(c->variance[fr.variance_last].ptr),
                             static_cast<float*>(c->var_scale.ptr), c->stream);
  fr.variance_last ^= 1;  // the buffer the pass writes
}

// the kernel's arguments.  Besides `a` this writes the reuse counters and FrameState::present_fused; *store as reproj_policy
// *px_normals (launch_atrous's): RTPT_FLAG_EXT_SMOOTH_GUIDE is active and the per-pixel plane covers the rows read — the launch
// has no id-pair table and every kernel weighs two pixels' cells.  A plane that does not (not written in this frame, or
// rtpt_set_plane(RTPT_PLANE_VIS_ID) since) leaves the call what it is without the flag: filtered with the triangles' normals.
int fill_atrous_args(rtpt_ctx* c, const FilterPlan& p, const FilterCall& f, rt::AtrousArgs& a, PlaneTag<ReprojKey>* store, bool* px_normals) {
  FrameState& fr = c->frame;
  std::memset(&a, 0, sizeof a);
  a.g = geom(c, f.y0, f.y1);
  a.k = p.k;
  a.stride = p.tap.stride;
  a.ext = c->cfg.flags & rt::kExtMask;
  a.exact = (c->cfg.flags & RTPT_FLAG_EXACT_FILTER) ? 1 : 0;
  a.direct = (c->cfg.flags & RTPT_FLAG_DIRECT_FILTER) ? 1 : 0;
  a.n_tris = c->scene.n_tris;
  a.pair_tab = static_cast<const float*>(c->scene.pair_tab.ptr);
  a.rows_stored = static_cast<int32_t>(c->rows());
  a.n_cu = c->n_cu;
  a.alpha_zero = p.alpha_zero ? 1 : 0;
  a.sigma_n = c->cfg.sigma_n;
  a.sigma_z = c->cfg.sigma_z;
  a.sigma_l = c->cfg.sigma_l;
  a.in = static_cast<const float4*>(c->color[p.in_buf].ptr);
  a.out = static_cast<float4*>(c->color[p.out_buf].ptr);
  a.vis = static_cast<const uint32_t*>(c->vis[fr.vis_cur].ptr);
  a.normal_tab = static_cast<const float4*>(c->scene.normal_tab.ptr);
  const Rows read = rows_read(c, f.y0, f.y1, p.tap.reach);
  if (c->normals.ptr && fr.normals_frame == c->frames_ended && fr.normals.covers(read.y0, read.y1)) a.normals = static_cast<const float4*>(c->normals.ptr);
  *px_normals = guide_active(c) && a.normals;
  if (*px_normals) a.pair_tab = nullptr;
  if (a.ext & rt::kExtVariance) {  // (filter_prelaunch left variance_last naming the buffer this pass writes)
    a.var_in = static_cast<const float*>(c->variance[fr.variance_last ^ 1].ptr);
    a.var_out = static_cast<float*>(c->variance[fr.variance_last].ptr);
    if ((a.ext & rt::kExtSvgfVariance) && c->var_scale.ptr) a.var_scale = static_cast<const float*>(c->var_scale.ptr);
  }
  if (!p.final_pass) return RTPT_OK;
  const PrevPlane hist = prev_history(c), guides = prev_guides(c, false);
  a.frame = f.pc.frameNumber;
  a.alpha = c->cfg.alpha;
  a.worldpos = static_cast<const float4*>(c->worldpos.ptr);
  a.lut_prev = static_cast<const float4*>(c->scene.lut[c->lut_cur ^ 1].ptr);
  rt::exact::mat_mul(f.ubo.projPrev, f.ubo.viewPrev, a.PVprev);  // temporalFiltering.comp.glsl:180
  a.prev_pixel = (c->debug_mask & RTPT_DEBUG_PREV_PIXEL) ? static_cast<int2*>(c->prev_pixel.ptr) : nullptr;
  a.gradient = static_cast<const float4*>(c->gradient.ptr);
  a.history = static_cast<const float4*>(hist.ptr);
  a.hist_row_base = hist.row_base;
  a.hist_y0 = hist.rows.y0;
  a.hist_y1 = hist.rows.y1;
  a.prev_vis = static_cast<const uint32_t*>(guides.ptr);
  a.pvis_row_base = guides.row_base;
  a.pvis_y0 = guides.rows.y0;
  a.pvis_y1 = guides.rows.y1;
  fr.present_fused_dst = nullptr;  // a new frame's final pass: the previous frame's blit is history
  if (p.levels > 1) return RTPT_OK;
  // (RTPT_FLAG_EXT_DEMODULATE: the pass stores demodulated colour, the swapchain takes colour x albedo — rtpt_present does the work)
  if (c->present_dst && Rows(f.y0, f.y1).covers(c->present_rows.y0, c->present_rows.y1) && !(c->cfg.flags & RTPT_FLAG_EXT_DEMODULATE) &&
      rt::atrous_final_fuses_present(a)) {
    a.present = static_cast<uint32_t*>(c->present_dst);
    a.present_y0 = c->present_rows.y0;
    a.present_y1 = c->present_rows.y1;
    fr.present_fused_dst = c->present_dst;
    fr.present_fused = c->present_rows;
  }
  // the other final-pass routes (direct, extension, chained) neither load nor store and leave the tag alone: it is keyed on
  // the pass's inputs, not on who ran
  return rt::atrous_final_plain_comb(a) ? reproj_policy(c, a, f.y0, f.y1, store) : RTPT_OK;
}

// the launch is out: afterwards every role names the buffer the separate passes would have left it in
void commit_filter(rtpt_ctx* c, const FilterPlan& p, const FilterCall& f, const PlaneTag<ReprojKey>& stored) {
  FrameState& fr = c->frame;
  if (stored.valid) c->tag_reproj = stored;
  fr.alpha_depth[p.out_buf] = !p.final_pass && !p.alpha_zero;
  fr.color_of_role[p.result_role] = p.out_buf;
  fr.color_of_role[p.result_role == ROLE_IMAGE ? ROLE_FILTERED : ROLE_IMAGE] = p.in_buf;
  if (p.k_last == p.max_it) {  // the rows of IMAGE that hold the filtered frame
    if (p.second_range)
      fr.final.extend(f.y0, f.y1);
    else
      fr.final = Rows(f.y0, f.y1);
  }
  if (p.final_pass) fr.final_swapped = true;
}

// may the prepared final pass `a` wait for the next rtpt_raytrace (DeferredFinal)?  A single launch of the plain comb kernel that
// a tracing launch can carry (rt::atrous_final_role: no extension, no prev_pixel store, no fused present, LDS within that
// launch's), reading and writing nothing but planes the context owns
bool defers(const rtpt_ctx* c, const FilterPlan& p, rt::AtrousArgs& a) {
  if (!c->final_defer || !p.final_pass || p.levels != 1 || p.second_range || c->frame.ext_history || c->frame.ext_prev_vis) return false;
  for (int i = 0; i < 3; i++)
    if (!c->color[i].owned) return false;
  if (!c->vis[c->frame.vis_cur].owned || !c->depth.owned) return false;
  return rt::atrous_final_role(a);
}

// defer: the call is the last record of a frame's run (filter_flush)
int filter_launch(rtpt_ctx* c, const FilterCall& f, int levels, bool defer = false) {
  HIP_TRY(hipSetDevice(c->device));
  const FilterPlan p = plan_filter(c, f, levels);
  filter_prelaunch(c, p, f);
  rt::AtrousArgs a;
  PlaneTag<ReprojKey> stored;
  bool px_normals = false;
  int rc = fill_atrous_args(c, p, f, a, &stored, &px_normals);
  if (rc) return rc;
  if (defer && defers(c, p, a)) {
    c->deferred.args = a;
    c->deferred.kernel = p.kernel;
    c->deferred_valid = true;
    c->defer_info[0]++;
    commit_filter(c, p, f, stored);
    return RTPT_OK;
  }
  {
    Timer tm(c, p.kernel);
    if (levels > 1)
      rt::launch_atrous_chain(a, levels, p.final_pass, c->filter_policy, c->stream);
    else
      rt::launch_atrous(a, p.final_pass, c->stream, px_normals);
  }
  if ((rc = launch_check("temporal_filter"))) return rc;
  commit_filter(c, p, f, stored);
  return RTPT_OK;
}

// how many of the records from calls[i] on run as one launch: the chain grows while the next record is the next iteration,
// its rows are covered and the kernel has the LDS.  Greedy from the front.
int chain_length(const rtpt_ctx* c, const std::vector<FilterCall>& calls, size_t i) {
  const int k0 = calls[i].pc.waveletIteration, max_it = calls[i].pc.maxWaveletIteration;
  int levels = 1;
  while (i + levels < calls.size() && levels < c->chain_max) {
    const FilterCall &cur = calls[i + levels - 1], &nxt = calls[i + levels];
    const int kn = nxt.pc.waveletIteration;
    if (kn != k0 + levels || nxt.pc.maxWaveletIteration != max_it) break;
    const bool nxt_final = is_final(kn, max_it);
    if (nxt_final && !c->chain_final) break;
    if (nxt_final && c->frame.final_swapped) break;
    const Rows need = rows_read(c, nxt.y0, nxt.y1, filter_reach(c->cfg.flags & rt::kExtMask, kn).reach);
    if (nxt.y1 <= nxt.y0 || !Rows(cur.y0, cur.y1).covers(need.y0, need.y1)) break;
    if (static_cast<int64_t>(nxt.y1 - nxt.y0) * c->cfg.width < c->chain_min_pixels) break;
    if (!rt::atrous_chain_supported(k0, levels + 1, c->scene.n_tris)) break;
    levels++;
    if (nxt_final) break;
  }
  return levels;
}

}  // namespace

namespace rtpt_impl {
// run the recorded iterations.  fuse = false: one launch per iteration (an observer is about to look at the planes)
int filter_flush(rtpt_ctx* c, bool fuse) {
  if (c->pending.empty()) return RTPT_OK;
  if (int rc = final_flush(c)) return rc;  // an earlier frame's deferred pass goes ahead of these
  std::vector<FilterCall> calls;
  calls.swap(c->pending);  // filter_launch may fail: the record is dropped either way
  fuse = fuse && records_filter_calls(c);
  for (size_t i = 0; i < calls.size();) {
    const int levels = fuse ? chain_length(c, calls, i) : 1;
    FilterCall f = calls[i];
    if (levels > 1) {
      const FilterCall& lastc = calls[i + levels - 1];
      f.y0 = lastc.y0;
      f.y1 = lastc.y1;
      f.has_ubo = lastc.has_ubo;
      f.ubo = lastc.ubo;
      f.pc.frameNumber = lastc.pc.frameNumber;
    }
    int rc = filter_launch(c, f, levels, fuse && i + static_cast<size_t>(levels) == calls.size());
    if (rc) return rc;
    i += static_cast<size_t>(levels);
  }
  return RTPT_OK;
}

}  // namespace rtpt_impl

extern "C" {

int rtpt_temporal_filter(rtpt_ctx* c, const rtpt_push_constants* pc, const rtpt_ubo* ubo, uint32_t y0, uint32_t y1) {
  if (!c || !pc) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  int rc = filter_validate(c, pc, ubo, y0, y1);
  if (rc) return rc;
  if ((rc = ensure_tables(c))) return rc;
  FilterCall f;
  f.pc = *pc;
  f.has_ubo = ubo != nullptr;
  if (ubo) f.ubo = *ubo;
  f.y0 = y0;
  f.y1 = y1;
  if (!records_filter_calls(c)) {
    FLUSH_FILTER(c);
    return filter_launch(c, f, 1);
  }
  // a recorded K0 (rtpt_gbuffer without rtpt_temporal_gradient behind it) goes out before the first filter record: the
  // filters read its id / depth planes and are launched from here on without looking at it again
  {
    int rcg = gbuffer_flush(c);
    if (rcg) return rcg;
  }
  // a record that does not continue the recorded run (same iteration twice, a restart) ends it
  if (!c->pending.empty() && (c->pending.back().pc.waveletIteration + 1 != pc->waveletIteration ||
                              c->pending.back().pc.maxWaveletIteration != pc->maxWaveletIteration))
    FLUSH_FILTER(c);
  c->pending.push_back(f);
  if (pc->waveletIteration == pc->maxWaveletIteration) return filter_flush(c, true);
  return RTPT_OK;
}

// ------------------------------------------------------------------------------------------ K4
int rtpt_end_frame(rtpt_ctx* c) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  {  // (a deferred final pass stays deferred: the roles rotate on top of what it will have written)
    int rcf = gbuffer_flush(c);
    if (rcf == RTPT_OK) rcf = filter_flush(c, false);
    if (rcf) return rcf;
  }
  // main.cpp:1364 image -> previousImage: rotate roles instead of blitting.  After the reference's
  // copy both images hold the same pixels; here IMAGE now names the old history buffer (about to be
  // overwritten by the next rtpt_raytrace), so until then rtpt_readback(IMAGE) is served from
  // PREVIOUS (image_alias).
  FrameState& fr = c->frame;
  std::swap(fr.color_of_role[ROLE_IMAGE], fr.color_of_role[ROLE_PREVIOUS]);
  fr.image_alias = true;
  fr.hist = fr.final;
  // the id plane (and, with RTPT_FLAG_EXT_VARIANCE, the moment plane) of the frame just ended cover the stored rows
  fr.guides = c->stored_rows();
  // main.cpp:1367 visibilityBuffer -> previousVisibilityBuffer; main.cpp:1372 LUT -> LUTprev
  fr.vis_cur ^= 1;
  fr.moments_cur ^= 1;
  c->lut_cur ^= 1;
  c->scene.lut_prev_valid = c->scene.n_tris != 0;
  fr.final_swapped = false;
  c->frames_ended++;
  return RTPT_OK;
}

// the swapchain image rows the next final filter pass should also write (fused blit); NULL clears the registration
int rtpt_present_target(rtpt_ctx* c, void* dst_device, uint32_t y0, uint32_t y1) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!dst_device) {
    c->present_dst = nullptr;
    return RTPT_OK;
  }
  if (reinterpret_cast<uintptr_t>(dst_device) & 3u) return fail(RTPT_E_INVALID, "swapchain image must be 4-byte aligned");
  FLUSH_FILTER(c);  // recorded iterations were recorded without it: they go out as they are
  int rc = check_rows(c, y0, y1);
  if (rc) return rc;
  c->present_dst = dst_device;
  c->present_rows = Rows(y0, y1);
  return RTPT_OK;
}

// main.cpp:1338-1361: the blit of `image` to the swapchain image
int rtpt_present(rtpt_ctx* c, void* dst_device, uint32_t y0, uint32_t y1) {
  if (!c || !dst_device) return fail(RTPT_E_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dst_device) & 3u) return fail(RTPT_E_INVALID, "swapchain image must be 4-byte aligned");
  FLUSH_FILTER(c);
  int rc = check_rows(c, y0, y1);
  if (rc) return rc;
  // already there: the frame's final pass wrote these rows of this image in swapchain format (rtpt_present_target)
  const FrameState& fr = c->frame;
  if (fr.present_fused_dst && fr.present_fused.covers(y0, y1) &&
      static_cast<char*>(dst_device) == static_cast<char*>(fr.present_fused_dst) + static_cast<size_t>(static_cast<int>(y0) - fr.present_fused.y0) * c->cfg.width * 4)
    return RTPT_OK;
  const auto [b, rows] = finished_frame(c);
  if (!b || !b->ptr) return fail(RTPT_E_INVALID, "no image plane");
  if (!rows.covers(y0, y1))
    return fail(RTPT_E_INVALID, "rtpt_present: rows [" + std::to_string(y0) + "," + std::to_string(y1) + ") outside the rows of the finished frame [" +
                                    std::to_string(rows.y0) + "," + std::to_string(rows.y1) + ")");
  HIP_TRY(hipSetDevice(c->device));
  {
    Timer tm(c, RTPT_K_PRESENT);
    rt::launch_present(geom(c, y0, y1), static_cast<const float4*>(b->ptr),
                       (c->cfg.flags & RTPT_FLAG_EXT_DEMODULATE) ? static_cast<const float4*>(c->albedo.ptr) : nullptr, static_cast<uint32_t*>(dst_device),
                       c->stream);
  }
  return launch_check("present");
}

// RTPT_FLAG_EXT_DEMODULATE: SHADED = frame x ALBEDO, the frame being what rtpt_present blits
int rtpt_modulate(rtpt_ctx* c, uint32_t y0, uint32_t y1) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!(c->cfg.flags & RTPT_FLAG_EXT_DEMODULATE)) return fail(RTPT_E_INVALID, "rtpt_modulate needs RTPT_FLAG_EXT_DEMODULATE");
  FLUSH_FILTER(c);
  int rc = check_rows(c, y0, y1);
  if (rc) return rc;
  const Buf* b = finished_frame(c).buf;
  if (!b || !b->ptr || !c->albedo.ptr || !c->shaded.ptr) return fail(RTPT_E_INVALID, "no image plane");
  HIP_TRY(hipSetDevice(c->device));
  {
    Timer tm(c, RTPT_K_MODULATE);
    rt::launch_modulate(geom(c, y0, y1), static_cast<const float4*>(b->ptr), static_cast<const float4*>(c->albedo.ptr),
                        static_cast<float4*>(c->shaded.ptr), c->stream);
  }
  return launch_check("modulate");
}

}  // extern "C"
