// api_context.hip — the context of the C ABI (include/rtpt.h): creation, planes, streams, copies, counters, timing, and the
// helpers shared by the other api_*.hip units (api_internal.hpp).
#include "api_internal.hpp"
#include "env_host.hpp"

#include <atomic>

namespace rtpt_impl {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}


// workgroups of the largest per-frame launch that traverses the BVH: the 64 x 4-pixel tiles of the stored rows
// (k_gbuffer, the tile kernel) or the persistent queue kernel's grid
size_t frame_blocks(const rtpt_ctx* c) {
  const size_t tiles = ((static_cast<size_t>(c->cfg.width) + 63) / 64) * ((static_cast<size_t>(c->cfg.row_end - c->cfg.row_begin) + 3) / 4);
  return std::max(tiles, static_cast<size_t>(c->n_cu > 0 ? c->n_cu : 256) * 8);
}
// the spill area of the BVH traversal stack holds (stack depth - LDS entries) x workgroups x 256 entries: grown (never
// shrunk) before a launch whose grid is larger than any before it
int ensure_stack_spill(rtpt_ctx* c, size_t blocks) {
  if (!c->scene.use_bvh) return RTPT_OK;
  const size_t depth = static_cast<size_t>(c->scene.tree.bvh_depth + 2 < 8 ? 8 : c->scene.tree.bvh_depth + 2);
  const size_t lds = std::min<size_t>(depth, static_cast<size_t>(c->bvh_stack_lds));
  if (depth <= lds || blocks <= c->stack_spill_blocks) return RTPT_OK;
  if (c->stack_spill.ptr) {
    hipError_t e = hipStreamSynchronize(c->stream);  // launches that spill into the old area
    if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    free_buf(c->stack_spill);
  }
  c->stack_spill_blocks = 0;
  int rc = alloc_buf(c->stack_spill, (depth - lds) * blocks * 256 * sizeof(uint32_t));
  if (rc) return rc;
  c->stack_spill_blocks = blocks;
  return RTPT_OK;
}

// bytes held by owned Bufs, process-wide (rtpt_debug_live_device_bytes): updated here and in Buf::release, the two places
// that allocate and free device memory
static std::atomic<uint64_t> g_live_device_bytes{0};

int alloc_buf(Buf& b, size_t bytes) {
  b.release();
  if (bytes == 0) return RTPT_OK;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return fail(RTPT_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  b.ptr = p;
  b.bytes = bytes;
  b.owned = true;
  g_live_device_bytes += bytes;
  return RTPT_OK;
}

void Buf::release() {
  if (owned && ptr) {
    (void)hipFree(ptr);
    g_live_device_bytes -= bytes;
  }
  ptr = nullptr, bytes = 0, owned = false;
}

void free_buf(Buf& b) { b.release(); }

Buf* plane_buf(rtpt_ctx* c, rtpt_plane which) {
  switch (which) {
    case RTPT_PLANE_IMAGE: return &c->color[c->frame.color_of_role[ROLE_IMAGE]];
    case RTPT_PLANE_FILTERED: return &c->color[c->frame.color_of_role[ROLE_FILTERED]];
    case RTPT_PLANE_PREVIOUS: return &c->color[c->frame.color_of_role[ROLE_PREVIOUS]];
    case RTPT_PLANE_WORLDPOS: return &c->worldpos;
    case RTPT_PLANE_GRADIENT: return &c->gradient;
    case RTPT_PLANE_DEPTH: return &c->depth;
    case RTPT_PLANE_VIS_ID: return &c->vis[c->frame.vis_cur];
    case RTPT_PLANE_PREV_VIS_ID: return &c->vis[c->frame.vis_cur ^ 1];
    case RTPT_PLANE_LUT: return &c->scene.lut[c->lut_cur];
    case RTPT_PLANE_LUT_PREV: return &c->scene.lut[c->lut_cur ^ 1];
    case RTPT_PLANE_PREV_PIXEL: return &c->prev_pixel;
    case RTPT_PLANE_RAYCOUNT: return &c->raycount;
    case RTPT_PLANE_HIT_ID: return &c->hit_id;
    case RTPT_PLANE_MOMENTS: return &c->moments[c->frame.moments_cur];
    case RTPT_PLANE_MOMENTS_PREV: return &c->moments[c->frame.moments_cur ^ 1];
    case RTPT_PLANE_VARIANCE: return &c->variance[c->frame.variance_last];
    case RTPT_PLANE_ALBEDO: return &c->albedo;
    case RTPT_PLANE_SHADED: return &c->shaded;
    default: return nullptr;
  }
}

int color_index(const rtpt_ctx* c, const Buf* b) {
  for (int i = 0; i < 4; i++)
    if (b == &c->color[i]) return i;
  return -1;
}

FinishedFrame finished_frame(rtpt_ctx* c) {
  if (c->frame.image_alias) return {plane_buf(c, RTPT_PLANE_PREVIOUS), c->frame.hist};
  return {plane_buf(c, RTPT_PLANE_IMAGE), c->frame.final};
}

size_t plane_size(const rtpt_ctx* c, rtpt_plane which) {
  const size_t px = c->pixels();
  switch (which) {
    case RTPT_PLANE_IMAGE:
    case RTPT_PLANE_FILTERED:
    case RTPT_PLANE_PREVIOUS:
    case RTPT_PLANE_WORLDPOS:
    case RTPT_PLANE_GRADIENT: return px * 16;
    case RTPT_PLANE_DEPTH:
    case RTPT_PLANE_VIS_ID:
    case RTPT_PLANE_PREV_VIS_ID:
    case RTPT_PLANE_HIT_ID:
    case RTPT_PLANE_VARIANCE: return px * 4;
    case RTPT_PLANE_MOMENTS:
    case RTPT_PLANE_MOMENTS_PREV:
    case RTPT_PLANE_ALBEDO:
    case RTPT_PLANE_SHADED: return px * 16;
    case RTPT_PLANE_PREV_PIXEL: return px * 8;
    case RTPT_PLANE_LUT:
    case RTPT_PLANE_LUT_PREV: return (static_cast<size_t>(c->scene.n_tris) + 1) * sizeof(rtpt_visibility_data);
    case RTPT_PLANE_RAYCOUNT: return 8;
    default: return 0;
  }
}


int check_rows(const rtpt_ctx* c, uint32_t& y0, uint32_t& y1) {
  if (y0 == 0 && y1 == 0) {
    y0 = c->cfg.row_begin;
    y1 = c->cfg.row_end;
  }
  if (y0 > y1 || y0 < c->cfg.row_begin || y1 > c->cfg.row_end)
    return fail(RTPT_E_INVALID, "row range [" + std::to_string(y0) + "," + std::to_string(y1) + ") outside stored rows [" +
                                    std::to_string(c->cfg.row_begin) + "," + std::to_string(c->cfg.row_end) + ")");
  return RTPT_OK;
}

rt::FrameGeom geom(const rtpt_ctx* c, uint32_t y0, uint32_t y1) {
  rt::FrameGeom g;
  g.W = static_cast<int32_t>(c->cfg.width);
  g.H = static_cast<int32_t>(c->cfg.height);
  g.row_base = static_cast<int32_t>(c->cfg.row_begin);
  g.y0 = static_cast<int32_t>(y0);
  g.y1 = static_cast<int32_t>(y1);
  return g;
}

rt::SceneView scene_view(const rtpt_ctx* c) {
  rt::SceneView s;
  s.isect_id = static_cast<const float4*>(c->scene.isect_id.ptr);
  s.isect_leaf = static_cast<const float4*>(c->scene.isect_leaf.ptr);
  s.leaf_ids = static_cast<const uint32_t*>(c->scene.tree.leaf_order.ptr);
  s.shade = static_cast<const float4*>(c->scene.shade.ptr);
  s.nodes = static_cast<const rt::BvhNodeQ*>(c->scene.tree.nodes.ptr);
  s.bvh_grid = static_cast<const float*>(c->scene.bvh_grid_dev.ptr);
  s.n_tris = c->scene.n_tris;
  s.use_bvh = c->scene.use_bvh ? 1u : 0u;
  s.paired = (c->scene.tris_paired && !c->no_pairing) ? 1u : 0u;
  s.leaf_pairs = c->scene.tree.leaf_pairs ? 1u : 0u;
  s.stack_depth = static_cast<uint32_t>(c->scene.tree.bvh_depth + 2 < 8 ? 8 : c->scene.tree.bvh_depth + 2);
  s.stack_lds = std::min<uint32_t>(s.stack_depth, static_cast<uint32_t>(c->bvh_stack_lds));
  s.stack_spill = static_cast<uint32_t*>(c->stack_spill.ptr);
  s.materials = static_cast<const float4*>(c->scene.materials.ptr);
  s.n_base_tris = c->scene.n_base_tris ? c->scene.n_base_tris : 1u;
  return s;
}

rt::TexView tex_view(const rtpt_ctx* c) {
  rt::TexView t;
  t.records = static_cast<const float4*>(c->scene.textures.records.ptr);
  t.desc = static_cast<const rt::TexDesc*>(c->scene.textures.desc.ptr);
  t.texels = static_cast<const float4*>(c->scene.textures.texels.ptr);
  t.levels = static_cast<const uint32_t*>(c->scene.textures.levels.ptr);
  t.bounce_spread = c->tex_bounce_spread;
  return t;
}

rt::LightTableView light_view(const rtpt_ctx* c) {
  const bool list = c->scene.lights.ptr && c->scene.materials.ptr;  // (the list is built beside the records and dropped with them)
  return rt::LightTableView{list ? static_cast<const uint32_t*>(c->scene.lights.ptr) : nullptr, list ? c->scene.n_lights : 0u,
                            static_cast<const uint64_t*>(c->scene.light_table.cdf.ptr)};
}

rt::NormalView normal_view(const rtpt_ctx* c) {
  const bool has = c->scene.normals.records.ptr && c->scene.normals.cof.ptr;
  const bool guide = guide_active(c);
  return rt::NormalView{has ? static_cast<const float4*>(c->scene.normals.records.ptr) : nullptr,
                        has ? static_cast<const float4*>(c->scene.normals.cof.ptr) : nullptr, guide ? 1u : 0u, guide ? c->cfg.sigma_n : 0};
}

rt::EnvView env_view(const rtpt_ctx* c) {
  const rtpt_ctx::Environment& e = c->envmap;
  rt::EnvView v{};
  v.texels = static_cast<const float4*>(e.texels.ptr);
  v.n = e.texels.ptr ? e.n : 0u;
  v.flags = e.flags;
  v.r0 = make_float4(e.rot[0], e.rot[1], e.rot[2], 0.0f);
  v.r1 = make_float4(e.rot[3], e.rot[4], e.rot[5], 0.0f);
  v.r2 = make_float4(e.rot[6], e.rot[7], e.rot[8], 0.0f);
  v.scale = make_float4(e.scale[0], e.scale[1], e.scale[2], 0.0f);
  return v;
}

bool guide_active(const rtpt_ctx* c) {
  return (c->cfg.flags & RTPT_FLAG_EXT_SMOOTH_GUIDE) && c->scene.normals.records.ptr && c->scene.normals.cof.ptr;
}

// Conservative screen bounds of the triangles of a small scene for a pinhole camera at `org` whose
// view-space axes are the columns c0,c1,c2 and whose pixel (x,y) looks along
// (nx/p00, ny/p11, -1), nx = (2(x+.5)-W)/W, ny = (2(y+.5)-H)/H  (the K0 ray; the K2 camera is the
// special case c = identity, p00 = H/(W*slope), p11 = -1/slope).  `jitter_px` widens the bounds by
// the largest possible sub-pixel offset of a primary ray.  A vertex at or behind the camera plane
// makes the projection unbounded: such a triangle is never culled.
bool screen_bounds(const rtpt_ctx* c, const double org[3], const double c0[3], const double c1[3], const double c2[3],
                   double p00, double p11, double jitter_px, rt::TriBounds* out) {
  if (c->scene.host_tris.empty() || c->scene.n_tris > static_cast<uint32_t>(rt::kCullMaxTris)) return false;
  const double W = c->cfg.width, H = c->cfg.height;
  for (uint32_t t = 0; t < c->scene.n_tris; t++) {
    double xmin = 1e30, xmax = -1e30, ymin = 1e30, ymax = -1e30;
    bool unbounded = false;
    for (int k = 0; k < 3; k++) {
      const float* P = c->scene.host_tris.data() + 9 * static_cast<size_t>(t) + 3 * k;
      const double r[3] = {P[0] - org[0], P[1] - org[1], P[2] - org[2]};
      const double xv = c0[0] * r[0] + c0[1] * r[1] + c0[2] * r[2];
      const double yv = c1[0] * r[0] + c1[1] * r[1] + c1[2] * r[2];
      const double zv = c2[0] * r[0] + c2[1] * r[1] + c2[2] * r[2];
      const double len = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
      if (!(-zv > 1e-4 * (len + 1.0))) {
        unbounded = true;
        break;
      }
      const double cx = (p00 * xv / (-zv) + 1.0) * 0.5 * W, cy = (p11 * yv / (-zv) + 1.0) * 0.5 * H;
      xmin = std::min(xmin, cx); xmax = std::max(xmax, cx);
      ymin = std::min(ymin, cy); ymax = std::max(ymax, cy);
    }
    auto clamp16 = [](double v) { return static_cast<int16_t>(std::max(-32000.0, std::min(32000.0, v))); };
    if (unbounded || !(xmax >= xmin)) {
      out[t] = rt::TriBounds{-32000, -32000, 32000, 32000};
    } else {
      const double pad = jitter_px + 1.5;  // pixel index = continuous coordinate - 0.5, +1 px of slack
      out[t] = rt::TriBounds{clamp16(std::floor(xmin - pad)), clamp16(std::floor(ymin - pad)), clamp16(std::ceil(xmax + pad)),
                             clamp16(std::ceil(ymax + pad))};
    }
  }
  return true;
}

bool is_identity(const float* m) {
  for (int i = 0; i < 16; i++)
    if (m[i] != ((i % 5 == 0) ? 1.0f : 0.0f)) return false;
  return true;
}

int launch_check(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
  return RTPT_OK;
}

}  // namespace rtpt_impl

extern "C" {


const char* rtpt_last_error(const rtpt_ctx*) { return g_err.c_str(); }

int rtpt_config_default(rtpt_config* cfg, uint32_t width, uint32_t height) {
  if (!cfg) return fail(RTPT_E_INVALID, "cfg is NULL");
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->struct_size = sizeof(rtpt_config);
  cfg->width = width;
  cfg->height = height;
  cfg->row_begin = 0;
  cfg->row_end = height;
  cfg->max_segments = 32;              // raytrace.comp.glsl:204
  cfg->samples_per_pixel = 1;          // raytrace.comp.glsl:306
  cfg->sigma_n = 128;                  // temporalFiltering.comp.glsl:203
  cfg->sigma_z = 1.0f;                 // :204
  cfg->sigma_l = 4.0f;                 // :205
  cfg->alpha = 0.3f;                   // :243
  cfg->light_radius = 0.20f;           // raytrace.comp.glsl:280
  cfg->light_intensity = 30.0f;        // :281
  cfg->first_hit_light_divisor = 5.0f; // :229
  cfg->fov_slope = 0.20271003f;        // tan(FOV = 0.20), common.h:16 / raytrace.comp.glsl:300
  cfg->pixel_jitter = 0.375f;          // :314
  cfg->ray_offset = 0.0001f;           // :250
  cfg->ray_tmax = 10000.0f;            // :216
  cfg->flags = 0;
  cfg->device = -1;
  return RTPT_OK;
}

// (re)allocate every per-pixel plane for c->cfg's frame and row range and reset the frame state; the scene
// (triangles, BVH, LUTs, tables) is untouched.  Caller-bound planes (rtpt_bind_plane) are dropped.
static int alloc_planes(rtpt_ctx* c) {
  const size_t px = c->pixels();
  int rc = RTPT_OK;
  for (int i = 0; i < 3 && rc == RTPT_OK; i++) rc = alloc_buf(c->color[i], px * 16);
  free_buf(c->color[3]);  // sized per frame: re-created by the next trace that carries a deferred final pass
  for (int i = 0; i < 2 && rc == RTPT_OK; i++) rc = alloc_buf(c->vis[i], px * 4);
  if (rc == RTPT_OK) rc = alloc_buf(c->worldpos, px * 16);
  if (rc == RTPT_OK) rc = alloc_buf(c->gradient, px * 16);
  if (rc == RTPT_OK) rc = alloc_buf(c->depth, px * 4);
  if (rc == RTPT_OK && !c->raycount.ptr) rc = alloc_buf(c->raycount, 8 * rt::kRayCounters);
  for (auto& b : c->path_queue) free_buf(b);  // sized per frame: re-created by the next rtpt_raytrace
  free_buf(c->normals);  // sized per frame: re-created by the next rtpt_gbuffer
  free_buf(c->reproj);   // sized per frame: re-created by the next final pass that stores (reuse_invalidate below drops its tag)
  reuse_invalidate(c, nullptr);  // new, cleared planes
  if (c->cfg.flags & RTPT_FLAG_EXT_VARIANCE) {
    for (int i = 0; i < 2 && rc == RTPT_OK; i++) rc = alloc_buf(c->moments[i], px * 16);
    for (int i = 0; i < 2 && rc == RTPT_OK; i++) rc = alloc_buf(c->variance[i], px * 4);
    for (int i = 0; i < 2 && rc == RTPT_OK; i++) {
      (void)hipMemsetAsync(c->moments[i].ptr, 0, px * 16, c->stream);
      (void)hipMemsetAsync(c->variance[i].ptr, 0, px * 4, c->stream);
    }
    if (rc == RTPT_OK && (c->cfg.flags & RTPT_FLAG_EXT_SVGF_VARIANCE)) rc = alloc_buf(c->var_scale, px * 4);
  }
  if (c->cfg.flags & RTPT_FLAG_EXT_DEMODULATE) {
    for (Buf* b : {&c->albedo, &c->shaded}) {
      if (rc == RTPT_OK) rc = alloc_buf(*b, px * 16);
      if (rc == RTPT_OK) (void)hipMemsetAsync(b->ptr, 0, px * 16, c->stream);
    }
  }
  if (rc == RTPT_OK && (c->debug_mask & RTPT_DEBUG_HIT_ID)) rc = alloc_buf(c->hit_id, px * 4);
  if (rc == RTPT_OK && (c->debug_mask & RTPT_DEBUG_PREV_PIXEL)) rc = alloc_buf(c->prev_pixel, px * 8);
  if (rc != RTPT_OK) return rc;
  // Vulkan images start undefined; zero them so readback before the first frame is defined
  for (int i = 0; i < 3; i++) (void)hipMemsetAsync(c->color[i].ptr, 0, px * 16, c->stream);
  for (int i = 0; i < 2; i++) (void)hipMemsetAsync(c->vis[i].ptr, 0, px * 4, c->stream);
  (void)hipMemsetAsync(c->worldpos.ptr, 0, px * 16, c->stream);
  (void)hipMemsetAsync(c->gradient.ptr, 0, px * 16, c->stream);
  (void)hipMemsetAsync(c->depth.ptr, 0, px * 4, c->stream);
  (void)hipMemsetAsync(c->raycount.ptr, 0, 8 * rt::kRayCounters, c->stream);
  if (c->hit_id.ptr) (void)hipMemsetAsync(c->hit_id.ptr, 0, px * 4, c->stream);
  if (c->prev_pixel.ptr) (void)hipMemsetAsync(c->prev_pixel.ptr, 0, px * 8, c->stream);
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("initial clear: ") + hipGetErrorString(e));
  // (without RTPT_FLAG_EXT_VARIANCE the moment planes were not reallocated above: one a caller bound keeps its place)
  const int moments_cur = (c->cfg.flags & RTPT_FLAG_EXT_VARIANCE) ? 0 : c->frame.moments_cur;
  c->frame = FrameState(c->stored_rows());
  c->frame.moments_cur = moments_cur;
  return RTPT_OK;
}

int rtpt_create(const rtpt_config* cfg, rtpt_ctx** out) {
  if (!cfg || !out) return fail(RTPT_E_INVALID, "NULL argument");
  *out = nullptr;
  if (cfg->struct_size != sizeof(rtpt_config)) return fail(RTPT_E_INVALID, "rtpt_config.struct_size mismatch (ABI)");
  if (cfg->width == 0 || cfg->height == 0 || cfg->row_begin >= cfg->row_end || cfg->row_end > cfg->height)
    return fail(RTPT_E_INVALID, "bad frame / row range");
  if (cfg->max_segments == 0 || cfg->samples_per_pixel == 0 || cfg->sigma_n < 1)
    return fail(RTPT_E_INVALID, "max_segments, samples_per_pixel and sigma_n must be >= 1");
  if ((cfg->flags & RTPT_FLAG_EXT_SVGF_VARIANCE) && !(cfg->flags & RTPT_FLAG_EXT_VARIANCE))
    return fail(RTPT_E_INVALID, "RTPT_FLAG_EXT_SVGF_VARIANCE completes RTPT_FLAG_EXT_VARIANCE: set both");
  if ((cfg->flags & RTPT_FLAG_EXT_DEMODULATE) && cfg->samples_per_pixel > 1)
    return fail(RTPT_E_INVALID, "RTPT_FLAG_EXT_DEMODULATE needs samples_per_pixel == 1 (the mean of products is not the product of means)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(RTPT_E_NO_GPU, "no HIP device visible; this library has no CPU fallback");
  }
  int dev = cfg->device;
  if (dev < 0) {
    HIP_TRY(hipGetDevice(&dev));
  } else {
    if (dev >= ndev) return fail(RTPT_E_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(dev));
  }
  rtpt_ctx* c = new (std::nothrow) rtpt_ctx();
  if (!c) return fail(RTPT_E_NOMEM, "host allocation failed");
  c->cfg = *cfg;
  c->device = dev;
  hipError_t e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return fail(RTPT_E_DEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  }
  c->stream = c->own_stream;
  {
    // per-DEVICE launch state (contexts on different GPUs of one process are independent, rtpt.h): CU count for the
    // persistent grids and the >64 KiB dynamic-LDS attribute of the staged filter kernels
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) c->n_cu = prop.multiProcessorCount;
    e = rt::prepare_device_atrous();
    if (e == hipSuccess) e = rt::prepare_device_atrous_chain();
    if (e != hipSuccess) {
      rtpt_destroy(c);
      return fail(RTPT_E_DEVICE, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
    }
  }
  // tuning knobs for A/B runs on the box (never needed for correctness: every setting computes the same pixels)
  if (const char* v = std::getenv("RTPT_NO_TRI_PAIRS")) c->no_pairing = std::atoi(v) != 0;
  if (const char* v = std::getenv("RTPT_HOST_REFIT")) c->host_refit = std::atoi(v) != 0;
  c->device_bvh = (cfg->flags & RTPT_FLAG_DEVICE_BVH_BUILD) != 0;
  c->device_bvh_sah = c->device_bvh && (cfg->flags & RTPT_FLAG_DEVICE_BVH_SAH) != 0;  // alone the bit is ignored
  if (const char* v = std::getenv("RTPT_DEVICE_BVH")) {
    if (!std::strcmp(v, "sah"))
      c->device_bvh = c->device_bvh_sah = true;
    else
      c->device_bvh = c->device_bvh || std::atoi(v) != 0;
  }
  c->device_flatten = c->device_bvh && (cfg->flags & RTPT_FLAG_DEVICE_FLATTEN) != 0;  // alone the bit is ignored
  if (const char* v = std::getenv("RTPT_LBVH_ORDER")) c->lbvh_by_height = !std::strcmp(v, "height");
  if (const char* v = std::getenv("RTPT_NO_TRACE_FUSION")) c->fuse_trace = std::atoi(v) == 0;
  if (const char* v = std::getenv("RTPT_NO_FRAME_REUSE")) c->frame_reuse = std::atoi(v) == 0;
  if (const char* v = std::getenv("RTPT_NO_REPROJ_REUSE")) c->reproj_reuse = std::atoi(v) == 0;
  if (const char* v = std::getenv("RTPT_TRACE_POOL")) c->trace_pool = std::atoi(v) != 0;
  if (const char* v = std::getenv("RTPT_TEX_BOUNCE_SPREAD")) {
    const float f = std::strtof(v, nullptr);
    if (f > 0.0f && f <= 64.0f) c->tex_bounce_spread = f;
  }
  if (const char* v = std::getenv("RTPT_PT_WINDOW")) c->trace_window = static_cast<uint32_t>(std::max(0, std::atoi(v)));
  if (const char* v = std::getenv("RTPT_CHAIN_G1")) c->filter_policy.chain_g_pin = std::atoi(v);
  if (const char* v = std::getenv("RTPT_CHAIN_GENERIC")) c->filter_policy.chain_generic = std::atoi(v);
  if (const char* v = std::getenv("RTPT_CHAIN_WG_PER_CU")) c->filter_policy.chain_wg_per_cu = std::atoi(v);
  if (const char* v = std::getenv("RTPT_CHAIN_SKEW")) {
    c->filter_policy.chain_skew = c->filter_policy.chain_skew2 = std::atoi(v);
    if (const char* comma = std::strchr(v, ',')) c->filter_policy.chain_skew2 = std::atoi(comma + 1);
  }
  if (const char* v = std::getenv("RTPT_CHAIN_BW")) c->filter_policy.chain_bw = std::atoi(v);
  if (const char* v = std::getenv("RTPT_NO_FINAL_DEFER")) c->final_defer = std::atoi(v) == 0;
  if (const char* v = std::getenv("RTPT_FINAL_FRONT")) {
    c->filter_policy.final_front = std::atoi(v);
    if (const char* comma = std::strchr(v, ',')) c->filter_policy.final_front_share = std::atoi(comma + 1);
  }
  if (const char* v = std::getenv("RTPT_EMPTY_RUN")) c->filter_policy.empty_run = std::max(0, std::atoi(v));
  if (const char* v = std::getenv("RTPT_CHAIN_SW")) c->filter_policy.chain_sw = std::atoi(v);
  if (const char* v = std::getenv("RTPT_CHAIN_SW_G1")) c->filter_policy.chain_sw_g1 = std::atoi(v);
  if (const char* v = std::getenv("RTPT_CHAIN_SW_G3")) c->filter_policy.chain_sw_g3 = std::atoi(v);
  if (const char* v = std::getenv("RTPT_CHAIN_MAX")) c->chain_max = std::max(1, std::min(3, std::atoi(v)));
  if (const char* v = std::getenv("RTPT_CHAIN_FINAL")) c->chain_final = std::atoi(v) != 0;
  if (const char* v = std::getenv("RTPT_BVH_STACK_LDS")) c->bvh_stack_lds = std::max(1, std::atoi(v));
  if (const char* v = std::getenv("RTPT_CHAIN_MIN_PIXELS")) c->chain_min_pixels = std::atoll(v);
  int rc = alloc_planes(c);
  if (rc != RTPT_OK) {
    rtpt_destroy(c);
    return rc;
  }
  *out = c;
  return RTPT_OK;
}

int rtpt_destroy(rtpt_ctx* c) {
  if (!c) return RTPT_OK;
  (void)hipSetDevice(c->device);
  (void)final_flush(c);  // (the caller may own the buffer it writes and expect the frame there)
  if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
  for (auto& t : c->timed) {
    (void)hipEventDestroy(t.start);
    (void)hipEventDestroy(t.stop);
  }
  for (auto& e : c->event_pool) (void)hipEventDestroy(e);
  if (c->handoff_event) (void)hipEventDestroy(c->handoff_event);
  for (hipEvent_t e : c->build_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& st : c->xf_stage) {
    if (st.done) (void)hipEventDestroy(st.done);
    if (st.host) (void)hipHostFree(st.host);
  }
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;  // every device buffer: the context and its scene own them through Buf members
  return RTPT_OK;
}

int rtpt_resize(rtpt_ctx* c, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (row_begin == 0 && row_end == 0) row_end = height;
  if (width == 0 || height == 0 || row_begin >= row_end || row_end > height) return fail(RTPT_E_INVALID, "bad frame / row range");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  rtpt_config old = c->cfg;
  c->cfg.width = width;
  c->cfg.height = height;
  c->cfg.row_begin = row_begin;
  c->cfg.row_end = row_end;
  c->present_dst = c->frame.present_fused_dst = nullptr;  // a swapchain image registered for the old size is not this size's
  int rc = alloc_planes(c);
  if (rc != RTPT_OK) {  // leave a usable context behind if the old size still fits
    c->cfg = old;
    (void)alloc_planes(c);
    return rc;
  }
  return RTPT_OK;
}

int rtpt_set_stream(rtpt_ctx* c, void* hip_stream) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  FLUSH_FILTER(c);
  hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->own_stream;
  if (s != c->stream) reuse_invalidate(c, nullptr);  // a reused plane was written on the other stream, in no order with this one
  c->stream = s;
  return RTPT_OK;
}

int rtpt_plane_bytes(const rtpt_ctx* c, rtpt_plane which, size_t* bytes) {
  if (!c || !bytes) return fail(RTPT_E_INVALID, "NULL argument");
  if (which < 0 || which >= RTPT_PLANE_COUNT) return fail(RTPT_E_INVALID, "unknown plane");
  *bytes = plane_size(c, which);
  return RTPT_OK;
}

int rtpt_plane_ptr(rtpt_ctx* c, rtpt_plane which, void** device_ptr) {
  if (!c || !device_ptr) return fail(RTPT_E_INVALID, "NULL argument");
  FLUSH_FILTER(c);  // roles rotate when recorded iterations run
  Buf* b = plane_buf(c, which);
  if (!b) return fail(RTPT_E_INVALID, "unknown plane");
  reuse_invalidate(c, b);  // the caller can write through the pointer
  *device_ptr = b->ptr;
  return RTPT_OK;
}

int rtpt_bind_plane(rtpt_ctx* c, rtpt_plane which, void* device_ptr, size_t bytes) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  FLUSH_FILTER(c);
  Buf* b = plane_buf(c, which);
  if (!b || which == RTPT_PLANE_RAYCOUNT || which == RTPT_PLANE_LUT || which == RTPT_PLANE_LUT_PREV)
    return fail(RTPT_E_INVALID, "plane cannot be bound");
  const size_t need = plane_size(c, which);
  reuse_invalidate(c, b);
  if (device_ptr == nullptr) {
    if (b->owned) return RTPT_OK;
    return alloc_buf(*b, need);
  }
  if (bytes < need) return fail(RTPT_E_INVALID, "bound buffer too small");
  if ((reinterpret_cast<uintptr_t>(device_ptr) & 15u) != 0) return fail(RTPT_E_INVALID, "bound buffer must be 16-byte aligned");
  HIP_TRY(hipStreamSynchronize(c->stream));
  free_buf(*b);
  b->ptr = device_ptr;
  b->bytes = bytes;
  b->owned = false;
  if (const int i = color_index(c, b); i >= 0) c->frame.alpha_depth[i] = false;
  return RTPT_OK;
}

int rtpt_set_external_history(rtpt_ctx* c, const void* device_ptr, uint32_t row_begin, uint32_t row_end) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (device_ptr && (row_begin >= row_end || row_end > c->cfg.height)) return fail(RTPT_E_INVALID, "bad history row range");
  if (device_ptr && (reinterpret_cast<uintptr_t>(device_ptr) & 15u)) return fail(RTPT_E_INVALID, "history buffer must be 16-byte aligned");
  if (int rc = final_flush(c)) return rc;  // (recorded iterations stay recorded: the registration is for the pass still to come)
  c->frame.ext_history = device_ptr;
  c->frame.ext_hist = Rows(row_begin, row_end);
  return RTPT_OK;
}

int rtpt_set_external_guides(rtpt_ctx* c, const void* prev_vis, const void* moments_prev, uint32_t row_begin, uint32_t row_end) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (int rc = final_flush(c)) return rc;
  if (!prev_vis && !moments_prev) {
    c->frame.ext_prev_vis = c->frame.ext_moments = nullptr;
    return RTPT_OK;
  }
  if (!prev_vis) return fail(RTPT_E_INVALID, "the previous id plane is needed whenever guides are registered");
  if (row_begin >= row_end || row_end > c->cfg.height) return fail(RTPT_E_INVALID, "bad guide row range");
  if ((reinterpret_cast<uintptr_t>(prev_vis) & 3u) || (reinterpret_cast<uintptr_t>(moments_prev) & 15u))
    return fail(RTPT_E_INVALID, "guide buffers must be 4- / 16-byte aligned");
  c->frame.ext_prev_vis = prev_vis;
  c->frame.ext_moments = moments_prev;
  c->frame.ext_guides = Rows(row_begin, row_end);
  return RTPT_OK;
}

int rtpt_stream_wait(rtpt_ctx* c, rtpt_ctx* other) {
  if (!c || !other) return fail(RTPT_E_INVALID, "NULL argument");
  // "everything submitted to `other` so far" includes its recorded iterations; this context's own recorded iterations
  // do not depend on `other` and go out ahead of the wait.  Neither call looks at a plane, so both may run chained.
  int rcw = gbuffer_flush(other);
  if (rcw == RTPT_OK) rcw = gbuffer_flush(c);
  if (rcw == RTPT_OK) rcw = filter_flush(other, true);
  if (rcw == RTPT_OK) rcw = filter_flush(c, true);
  // (a final pass those two deferred included: the wait orders everything submitted so far, and the pass of `c` must not end
  // up behind a wait it was recorded in front of)
  if (rcw == RTPT_OK) rcw = final_flush(other);
  if (rcw == RTPT_OK) rcw = final_flush(c);
  if (rcw) return rcw;
  if (c == other || c->stream == other->stream) return RTPT_OK;  // one stream is already in order
  if (c->device != other->device) return fail(RTPT_E_INVALID, "rtpt_stream_wait: the contexts are on different devices");
  HIP_TRY(hipSetDevice(c->device));

  if (!other->handoff_event) HIP_TRY(hipEventCreateWithFlags(&other->handoff_event, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(other->handoff_event, other->stream));
  HIP_TRY(hipStreamWaitEvent(c->stream, other->handoff_event, 0));
  return RTPT_OK;
}

int rtpt_enable_debug(rtpt_ctx* c, uint32_t mask) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  if ((mask & RTPT_DEBUG_HIT_ID) && !c->hit_id.ptr) {
    int rc = alloc_buf(c->hit_id, c->pixels() * 4);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->hit_id.ptr, 0, c->pixels() * 4, c->stream));
  }
  if ((mask & RTPT_DEBUG_PREV_PIXEL) && !c->prev_pixel.ptr) {
    int rc = alloc_buf(c->prev_pixel, c->pixels() * 8);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->prev_pixel.ptr, 0, c->pixels() * 8, c->stream));
  }
  if (mask != c->debug_mask) reuse_invalidate(c, nullptr);  // what the passes write changes with the mask
  c->debug_mask = mask;
  return RTPT_OK;
}

// frame reuse, observed: [0] frames whose K0 + K1 were not launched, [1], [2] reserved and 0 (the cached reprojection of the
// final pass reports through rtpt_debug_reproj_info), [3] plane tags invalidated
int rtpt_debug_reuse_info(rtpt_ctx* c, uint64_t out[4]) {
  if (!c || !out) return fail(RTPT_E_INVALID, "NULL argument");
  for (int i = 0; i < 4; i++) out[i] = c->reuse_info[i];
  return RTPT_OK;
}

// reprojection reuse, observed: [0] final passes that stored, [1] final passes that loaded, [2] invalidations of the
// plane's tag, [3] bytes of the plane
int rtpt_debug_reproj_info(rtpt_ctx* c, uint64_t out[4]) {
  if (!c || !out) return fail(RTPT_E_INVALID, "NULL argument");
  for (int i = 0; i < 3; i++) out[i] = c->reproj_info[i];
  out[3] = c->reproj.bytes;
  return RTPT_OK;
}

// the deferred final pass, observed: [0] passes recorded instead of launched, [1] of those launched inside a tracing launch,
// [2] launched alone, [3] bytes of the fourth colour buffer
int rtpt_debug_defer_info(rtpt_ctx* c, uint64_t out[4]) {
  if (!c || !out) return fail(RTPT_E_INVALID, "NULL argument");
  for (int i = 0; i < 3; i++) out[i] = c->defer_info[i];
  out[3] = c->color[3].bytes;
  return RTPT_OK;
}

// the last rtpt_raytrace launch, observed: [0] tile columns served one workgroup per tile, [1] run workgroups, [2] tiles served in
// runs, [3] the tiles a run workgroup takes at most (RTPT_EMPTY_RUN)
int rtpt_debug_empty_run_info(rtpt_ctx* c, uint64_t out[4]) {
  if (!c || !out) return fail(RTPT_E_INVALID, "NULL argument");
  for (int i = 0; i < 3; i++) out[i] = c->empty_run_info[i];
  out[3] = static_cast<uint64_t>(c->filter_policy.empty_run);
  return RTPT_OK;
}

int rtpt_debug_live_device_bytes(uint64_t* out) {
  if (!out) return fail(RTPT_E_INVALID, "NULL argument");
  *out = g_live_device_bytes.load();
  return RTPT_OK;
}

// the light list as it stands on the device: *n = its entries, of which the first min(*n, cap) are copied to ids
int rtpt_debug_light_list(rtpt_ctx* c, uint32_t* ids, uint32_t cap, uint32_t* n) {
  if (!c || !n || (cap && !ids)) return fail(RTPT_E_INVALID, "NULL argument");
  const uint32_t have = c->scene.lights.ptr ? c->scene.n_lights : 0u;
  *n = have;
  const uint32_t take = have < cap ? have : cap;
  if (!take) return RTPT_OK;  // no zero-byte copy
  if (static_cast<size_t>(have) * 4 > c->scene.lights.bytes) return fail(RTPT_E_INVALID, "internal: the light list is shorter than its count");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(ids, c->scene.lights.ptr, static_cast<size_t>(take) * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTPT_OK;
}

// ... and the cumulative table of RTPT_FLAG_EXT_NEE_POWER beside it, the same way
int rtpt_debug_light_table(rtpt_ctx* c, uint64_t* cdf, uint32_t cap, uint32_t* n) {
  if (!c || !n || (cap && !cdf)) return fail(RTPT_E_INVALID, "NULL argument");
  const uint32_t have = (c->scene.light_table.cdf.ptr && c->scene.lights.ptr) ? c->scene.n_lights : 0u;
  *n = have;
  const uint32_t take = have < cap ? have : cap;
  if (!take) return RTPT_OK;  // no zero-byte copy
  if (static_cast<size_t>(have) * 8 > c->scene.light_table.cdf.bytes) return fail(RTPT_E_INVALID, "internal: the light table is shorter than its list");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(cdf, c->scene.light_table.cdf.ptr, static_cast<size_t>(take) * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTPT_OK;
}

// the per-pixel normal plane of the filter's edge stop, as it stands on the device
int rtpt_debug_guide_normals(rtpt_ctx* c, float* out, size_t bytes) {
  if (!c || !out) return fail(RTPT_E_INVALID, "NULL argument");
  FLUSH_FILTER(c);
  if (!c->normals.ptr) return fail(RTPT_E_INVALID, "the context has no per-pixel normal plane");
  const size_t need = c->pixels() * 16;
  if (bytes < need || c->normals.bytes < need) return fail(RTPT_E_INVALID, "destination too small");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(out, c->normals.ptr, need, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTPT_OK;
}

// ... and injected: the plane counts as written by K0 for every stored row of the current frame
int rtpt_debug_set_guide_normals(rtpt_ctx* c, const float* src, size_t bytes) {
  if (!c || !src) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  if (!no_pair_table(c)) return fail(RTPT_E_INVALID, "no filter kernel of this context reads per-pixel normals (id-pair table, RTPT_FLAG_EXT_SMOOTH_GUIDE not active)");
  FLUSH_FILTER(c);
  const size_t need = c->pixels() * 16;
  if (bytes < need) return fail(RTPT_E_INVALID, "source too small");
  HIP_TRY(hipSetDevice(c->device));
  if (c->normals.bytes != need)
    if (int rc = alloc_buf(c->normals, need)) return rc;
  reuse_invalidate(c, &c->normals);
  HIP_TRY(hipMemcpyAsync(c->normals.ptr, src, need, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->frame.normals = c->stored_rows();
  c->frame.normals_frame = c->frames_ended;
  return RTPT_OK;
}

// ------------------------------------------------------------------------------------------ the environment map
int rtpt_set_environment(rtpt_ctx* c, const float* texels_rgba, uint32_t n, uint32_t flags, const float* rotation, const float* scale) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  const bool drop = !texels_rgba || !n;
  // everything that can refuse the call comes first: a refused call leaves the environment the context has untouched
  if (!drop)
    if (const char* why = rtpt_env::check_environment(texels_rgba, n, flags, rotation, scale, c->cfg.flags)) return fail(RTPT_E_INVALID, why);
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));  // launches that read the map being replaced
  // K0, K1 and the filter read nothing of it: no plane tag, no scene generation changes — frame reuse and reprojection reuse go on
  if (drop) {
    c->envmap = rtpt_ctx::Environment{};
    return RTPT_OK;
  }
  rtpt_ctx::Environment e;  // joins the context when it is complete; the map it replaces stays until then
  const size_t bytes = 16 * static_cast<size_t>(n) * n;
  if (int rc = alloc_buf(e.texels, bytes)) return rc;
  HIP_TRY(hipMemcpyAsync(e.texels.ptr, texels_rgba, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's array may die at return
  e.n = n;
  e.flags = flags;
  if (rotation) std::memcpy(e.rot, rotation, sizeof e.rot);
  if (scale) std::memcpy(e.scale, scale, sizeof e.scale);
  c->envmap = std::move(e);
  return RTPT_OK;
}

int rtpt_debug_upload_info(rtpt_ctx* c, uint64_t out[4]) {
  if (!c || !out) return fail(RTPT_E_INVALID, "NULL argument");
  for (int i = 0; i < 4; i++) out[i] = c->upload_info[i];
  return RTPT_OK;
}

// ------------------------------------------------------------------------------------------ sync / copies
int rtpt_sync(rtpt_ctx* c) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTPT_OK;
}

int rtpt_readback(rtpt_ctx* c, rtpt_plane which, void* dst, size_t bytes) {
  if (!c || !dst) return fail(RTPT_E_INVALID, "NULL argument");
  FLUSH_FILTER(c);
  Buf* b = which == RTPT_PLANE_IMAGE ? finished_frame(c).buf : plane_buf(c, which);
  if (!b) return fail(RTPT_E_INVALID, "unknown plane");
  if (!b->ptr) return fail(RTPT_E_INVALID, "plane not allocated (scene not uploaded / debug plane not enabled)");
  const size_t need = plane_size(c, which);
  if (bytes < need) return fail(RTPT_E_INVALID, "destination too small");
  HIP_TRY(hipSetDevice(c->device));
  if (which == RTPT_PLANE_RAYCOUNT) {  // kept as partial sums on the device
    unsigned long long part[rt::kRayCounters];
    HIP_TRY(hipMemcpyAsync(part, b->ptr, sizeof part, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    unsigned long long total = 0;
    for (unsigned long long v : part) total += v;
    std::memcpy(dst, &total, sizeof total);
    return RTPT_OK;
  }
  HIP_TRY(hipMemcpyAsync(dst, b->ptr, need, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (const int i = color_index(c, b); i >= 0 && c->frame.alpha_depth[i]) {
    // the reference's colour images have alpha 0; internally alpha carries depth between passes
    float* f = static_cast<float*>(dst);
    for (size_t px = 0, n = need / 16; px < n; px++) f[4 * px + 3] = 0.0f;
  }
  return RTPT_OK;
}

int rtpt_set_plane(rtpt_ctx* c, rtpt_plane which, const void* src, size_t bytes) {
  if (!c || !src) return fail(RTPT_E_INVALID, "NULL argument");
  FLUSH_FILTER(c);
  Buf* b = plane_buf(c, which);
  if (!b) return fail(RTPT_E_INVALID, "unknown plane");
  if (!b->ptr) return fail(RTPT_E_INVALID, "plane not allocated (scene not uploaded / debug plane not enabled)");
  const size_t need = plane_size(c, which);
  if (bytes < need) return fail(RTPT_E_INVALID, "source too small");
  HIP_TRY(hipSetDevice(c->device));
  reuse_invalidate(c, b);
  HIP_TRY(hipMemcpyAsync(b->ptr, src, need, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (const int i = color_index(c, b); i >= 0) c->frame.alpha_depth[i] = false;
  if (which == RTPT_PLANE_PREVIOUS) c->frame.hist = c->stored_rows();
  if (which == RTPT_PLANE_PREV_VIS_ID || which == RTPT_PLANE_MOMENTS_PREV) c->frame.guides = c->stored_rows();
  if (which == RTPT_PLANE_LUT_PREV) {
    c->scene.lut_prev_valid = true;
    c->scene.lut_version[c->lut_cur ^ 1] = ~0ull;  // injected content: rebuild when it becomes current
  }
  if (which == RTPT_PLANE_LUT) c->scene.lut_version[c->lut_cur] = ~0ull;
  if (which == RTPT_PLANE_VIS_ID) c->frame.normals = Rows();  // the normal plane no longer matches the ids
  return RTPT_OK;
}

int rtpt_reset_counters(rtpt_ctx* c) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemsetAsync(c->raycount.ptr, 0, 8 * rt::kRayCounters, c->stream));
  return RTPT_OK;
}

int rtpt_set_count_rows(rtpt_ctx* c, uint32_t y0, uint32_t y1) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (y0 > y1) return fail(RTPT_E_INVALID, "y0 > y1");
  c->frame.count = Rows(y0, y1);
  return RTPT_OK;
}

// ------------------------------------------------------------------------------------------ timing
int rtpt_timing_enable(rtpt_ctx* c, int enable) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  c->timing_period = enable > 0 ? enable : 0;
  return RTPT_OK;
}

int rtpt_timing_collect(rtpt_ctx* c, double ms_sum[RTPT_K_COUNT], uint32_t launches[RTPT_K_COUNT]) {
  if (!c || !ms_sum || !launches) return fail(RTPT_E_INVALID, "NULL argument");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int i = 0; i < RTPT_K_COUNT; i++) {
    ms_sum[i] = 0.0;
    launches[i] = 0;
  }
  for (auto& t : c->timed) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
      ms_sum[t.kernel] += ms;
      launches[t.kernel]++;
    }
    c->event_pool.push_back(t.start);
    c->event_pool.push_back(t.stop);
  }
  c->timed.clear();
  return RTPT_OK;
}

const char* rtpt_kernel_name(rtpt_kernel_id k) {
  switch (k) {
    case RTPT_K_GBUFFER: return "k_gbuffer";
    case RTPT_K_LUT: return "k_lut";
    case RTPT_K_GRADIENT: return "k_gradient";
    case RTPT_K_PATHTRACE: return "k_pathtrace";
    case RTPT_K_ATROUS: return "k_atrous";
    case RTPT_K_ATROUS_FINAL: return "k_atrous_final";
    case RTPT_K_ATROUS_CHAIN: return "k_atrous_chain";
    case RTPT_K_ATROUS_CHAIN_FINAL: return "k_atrous_chain_final";
    case RTPT_K_GBUFFER_GRADIENT: return "k_gbuffer_gradient";
    case RTPT_K_GBUFFER_PATHTRACE: return "k_gbuffer_pathtrace";
    case RTPT_K_PRESENT: return "k_present";
    case RTPT_K_MODULATE: return "k_modulate";
    default: return "?";
  }
}

}  // extern "C"
