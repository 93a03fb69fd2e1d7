// api_internal.hpp — what the translation units of the C ABI (api_*.hip) share: the context, the recording state and the
// helpers every entry point uses.  Nothing here is part of the ABI (include/rtpt.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cfloat>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtpt.h"
#include "bvh.hpp"
#include "kernels.hpp"
#include "rtpt_math.hpp"


namespace rtpt_impl {


extern thread_local std::string g_err;  // rtpt_last_error (api_context.hip)
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                 \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return fail(RTPT_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)

// A device buffer.  Move-only: an owned allocation (alloc_buf) is released by release(), by the destructor and when another
// Buf is moved in; a borrowed pointer (rtpt_bind_plane, owned == false) is never freed.  Every release must run with the
// context's device current: the entry points set it before anything that holds a Buf is replaced or destroyed.
struct Buf {
  void* ptr = nullptr;
  size_t bytes = 0;
  bool owned = false;
  Buf() = default;
  Buf(Buf&& o) noexcept : ptr(o.ptr), bytes(o.bytes), owned(o.owned) { o.ptr = nullptr, o.bytes = 0, o.owned = false; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      release();
      ptr = o.ptr, bytes = o.bytes, owned = o.owned;
      o.ptr = nullptr, o.bytes = 0, o.owned = false;
    }
    return *this;
  }
  ~Buf() { release(); }
  void release();  // api_context.hip: hipFree of an owned allocation (counted, rtpt_debug_live_device_bytes); leaves *this empty
};

enum ColorRole { ROLE_IMAGE = 0, ROLE_FILTERED = 1, ROLE_PREVIOUS = 2 };

struct FilterCall {  // one recorded rtpt_temporal_filter call
  rtpt_push_constants pc;
  rtpt_ubo ubo;
  bool has_ubo;
  uint32_t y0, y1;
};

// A final filter pass that was prepared and not launched (api_passes.hip: filter_launch): the next rtpt_raytrace takes it into
// its launch when it can, every other entry point that launches, exposes or changes anything launches it first, alone
// (final_flush).  Roles, tags and FrameState already say what they say after the launch.
struct DeferredFinal {
  rt::AtrousArgs args;  // finished: what launch_atrous or launch_pathtrace takes
  int kernel;           // for the timer of a launch of its own
};

struct TimedLaunch {
  int kernel;
  hipEvent_t start, stop;
};

// Frame reuse: K0 and K1 are functions of what these keys hold and of nothing else (no frame number, no random stream), so a
// plane that still carries the key of the pass about to write it already holds that pass's output.  Compared as bytes
// (new_key zero-fills the padding); a float that compares equal with other bits (-0) only costs a recomputation.
struct K0Key {
  float org[3], c0[3], c1[3], c2[3];  // camera origin and basis
  float PV[16], p00, p11, tmax;
  int32_t W, H, row_base, y0, y1;
  int32_t normals_on;                 // the per-pixel normal plane is written too
  int32_t guide;                      // ... with guide normals (RTPT_FLAG_EXT_SMOOTH_GUIDE is active), formed with ...
  int32_t guide_sigma_n;              // ... this exponent in the self weight; both 0 without
  uint64_t model_version, scene_gen;
};
struct K1Key {
  K0Key k0;
  float cam[3], light[3], light_prev[3], color[3], color_prev[3];
  int32_t y0, y1;
  uint64_t lut_version[2];            // of LUT and LUT_PREV, in that order
};
// Reprojection reuse: the pixel pair the final filter pass reprojects to (device_common.hpp: reproject_pixel) is a function
// of the world-position plane and the id plane (both the output of the K0 call with key k0), the bytes of LUT_PREV, PVprev
// and the frame size (in k0), over the rows the pass covers.
struct ReprojKey {
  K0Key k0;               // carried by tag_worldpos and by the tag of the id plane the pass reads
  uint64_t lut_version;   // of the buffer that is LUT_PREV; never ~0 (injected content)
  float PVprev[16];
  int32_t y0, y1;         // rows of the final pass
};
template <class K>
inline K new_key() {
  K k;
  std::memset(&k, 0, sizeof k);
  return k;
}
template <class K>
struct PlaneTag {  // what a plane the context owns holds: the output of the pass with this key, over the key's rows
  bool valid = false;
  K key;
  bool holds(const K& k) const { return valid && std::memcmp(&key, &k, sizeof k) == 0; }
};

struct Rows {  // frame rows [y0, y1)
  int y0, y1;
  Rows(int64_t a = 0, int64_t b = 0) : y0(static_cast<int>(a)), y1(static_cast<int>(b)) {}
  bool covers(int64_t a, int64_t b) const { return y0 <= a && y1 >= b; }
  void extend(int64_t a, int64_t b) { *this = Rows(std::min<int64_t>(y0, a), std::max<int64_t>(y1, b)); }
};

// The frames rendered so far at this size: which buffer plays which part and which rows of it mean something.  One value:
// alloc_planes replaces it whole, so a member added here is reset by rtpt_resize without being listed anywhere.
struct FrameState {
  int color_of_role[3] = {0, 1, 2};             // role -> physical index of rtpt_ctx::color
  int color_spare = 3;    // the buffer no role names: the trace that carries a deferred final pass writes it (rtpt_ctx::deferred)
  bool alpha_depth[4] = {false, false, false, false};  // physical buffer carries depth in alpha ("rgbd")
  int vis_cur = 0;        // vis[vis_cur] = VIS_ID, the other PREV_VIS_ID
  int moments_cur = 0;    // moments[moments_cur] is written this frame, the other one is the history
  int variance_last = 0;  // variance[] buffer holding the newest values
  bool final_swapped = false;  // the final filter pass already rotated IMAGE <-> FILTERED this frame
  bool image_alias = false;    // between rtpt_end_frame and the next rtpt_raytrace IMAGE reads as PREVIOUS
  Rows final;    // of IMAGE the frame's last filter iteration wrote
  Rows hist;     // of PREVIOUS holding a valid previous frame
  Rows guides;   // of the context's own previous id / moment planes that hold a previous frame
  Rows normals;  // of rtpt_ctx::normals that match VIS_ID ...
  uint64_t normals_frame = ~0ull;  // ... in this frame (frames_ended)
  const void* ext_history = nullptr;  // rtpt_set_external_history
  Rows ext_hist;
  const void* ext_prev_vis = nullptr;  // rtpt_set_external_guides: previous frame's ids / moments gathered across strips
  const void* ext_moments = nullptr;
  Rows ext_guides;
  void* present_fused_dst = nullptr;  // what the last final pass wrote of rtpt_ctx::present_dst: rtpt_present skips its launch
  Rows present_fused;
  Rows count;  // counted into RAYCOUNT: the stored rows until rtpt_set_count_rows
  explicit FrameState(Rows stored = Rows()) : count(stored) {}
};

// The acceleration structure over Scene::tris.  One value: rtpt_scene_rebuild swaps a whole Tree in (api_scene.hip).
struct Tree {
  Buf nodes, leaf_order;
  // device-side refit (refit.hip): nodes sorted by height, scratch boxes, the slice of the order per height (levels + 1)
  Buf refit_order, refit_fbox;
  std::vector<uint32_t> refit_level_first;
  uint32_t n_nodes = 0;
  int bvh_depth = 0;
  bool leaf_pairs = false;   // built over fan pairs (bvh.hpp build_bvh(pairs)): every leaf is one pair (2q, 2q + 1)
  bool device_tree = false;  // built on the device: bvh_host is empty, every refit runs on the device
  rt::Bvh bvh_host;          // a host-built tree's topology, for the host refit
  rt::BvhGrid bvh_grid{};    // of the host-built / host-refit node boxes (bvh_grid_dev is what the traversal reads)
};

// Everything that belongs to the uploaded scene.  rtpt_scene_upload assembles a new one and moves it into the context when
// it is complete; n_tris == 0 is "no scene" (RTPT_E_NO_SCENE).
struct Scene {
  uint32_t n_tris = 0;       // flattened: n_instances * n_base_tris
  uint32_t n_base_tris = 0;
  uint32_t n_instances = 0;  // of the upload; 1 with has_xf false: uploaded without transforms
  bool has_xf = false;
  Buf tris, isect_id, isect_leaf, shade;  // posed triangles and the records made from them (scene_prepare)
  Buf obj_tris_dev;                       // the un-posed triangles (instance transforms applied, model not)
  Buf bvh_grid_dev;                       // the grid of the node boxes, as the traversal reads it (a refit rewrites it)
  Tree tree;
  // instances (scene_flatten.hip): the mesh and its instance transforms, resident on the device for RTPT_FLAG_DEVICE_FLATTEN
  // uploads and from the first rtpt_scene_set_instances on (12 n_verts + 12 n_tris + 48 n_instances bytes); the host keeps
  // the mesh too (the host path re-flattens from it)
  struct DeviceMesh {
    Buf xyz, idx, xf;
  } mesh_dev;
  std::vector<float> mesh_xyz;
  std::vector<uint32_t> mesh_idx;
  bool use_bvh = false;
  bool tris_paired = false;  // every (2q, 2q+1) is a fan pair: same v0, v2_A == v1_B bitwise (closest_hit.hpp tri_pair_test)
  std::vector<float> host_tris;  // flattened world-space triangles, kept for small scenes (screen bounds)
  // animated model matrix (main.cpp:1469 recomputes ubo.model every frame; it is the identity there): the scene as
  // uploaded (object space), and the model it is posed with.  obj_tris is kept where the host reads it: scenes small
  // enough for screen bounds and scenes re-posed on the host
  std::vector<float> obj_tris;
  float model[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  uint64_t model_version = 0;                // bumped whenever the posed geometry changes
  Buf lut[2], normal_tab, pair_tab;          // rtpt_ctx::lut_cur says which LUT is the current one
  uint64_t lut_version[2] = {~0ull, ~0ull};  // model_version each LUT buffer was built for
  bool lut_prev_valid = false;               // D3
  Buf materials;                             // optional per-base-triangle (Kd, Ke) records, rtpt_scene_set_materials
  int materials_specular = 0;                // 1: some triangle's record is specular (rtpt_scene_set_materials_ext), 2: some
                                             // triangle's is a dielectric — the SPEC kernels; 0: every record is diffuse
  // RTPT_FLAG_EXT_NEE: the light list (light_list_host.hpp), id + 1 of every posed emissive triangle, built beside the material
  // records on a context with the flag and dropped with them; empty (no allocation) without the flag or without an emitter.  An
  // upload drops it with the scene; moved instances, a rebuilt tree, a changed model and a resize keep it: ids do not change
  Buf lights;
  uint32_t n_lights = 0;
  // RTPT_FLAG_EXT_NEE_POWER (with RTPT_FLAG_EXT_NEE, and a list with entries; no allocation otherwise): the cumulative table of
  // the weighted pick, 8 bytes an entry, and the builder's work area (rt::light_table_scratch_bytes).  Joined and dropped with
  // the list; rebuilt on the context's stream behind every launch_scene_prepare, so that it belongs to the shade records a trace
  // reads (api_scene.hip: rebuild_light_table)
  struct LightTable {
    Buf cdf, scratch;
  } light_table;
  // optional albedo textures, rtpt_scene_set_textures: per-base-triangle uv records, descriptors, the RGBA32F atlas
  struct Textures {
    Buf records, desc, texels;
    Buf levels;  // the level table, only when some texture has RTPT_TEX_MIPMAP; texels then also holds the generated levels
    uint32_t n_textures = 0;
  } textures;
  // optional vertex normals, rtpt_scene_set_normals (shading_normal.hpp): the per-base-triangle corner normals and the cofactor
  // matrix of every instance's pose, 48 bytes each.  The table follows the pose: repose_scene rebuilds it (api_scene.hip:
  // rebuild_normal_cof) on the context's stream from the model and the instance transforms — on the device route from the
  // transforms as they stand on the device (mesh_dev.xf where it holds them, xf_dev_current; else `xf`, this struct's own
  // copy), on the host route from inst_xf.  While the records exist the scene traces through its tree (use_bvh).
  struct Normals {
    Buf records, cof;
    Buf xf;  // the instance transforms, where mesh_dev.xf does not hold them
    bool xf_current = false;  // ... and it holds inst_xf
    std::vector<float> cof_host;  // the host route's staging for `cof`
  } normals;
  // the instance transforms as last given (12 floats each), kept where the device mesh does not hold them (a host-flattened
  // upload, the host route's moves) and while the scene has normals; a scene with transforms has them here, there, or both
  std::vector<float> inst_xf;
  bool xf_dev_current = false;  // mesh_dev.xf holds the transforms as last given
  struct rtpt_scene_build_info build_info {};
  bool build_ms_pending = false;  // build_ms is still in rtpt_ctx::build_ev; read lazily by rtpt_scene_build_info
};

}  // namespace rtpt_impl
using namespace rtpt_impl;

struct rtpt_ctx {
  rtpt_config cfg;
  int device = 0;
  int n_cu = 256;  // compute units of `device` (persistent-grid sizes); per context, not per process
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;

  Buf color[4];  // physical RGBA32F buffers (FrameState::color_of_role, color_spare); [3] is allocated by the first trace that
                 // carries a deferred final pass
  Buf vis[2];
  int lut_cur = 0;  // scene.lut[lut_cur] = LUT, the other LUT_PREV
  Buf worldpos, gradient, depth, prev_pixel, hit_id, raycount;
  Buf moments[2], variance[2];  // RTPT_FLAG_EXT_VARIANCE
  Buf var_scale;                // RTPT_FLAG_EXT_SVGF_VARIANCE: the prefiltered variance of the iteration being launched
  Buf albedo, shaded;           // RTPT_FLAG_EXT_DEMODULATE: the first hit's albedo (rtpt_raytrace) and the frame times it (rtpt_modulate)
  Buf path_queue[2], path_queue_count;  // long paths: survivors handed from one k_pathtrace launch to the next
  Buf normals;                  // per-pixel normal plane for the LDS-staged filter of scenes without an id-pair table
  FrameState frame;             // reset by alloc_planes (rtpt_create, rtpt_resize); everything else here survives a resize
  // rtpt_present_target: the swapchain image rows the NEXT final pass also writes (fused blit)
  void* present_dst = nullptr;
  Rows present_rows;
  Buf ray_tab;  // K0: view-space ray direction per column / per row, for the projection and size below
  float ray_tab_p00 = 0.f, ray_tab_p11 = 0.f;
  uint32_t ray_tab_w = 0, ray_tab_h = 0;

  // The scene.  The context owns every device buffer through a Buf member, of itself or of the scene: `delete` frees
  // them all.  What follows the scene here survives an upload: switches, the builder's work area, staging, counters.
  Scene scene;
  // The environment map (rtpt_set_environment; env.hpp): of the context, not of the scene — it survives uploads, resizes and
  // everything between.  texels: exactly 16 n^2 bytes; empty without an environment
  struct Environment {
    Buf texels;
    uint32_t n = 0, flags = 0;
    float rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};  // row-major
    float scale[3] = {1, 1, 1};
  } envmap;
  bool no_pairing = false;   // RTPT_NO_TRI_PAIRS=1: A/B switch
  bool host_refit = false;   // RTPT_HOST_REFIT=1: round 2's host path for every scene (A/B)
  // device-side BVH build (bvh_build.hip): RTPT_FLAG_DEVICE_BVH_BUILD, or RTPT_DEVICE_BVH=1 at rtpt_create
  bool device_bvh = false;      // rtpt_scene_upload builds the tree on the device
  bool device_bvh_sah = false;  // ... with the SAH builder (bvh_build_sah.hip): RTPT_FLAG_DEVICE_BVH_SAH too, or RTPT_DEVICE_BVH=sah
  bool lbvh_by_height = false;  // RTPT_LBVH_ORDER=height: the device builder's other node numbering (A/B; same pixels)
  bool device_flatten = false;  // RTPT_FLAG_DEVICE_FLATTEN (with device_bvh)
  Buf bvh_build_scratch, bvh_build_header;  // the builder's work area (grows, never shrinks) and its readback words
  hipEvent_t build_ev[2] = {nullptr, nullptr};  // around a device build (Scene::build_ms_pending)
  Buf pair_word;  // the device's fan-pair decision (scene_flatten.hip), read back by a device-flatten upload
  // pinned staging for the transforms of a rtpt_scene_set_instances call, two in turn, so that the copy needs no
  // synchronisation and the caller's array may die at return
  struct XfStage {
    void* host = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
  } xf_stage[2];
  int xf_stage_cur = 0;
  uint64_t upload_info[4] = {0, 0, 0, 0};  // rtpt_debug_upload_info

  bool tables_valid = false;  // normal / id-pair tables match the scene
  uint32_t debug_mask = 0;
  hipEvent_t handoff_event = nullptr;  // rtpt_stream_wait(x, this): recorded on this context's stream

  // K0 recorded by rtpt_gbuffer: launched together with K1 when rtpt_temporal_gradient follows at once, alone otherwise
  rt::GbufferArgs pending_gb{};
  bool pending_gb_valid = false;
  // recorded K0 (+ K1): rtpt_raytrace right behind them launches all three as one grid (kernels.hip: k_gbuffer_pathtrace);
  // RTPT_NO_TRACE_FUSION=1 (read at rtpt_create) keeps K0 + K1 a launch of their own for A/B runs
  bool fuse_trace = true;
  // Frame reuse (api_passes.hip: reuse_covers): while camera, light and scene rest, the recorded K0 + K1 would rewrite the
  // planes with the bytes they hold, so neither is launched.  vis[] rotates at rtpt_end_frame — the buffer about to be
  // written holds the frame before last — hence the third consecutive frame with equal keys is the first one served.
  // RTPT_NO_FRAME_REUSE=1 (read at rtpt_create) turns it off.
  bool frame_reuse = true;
  uint64_t scene_gen = 0;  // bumped by everything that changes the geometry or the tree the passes traverse
  K1Key pending_key;       // of pending_gb (k0 from rtpt_gbuffer, the rest once rtpt_temporal_gradient joined it)
  PlaneTag<K0Key> tag_vis[2], tag_worldpos, tag_depth, tag_normals;
  PlaneTag<K1Key> tag_gradient;
  uint64_t reuse_info[4] = {0, 0, 0, 0};  // rtpt_debug_reuse_info
  // Reprojection reuse (api_passes.hip: reproj_policy): a single-launch final pass of the plain comb kernel whose ReprojKey
  // equals the previous frame's stores its reprojected pixels, packed to 4 bytes, into `reproj`; from then on, while the key
  // holds, the pass loads them instead of reprojecting.  `reproj` is allocated at the first store.  A moving camera changes
  // the key every frame and never stores.  RTPT_NO_REPROJ_REUSE=1 (read at rtpt_create) turns it off; so does
  // RTPT_NO_FRAME_REUSE=1, without which no plane tag is ever valid.
  bool reproj_reuse = true;
  Buf reproj;
  PlaneTag<ReprojKey> tag_reproj;       // what `reproj` holds
  PlaneTag<ReprojKey> reproj_last;      // the key of the previous frame's final pass (valid: that pass was eligible)
  uint64_t reproj_info[4] = {0, 0, 0, 0};  // rtpt_debug_reproj_info ([3] is read from `reproj`)
  // K2 of scenes whose BVH is built over fan pairs as the path-pool kernel (kernels.hip: k_pathtrace_pool): RTPT_TRACE_POOL
  // (read at rtpt_create); path_pool = the workgroups' slabs, allocated on first use
  bool trace_pool = false;
  // segments of a path the tile kernel runs before the survivors go through the queue kernels (kernels.hpp: pt_first_window is
  // the default); RTPT_PT_WINDOW at rtpt_create, 0 = the default
  uint32_t trace_window = 0;
  float tex_bounce_spread = rt::kTexBounceSpread;  // RTPT_TEX_BOUNCE_SPREAD, for measurements only (texture.hpp)
  Buf path_pool;
  rt::FilterPolicy filter_policy;  // RTPT_CHAIN_*, RTPT_FINAL_FRONT (read once, here: rtpt_create)
  // The last final pass, deferred (DeferredFinal): RTPT_NO_FINAL_DEFER=1 (read at rtpt_create) launches every pass where it is
  // recorded, as before
  bool final_defer = true;
  bool deferred_valid = false;
  DeferredFinal deferred;
  uint64_t defer_info[4] = {0, 0, 0, 0};  // rtpt_debug_defer_info
  uint32_t empty_run_info[3] = {0, 0, 0};  // rtpt_debug_empty_run_info: the last tracing launch
  // K3 iterations recorded by rtpt_temporal_filter and not launched yet (see filter_flush)
  std::vector<FilterCall> pending;
  int chain_max = 2;        // iterations per chained launch (1 = never chain)
  bool chain_final = false; // may a chain end in the FINAL pass
  // A chain slides down column strips in row segments and pays sum(s) + lag rows of pipeline fill per segment: with
  // fewer pixels than this per launch the segments that fill the GPU are too short for that to pay, so smaller launches
  // run one kernel per iteration (measured, pair vs 2 separate: 4K 98 vs 128 us, 1080p 38.2 vs 40.3, a 300-row strip of
  // 3840 columns 27.1 vs 28.9 — the kernel itself no longer wins there, the launch it saves does: frame 0.171 vs 0.173 ms)
  int64_t chain_min_pixels = 1000000;

  // timing
  // BVH traversal: stack entries per lane kept in LDS (kernels.hpp SceneView::stack_lds) and the global-memory home of
  // the deeper ones, sized for the largest grid that traverses (ensure_stack_spill)
  int bvh_stack_lds = 16;
  Buf stack_spill;
  size_t stack_spill_blocks = 0;

  int timing_period = 0;          // 0 off, n: kernels of every n-th frame are bracketed by events
  uint64_t frames_ended = 0;
  bool timing_now() const { return timing_period > 0 && (frames_ended % static_cast<uint64_t>(timing_period)) == 0; }
  std::vector<TimedLaunch> timed;
  std::vector<hipEvent_t> event_pool;

  uint32_t rows() const { return cfg.row_end - cfg.row_begin; }
  Rows stored_rows() const { return Rows(cfg.row_begin, cfg.row_end); }
  bool width_fits_i16() const { return cfg.width < 30000 && cfg.height < 30000; }
  size_t pixels() const { return static_cast<size_t>(rows()) * cfg.width; }
};

namespace rtpt_impl {

// K3 iterations recorded by rtpt_temporal_filter are launched before anything else looks at or changes the planes
int filter_flush(rtpt_ctx* c, bool fuse);
int gbuffer_flush(rtpt_ctx* c);
int final_flush(rtpt_ctx* c);  // a deferred final pass goes out, alone (no-op without one)
// frame reuse: something other than K0 / K1 may write plane b (NULL: any plane) — its tag no longer describes it
void reuse_invalidate(rtpt_ctx* c, const Buf* b);
#define FLUSH_FILTER(c)                              \
  do {                                               \
    int rcf_ = final_flush(c);                       \
    if (rcf_ == RTPT_OK) rcf_ = gbuffer_flush(c);    \
    if (rcf_ == RTPT_OK) rcf_ = filter_flush((c), false); \
    if (rcf_) return rcf_;                           \
  } while (0)

int alloc_buf(Buf& b, size_t bytes);
void free_buf(Buf& b);

size_t frame_blocks(const rtpt_ctx* c);
int ensure_stack_spill(rtpt_ctx* c, size_t blocks);
Buf* plane_buf(rtpt_ctx* c, rtpt_plane which);
size_t plane_size(const rtpt_ctx* c, rtpt_plane which);
int check_rows(const rtpt_ctx* c, uint32_t& y0, uint32_t& y1);
rt::FrameGeom geom(const rtpt_ctx* c, uint32_t y0, uint32_t y1);
rt::SceneView scene_view(const rtpt_ctx* c);
rt::TexView tex_view(const rtpt_ctx* c);  // the albedo textures, all NULL without (rtpt_scene_set_textures)
rt::LightTableView light_view(const rtpt_ctx* c);  // the light list, NULL and 0 without (Scene::lights), and its table or NULL
rt::NormalView normal_view(const rtpt_ctx* c);     // the vertex normals, both NULL without (rtpt_scene_set_normals), and the guide switch
rt::EnvView env_view(const rtpt_ctx* c);           // the environment map, texels NULL without (rtpt_set_environment)
// RTPT_FLAG_EXT_SMOOTH_GUIDE is active: the context has the flag and the scene holds normals.  K0 then writes guide normals into
// rtpt_ctx::normals, and the context behaves as if the scene had no id-pair table
bool guide_active(const rtpt_ctx* c);
inline bool no_pair_table(const rtpt_ctx* c) { return !c->scene.pair_tab.ptr || guide_active(c); }
bool screen_bounds(const rtpt_ctx* c, const double org[3], const double c0[3], const double c1[3], const double c2[3], double p00, double p11,
                   double jitter_px, rt::TriBounds* out);
bool is_identity(const float* m);
int launch_check(const char* what);
int color_index(const rtpt_ctx* c, const Buf* b);  // of c->color, -1 for any other buffer
// The finished frame: IMAGE until rtpt_end_frame, PREVIOUS after it (the reference blits before it copies, the pixels are the
// same); only the rows the last final pass wrote hold it
struct FinishedFrame {
  Buf* buf;
  Rows rows;
};
FinishedFrame finished_frame(rtpt_ctx* c);
int apply_model(rtpt_ctx* c, const float* model);  // api_scene.hip
void build_tables(rtpt_ctx* c);                      // api_passes.hip: k_lut + k_pair_weights for the posed scene
int ensure_tables(rtpt_ctx* c);                      // api_passes.hip: build_tables + the D3 LUTprevious, when the tables are stale

// HIP events around a launch on the launch stream, every rtpt_timing_enable(period)-th frame (rtpt_timing_collect)
struct Timer {
  rtpt_ctx* c;
  bool on;
  TimedLaunch t;
  Timer(rtpt_ctx* ctx, int kernel) : c(ctx), on(ctx->timing_now()) {
    if (!on) return;
    t.kernel = kernel;
    for (hipEvent_t* e : {&t.start, &t.stop}) {
      if (!c->event_pool.empty()) {
        *e = c->event_pool.back();
        c->event_pool.pop_back();
      } else if (hipEventCreateWithFlags(e, hipEventDisableSystemFence) != hipSuccess) {
        // (timing only: without the system-scope fence a record does not write back and invalidate the caches, which is
        // what made a bracketed launch cost ~5 us and a fully bracketed frame 6 %)
        on = false;
        return;
      }
    }
    (void)hipEventRecord(t.start, c->stream);
  }
  ~Timer() {
    if (!on) return;
    (void)hipEventRecord(t.stop, c->stream);
    c->timed.push_back(t);
  }
};

}  // namespace rtpt_impl
