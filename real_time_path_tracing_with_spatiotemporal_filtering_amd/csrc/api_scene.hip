// api_scene.hip — the scene side of the C ABI: rtpt_scene_upload (loadMesh + buildAccelerationStructure, main.cpp:409-462,
// :687-742; flattened on the host, or on the device: scene_flatten.hip), instances that move between frames
// (rtpt_scene_set_instances), the posed scene of a changed ubo.model (device-side refit, refit.hip), materials.
#include "api_internal.hpp"
#include "light_list_host.hpp"
#include "material_host.hpp"
#include "normal_host.hpp"
#include "shading_normal.hpp"
#include "texture_host.hpp"

#include <chrono>

namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

rt::ScenePrepArgs scene_prep_args(const Scene& s) {
  rt::ScenePrepArgs sp;
  sp.n_tris = s.n_tris;
  sp.tris = static_cast<const float*>(s.tris.ptr);
  sp.leaf_order = static_cast<const uint32_t*>(s.tree.leaf_order.ptr);
  sp.isect_id = static_cast<float4*>(s.isect_id.ptr);
  sp.isect_leaf = static_cast<float4*>(s.isect_leaf.ptr);
  sp.shade = static_cast<float4*>(s.shade.ptr);
  sp.leaf_pairs = s.tree.leaf_pairs ? 1u : 0u;
  return sp;
}
// what follows every launch_scene_prepare: the cumulative light table of RTPT_FLAG_EXT_NEE_POWER, where the scene has one
// (defined beside the light list below)
void rebuild_light_table(rtpt_ctx* c, Scene& s);

// ... and the cofactor table of smooth shading, where the scene has vertex normals (rtpt_scene_set_normals): it follows the pose,
// so repose_scene — the one routine that re-poses — rebuilds it on both of its routes (defined beside the entry point below)
int rebuild_normal_cof(rtpt_ctx* c, Scene& s, const float* model, bool on_device);

rt::RefitArgs refit_args(const Scene& s) {
  rt::RefitArgs ra;
  ra.tris = static_cast<const float*>(s.tris.ptr);
  ra.leaf_order = static_cast<const uint32_t*>(s.tree.leaf_order.ptr);
  ra.order = static_cast<const uint32_t*>(s.tree.refit_order.ptr);
  ra.nodes = static_cast<rt::BvhNodeQ*>(s.tree.nodes.ptr);
  ra.fbox = static_cast<float*>(s.tree.refit_fbox.ptr);
  ra.grid = static_cast<float*>(s.bvh_grid_dev.ptr);
  return ra;
}

// a device-built tree has no host copy (bvh_host is empty): it is refit on the device whatever traces the scene —
// also the small scenes that trace by brute force, whose host_tris are still re-posed on the host
bool refits_on_device(const rtpt_ctx* c, const Scene& s) {
  return ((s.use_bvh && !c->host_refit) || s.tree.device_tree) && s.obj_tris_dev.ptr && s.tree.refit_order.ptr;
}

// the traversal addresses leaf records and nodes as base + 32-bit byte offset (48 bytes per triangle at most, 32 per node);
// the kernels of the device routes index 3 x total vertices in 32 bits, a looser limit.  A device-built tree has fewer
// nodes than triangles, so for it the first test implies the second
int check_record_offsets(uint64_t total, uint64_t n_nodes) {
  if (total * 48u >= (1ull << 32) || n_nodes >= (1ull << 27))
    return fail(RTPT_E_INVALID, "scene too large for the traversal's 32-bit record offsets (more than 89,478,485 triangles)");
  return RTPT_OK;
}

// The frame state that described the scene or the tree that was just replaced: tables, the per-pixel normal plane, the
// spill area (sized by the replaced tree's depth), and what frame reuse and the LUTs compare.  Every replacement calls it.
void forget_scene(rtpt_ctx* c) {
  c->tables_valid = false;
  c->frame.normals = Rows();
  free_buf(c->stack_spill);
  c->stack_spill_blocks = 0;
  c->scene.model_version++;
  c->scene_gen++;  // another tree may resolve a tie between equally near triangles differently
}

// the posed scene changed under the same tree topology: LUT, per-id normals and pair weights, and frame reuse follow
void mark_reposed(rtpt_ctx* c, const float* model) {
  std::memmove(c->scene.model, model, sizeof c->scene.model);
  c->scene.model_version++;
  c->scene_gen++;
  c->tables_valid = false;
}

// The device buffers of a scene of `total` triangles, the tree excepted, with both LUTs cleared.
int alloc_scene(rtpt_ctx* c, Scene& s, uint32_t total) {
  int rc;
  const size_t n = total, tri_bytes = n * 9 * sizeof(float);
  if ((rc = alloc_buf(s.tris, tri_bytes)) || (rc = alloc_buf(s.obj_tris_dev, tri_bytes))) return rc;
  if ((rc = alloc_buf(s.isect_id, n * 48)) || (rc = alloc_buf(s.isect_leaf, n * 48)) || (rc = alloc_buf(s.shade, n * 48))) return rc;
  if ((rc = alloc_buf(s.normal_tab, (n + 1) * 32))) return rc;  // normals, then per-id areas
  if ((rc = alloc_buf(s.pair_tab, total + 1 <= 64 ? (n + 1) * (total + 1) * 4 : 0))) return rc;
  if ((rc = alloc_buf(s.bvh_grid_dev, 8 * sizeof(float)))) return rc;
  for (Buf& lut : s.lut) {
    if ((rc = alloc_buf(lut, (n + 1) * sizeof(rtpt_visibility_data)))) return rc;
    HIP_TRY(hipMemsetAsync(lut.ptr, 0, lut.bytes, c->stream));
  }
  s.n_tris = total;
  return RTPT_OK;
}

int alloc_tree(Tree& t, size_t n_nodes, size_t total) {
  int rc;
  if ((rc = alloc_buf(t.nodes, n_nodes * sizeof(rt::BvhNodeQ))) || (rc = alloc_buf(t.leaf_order, total * 4))) return rc;
  if ((rc = alloc_buf(t.refit_order, n_nodes * 4))) return rc;
  return alloc_buf(t.refit_fbox, n_nodes * 12 * sizeof(float));
}

// Where every upload route starts, after all that can refuse the call on the host.  The stream drains, and the previous
// scene (with what a route that gave up left in `s`) releases its memory BEFORE the new one's is allocated: a large scene
// is never resident twice.  From here to the commit the context has no scene: a failure leaves RTPT_E_NO_SCENE, never
// a count over buffers of another size.
int begin_scene(rtpt_ctx* c, Scene& s, uint32_t total) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->scene = Scene{};
  s = Scene{};
  forget_scene(c);
  return alloc_scene(c, s, total);
}

// the host-flattened triangles: posed (a fresh upload stands under the identity model) and un-posed
int upload_tris(rtpt_ctx* c, Scene& s, const std::vector<float>& tris) {
  const size_t tri_bytes = tris.size() * sizeof(float);
  HIP_TRY(hipMemcpyAsync(s.tris.ptr, tris.data(), tri_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(s.obj_tris_dev.ptr, tris.data(), tri_bytes, hipMemcpyHostToDevice, c->stream));
  c->upload_info[0] += 2 * tri_bytes;
  return RTPT_OK;
}

// the grid of a host-built or host-refit tree, to where the traversal reads it (a device-side refit writes these words
// itself).  `stage` is the caller's: it lives until the caller synchronises
int upload_grid(rtpt_ctx* c, Scene& s, float (&stage)[8]) {
  for (int i = 0; i < 3; i++) stage[i] = s.tree.bvh_grid.origin[i], stage[3 + i] = s.tree.bvh_grid.cell[i];
  stage[6] = stage[7] = 0.f;
  HIP_TRY(hipMemcpyAsync(s.bvh_grid_dev.ptr, stage, sizeof stage, hipMemcpyHostToDevice, c->stream));
  return RTPT_OK;
}

// world triangle = model * uploaded triangle, in the fixed-order fma arithmetic the LUT uses (mat_row_point)
void host_pose(const float* model, const std::vector<float>& obj, std::vector<float>& out) {
  const bool ident = is_identity(model);
  out.resize(obj.size());
  for (size_t v = 0; v < obj.size(); v += 3) {
    const rt::f3 q{obj[v], obj[v + 1], obj[v + 2]};
    for (int r = 0; r < 3; r++) out[v + r] = ident ? obj[v + r] : rt::exact::mat_row_point(model, r, q);
  }
}

// device-side refit table of a host-built tree: its nodes by HEIGHT (a node after both of its subtrees) and the slice of
// that order per height
void nodes_by_height(const std::vector<rt::BvhNodeQ>& nodes, std::vector<uint32_t>& order, std::vector<uint32_t>& level_first) {
  const size_t nn = nodes.size();
  std::vector<int> height(nn, 0);
  int maxh = 0;
  for (size_t ii = nn; ii-- > 0;) {  // pre-order numbering: children carry larger indices than their parent
    int hgt = 0;
    for (uint32_t ref : {nodes[ii].lref, nodes[ii].rref})
      if (ref != rt::kBvhEmpty && !(ref & 0x80000000u) && ref < nn) hgt = std::max(hgt, height[ref] + 1);
    height[ii] = hgt;
    maxh = std::max(maxh, hgt);
  }
  level_first.assign(static_cast<size_t>(maxh) + 2, 0);
  for (size_t ii = 0; ii < nn; ii++) level_first[static_cast<size_t>(height[ii]) + 1]++;
  for (size_t h = 1; h < level_first.size(); h++) level_first[h] += level_first[h - 1];
  order.resize(nn);
  std::vector<uint32_t> fill(level_first.begin(), level_first.end() - 1);
  for (size_t ii = 0; ii < nn; ii++) order[fill[static_cast<size_t>(height[ii])]++] = static_cast<uint32_t>(ii);
}

// what rtpt_scene_build_info says about the tree `s` stands on (upload_ms is the entry point's)
void set_build_info(Scene& s, uint32_t builder, uint32_t fallback, float build_ms) {
  s.build_info.builder = builder;
  s.build_info.fallback = fallback;
  s.build_info.n_primitives = s.tree.leaf_pairs ? s.n_tris / 2 : s.n_tris;
  s.build_info.n_nodes = s.tree.n_nodes;
  s.build_info.depth = static_cast<uint32_t>(s.tree.bvh_depth);
  s.build_info.leaf_pairs = s.tree.leaf_pairs ? 1u : 0u;
  s.build_info.build_ms = build_ms;
}

// The tree over s.tris (as they stand on the device) built on the device (bvh_build.hip, or bvh_build_sah.hip with
// c->device_bvh_sah: fewer nodes than primitives - 1 where a leaf holds two triangles) and swapped into `s` as one value:
// nodes, leaf order, nodes by height, depth; then the refit that fills boxes and grid and the leaf records.  Built
// aside, so a tree deeper than the traversal stack (*too_deep, RTPT_OK) or an error leaves the tree of `s` as it was.  `s`
// is a scene being uploaded (alloc_scene) or the context's own (rtpt_scene_rebuild); the stream must be idle on entry.
// The LBVH synchronises ONCE, for the readback of kLbvhHeaderWords dwords; the SAH build also synchronises inside
// launch_sah_build, once at its start and one to three times per level of the tree (its segment counts come back to the host).
int device_build_tree(rtpt_ctx* c, Scene& s, bool leaf_pairs, bool* too_deep) {
  *too_deep = false;
  const bool sah = c->device_bvh_sah;
  const uint32_t total = s.n_tris, w = leaf_pairs ? 2u : 1u, n_prims = total / w;
  uint32_t n_nodes = n_prims > 1 ? n_prims - 1 : 1;  // the SAH builder may write fewer: its header says how many
  const size_t need = sah ? rt::sah_scratch_bytes(n_prims) : rt::lbvh_scratch_bytes(n_prims, c->lbvh_by_height);
  if (!need) return fail(RTPT_E_DEVICE, "device BVH build: the sort's temporary-storage query failed");
  int rc;
  if (c->bvh_build_scratch.bytes < need && (rc = alloc_buf(c->bvh_build_scratch, need))) return rc;
  if (!c->bvh_build_header.ptr && (rc = alloc_buf(c->bvh_build_header, rt::kLbvhHeaderWords * 4))) return rc;
  for (hipEvent_t& e : c->build_ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  // The new tree until the swap, the replaced one after it.  The replaced tree (and its host copy: tens of megabytes to
  // unmap for a large scene) is freed where `t` goes out of scope, after the refit and the events are enqueued: hipFree
  // waits for the device, and the refit should not wait behind it
  Tree t;
  if ((rc = alloc_tree(t, n_nodes, total))) return rc;
  rt::LbvhArgs la;
  la.n_prims = n_prims;
  la.prim_w = w;
  la.tris = static_cast<const float*>(s.tris.ptr);
  la.nodes = static_cast<rt::BvhNodeQ*>(t.nodes.ptr);
  la.leaf_order = static_cast<uint32_t*>(t.leaf_order.ptr);
  la.refit_order = static_cast<uint32_t*>(t.refit_order.ptr);
  la.header = static_cast<uint32_t*>(c->bvh_build_header.ptr);
  la.by_height = c->lbvh_by_height ? 1u : 0u;
  uint32_t header[rt::kLbvhHeaderWords];
  hipError_t e = hipEventRecord(c->build_ev[0], c->stream);
  if (e == hipSuccess)
    e = sah ? rt::launch_sah_build(la, c->bvh_build_scratch.ptr, c->bvh_build_scratch.bytes, c->stream)
            : rt::launch_lbvh_build(la, c->bvh_build_scratch.ptr, c->bvh_build_scratch.bytes, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(header, c->bvh_build_header.ptr, sizeof header, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("device BVH build: ") + hipGetErrorString(e));
  const uint32_t depth = header[0];
  uint32_t counted = 0, levels = 0;
  for (uint32_t h = 0; h < rt::kLbvhMaxLevels; h++) {
    counted += header[2 + h];
    if (header[2 + h]) levels = h + 1;
  }
  if (depth >= static_cast<uint32_t>(rt::kBvhMaxDepth)) {
    *too_deep = true;
    return RTPT_OK;
  }
  if (sah && header[1] >= 1 && header[1] <= n_nodes) n_nodes = header[1];
  if (header[1] != n_nodes || counted != n_nodes || levels != std::max(depth, 1u))
    return fail(RTPT_E_INVALID, "internal: the device BVH build lost nodes");
  t.n_nodes = n_nodes;
  t.refit_level_first.assign(static_cast<size_t>(levels) + 1, 0);
  for (uint32_t h = 0; h < levels; h++) t.refit_level_first[h + 1] = t.refit_level_first[h] + header[2 + h];
  t.bvh_depth = static_cast<int>(depth);
  t.leaf_pairs = leaf_pairs;
  t.device_tree = true;
  std::swap(s.tree, t);
  rt::launch_refit(refit_args(s), s.tree.refit_level_first.data(), static_cast<int>(levels), n_nodes, 1e-5f, c->stream);
  rt::launch_scene_prepare(scene_prep_args(s), c->stream);
  rebuild_light_table(c, s);
  const int rcl = launch_check("device BVH build");
  const hipError_t ee = hipEventRecord(c->build_ev[1], c->stream);
  if (rcl) return rcl;
  HIP_TRY(ee);
  s.build_ms_pending = true;
  set_build_info(s, sah ? static_cast<uint32_t>(RTPT_BUILDER_DEVICE_SAH) : static_cast<uint32_t>(RTPT_BVH_BUILDER_DEVICE_LBVH), RTPT_BVH_FALLBACK_NONE, 0.f);
  return RTPT_OK;
}

// RTPT_FLAG_EXT_NEE: the light list of a material call (light_list_host.hpp), built on the host before anything of the scene is
// touched.  Without the flag the list stays empty and nothing else happens
template <class M>
int host_light_list(const rtpt_ctx* c, const uint32_t* tri_material, const M* materials, std::vector<uint32_t>* list) {
  list->clear();
  if (!(c->cfg.flags & RTPT_FLAG_EXT_NEE)) return RTPT_OK;
  const int r = rtpt_light::build_light_list(tri_material, materials, c->scene.n_base_tris, c->scene.n_instances ? c->scene.n_instances : 1u, list);
  if (r == rtpt_light::kListTooLong) return fail(RTPT_E_INVALID, "more than 2^24 emissive triangles: the light list of RTPT_FLAG_EXT_NEE has no room for them");
  if (r != rtpt_light::kListOk) return fail(RTPT_E_NOMEM, "host allocation failed (light list)");
  return RTPT_OK;
}

// ... to the device, in the manner of the material records: `list` outlives the caller's synchronise, and `ids` is the caller's
// local, which joins the scene together with the records once both copies are complete (join_materials): a failure here or
// there leaves the scene without either.  An empty list allocates and copies nothing
int upload_light_list(rtpt_ctx* c, const std::vector<uint32_t>& list, Buf& ids) {
  if (list.empty()) return RTPT_OK;
  const size_t bytes = list.size() * sizeof(uint32_t);
  int rc = alloc_buf(ids, bytes);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(ids.ptr, list.data(), bytes, hipMemcpyHostToDevice, c->stream));
  return RTPT_OK;
}
// RTPT_FLAG_EXT_NEE_POWER: room for the cumulative table of a list of n_lights entries and for its builder, the caller's local
// like `ids`.  Without both bits, or for an empty list, nothing is allocated
int alloc_light_table(const rtpt_ctx* c, size_t n_lights, Scene::LightTable& tab) {
  const uint32_t both = RTPT_FLAG_EXT_NEE | RTPT_FLAG_EXT_NEE_POWER;
  if ((c->cfg.flags & both) != both || !n_lights) return RTPT_OK;
  int rc;
  if ((rc = alloc_buf(tab.cdf, n_lights * sizeof(uint64_t))) || (rc = alloc_buf(tab.scratch, rt::light_table_scratch_bytes(n_lights)))) return rc;
  return RTPT_OK;
}
// The table of scene s from its light list, shade records and material records as they stand on the stream: behind every
// launch_scene_prepare, and where the list joins the scene.  No synchronisation, no readback; nothing without a table
void rebuild_light_table(rtpt_ctx* c, Scene& s) {
  if (!s.light_table.cdf.ptr || !s.lights.ptr || !s.n_lights || !s.materials.ptr || !s.shade.ptr) return;
  rt::LightTableArgs la;
  la.ids = static_cast<const uint32_t*>(s.lights.ptr);
  la.n = s.n_lights;
  la.shade = static_cast<const float4*>(s.shade.ptr);
  la.materials = static_cast<const float4*>(s.materials.ptr);
  la.n_base_tris = s.n_base_tris;
  la.cdf = static_cast<uint64_t*>(s.light_table.cdf.ptr);
  la.scratch = s.light_table.scratch.ptr;
  rt::launch_light_table(la, c->stream);
}
// The cofactor table of scene s under `model` (shading_normal.hpp: cof_rows), one matrix per instance; nothing without normals.
// on_device: a small kernel on the context's stream from the transforms as they stand there — no upload, no synchronisation.
// Otherwise the same function on the host, into a staging vector the scene owns, and one copy; the caller synchronises.
// The transforms of a scene that has any are on the device (mesh_dev.xf, xf_dev_current), on the host (inst_xf), or both.
int rebuild_normal_cof(rtpt_ctx* c, Scene& s, const float* model, bool on_device) {
  if (!s.normals.records.ptr || !s.normals.cof.ptr) return RTPT_OK;
  const uint32_t ni = s.n_instances ? s.n_instances : 1u;
  const bool on_dev = s.xf_dev_current && s.mesh_dev.xf.ptr, on_host = !s.inst_xf.empty();
  const bool with_xf = on_dev || on_host;
  if (on_host && s.inst_xf.size() != 12 * static_cast<size_t>(ni)) return fail(RTPT_E_INVALID, "internal: the host copy of the instance transforms is missing");
  if (on_device) {
    const float* xf = nullptr;
    if (on_dev) {
      xf = static_cast<const float*>(s.mesh_dev.xf.ptr);
    } else if (on_host) {
      // transforms that never went to the device mesh, or went stale there on the host route: the normals' own copy, which
      // rtpt_scene_set_normals uploaded.  Only where it is stale (a host-route move, then a route that changed) it goes up
      // again, and the stream drains before the pageable source may change
      if (!s.normals.xf_current) {
        int rc;
        if (s.normals.xf.bytes != static_cast<size_t>(ni) * 48 && (rc = alloc_buf(s.normals.xf, static_cast<size_t>(ni) * 48))) return rc;
        HIP_TRY(hipMemcpyAsync(s.normals.xf.ptr, s.inst_xf.data(), s.normals.xf.bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        s.normals.xf_current = true;
      }
      xf = static_cast<const float*>(s.normals.xf.ptr);
    }
    rt::RefitModel rm;
    std::memcpy(rm.m, model, sizeof rm.m);
    rm.identity = is_identity(model) ? 1 : 0;
    rt::launch_normal_cof(ni, xf, rm, static_cast<float4*>(s.normals.cof.ptr), c->stream);
    return RTPT_OK;
  }
  if (with_xf && !on_host) return fail(RTPT_E_INVALID, "internal: the host copy of the instance transforms is missing");
  try {
    s.normals.cof_host.resize(12 * static_cast<size_t>(ni));
  } catch (const std::bad_alloc&) {
    return fail(RTPT_E_NOMEM, "host allocation failed (normal cofactors)");
  }
  for (uint32_t i = 0; i < ni; i++)
    rt::nrm::cof_rows(model, with_xf ? s.inst_xf.data() + 12 * static_cast<size_t>(i) : nullptr, s.normals.cof_host.data() + 12 * static_cast<size_t>(i));
  HIP_TRY(hipMemcpyAsync(s.normals.cof.ptr, s.normals.cof_host.data(), s.normals.cof.bytes, hipMemcpyHostToDevice, c->stream));
  return RTPT_OK;
}
int join_materials(rtpt_ctx* c, Buf& recs, Buf& ids, size_t n_lights, Scene::LightTable& tab) {
  c->scene.materials = std::move(recs);
  if (ids.ptr) {
    c->scene.lights = std::move(ids);
    c->scene.n_lights = static_cast<uint32_t>(n_lights);
    if (tab.cdf.ptr) {
      c->scene.light_table = std::move(tab);
      rebuild_light_table(c, c->scene);
      return launch_check("light table");
    }
  }
  return RTPT_OK;
}

void drop_lights(rtpt_ctx* c) {
  free_buf(c->scene.lights);
  c->scene.n_lights = 0;
  free_buf(c->scene.light_table.cdf);
  free_buf(c->scene.light_table.scratch);
}

// the mesh and the instance transforms of one rtpt_scene_upload call
struct MeshIn {
  const float* xyz;
  uint32_t n_verts;
  const uint32_t* idx;
  uint32_t n_tris;
  const float* xf;  // NULL: one identity instance
  uint32_t ni;      // instances (1 without transforms)
};

// triangle t of instance inst, un-posed: xf[inst] * xyz[idx[3 t + k]].  THE arithmetic of the flattened scene: k_flatten
// (scene_flatten.hip) and oracle_flatten state the same expression, so the three agree bit for bit
inline void flatten_tri(const float* xyz, const uint32_t* idx, const float* xf, uint32_t inst, uint32_t t, float* o) {
  for (int k = 0; k < 3; k++, o += 3) {
    const float* v = xyz + 3 * static_cast<size_t>(idx[3 * static_cast<size_t>(t) + k]);
    if (xf) {
      const float* m = xf + 12 * static_cast<size_t>(inst);
      for (int r = 0; r < 3; r++)
        o[r] = rt::fmaf_(m[4 * r + 2], v[2], rt::fmaf_(m[4 * r + 1], v[1], m[4 * r] * v[0])) + m[4 * r + 3];
    } else {
      o[0] = v[0];
      o[1] = v[1];
      o[2] = v[2];
    }
  }
}

// flattened world-space triangle soup, id = instance * n_tris + t  (one identity instance in the
// reference, main.cpp:728-741)
void host_flatten(const float* xyz, const uint32_t* idx, uint32_t n_tris, const float* xf, uint32_t ni, float* out) {
  for (uint32_t inst = 0; inst < ni; inst++)
    for (uint32_t t = 0; t < n_tris; t++) flatten_tri(xyz, idx, xf, inst, t, out + 9 * (static_cast<size_t>(inst) * n_tris + t));
}

// fan pair (a, b, c), (a, c, d): the posed records are computed from these vertices with one arithmetic, so bitwise
// equality here is bitwise equality of v0 and of e2_A / e1_B on the device, whatever the model matrix
inline bool fan_pair(const float* ta, const float* tb) { return std::memcmp(ta, tb, 12) == 0 && std::memcmp(ta + 6, tb + 3, 12) == 0; }

bool host_fan_pairs(const float* tris, uint32_t total) {
  bool paired_all = total >= 2 && total % 2 == 0;
  for (uint32_t q = 0; paired_all && q < total / 2; q++) paired_all = fan_pair(tris + 18 * static_cast<size_t>(q), tris + 18 * static_cast<size_t>(q) + 9);
  return paired_all;
}

// the mesh and room for its transforms, resident on the device: what k_flatten reads
int alloc_device_mesh(Scene::DeviceMesh& m, size_t n_verts, size_t n_tris, size_t ni) {
  int rc;
  if ((rc = alloc_buf(m.xyz, n_verts * 12)) || (rc = alloc_buf(m.idx, n_tris * 12))) return rc;
  return alloc_buf(m.xf, ni * 48);
}

rt::FlattenArgs flatten_args(const Scene& s, uint32_t n_tris, bool with_xf) {
  rt::FlattenArgs fa;
  fa.n_tris = n_tris;
  fa.n_out_verts = s.n_tris * 3;
  fa.xyz = static_cast<const float*>(s.mesh_dev.xyz.ptr);
  fa.idx = static_cast<const uint32_t*>(s.mesh_dev.idx.ptr);
  fa.xf = with_xf ? static_cast<const float*>(s.mesh_dev.xf.ptr) : nullptr;
  fa.out = static_cast<float*>(s.obj_tris_dev.ptr);
  return fa;
}

// The three routes of rtpt_scene_upload; each assembles `s` (triangles, records, tree) on the device.  Host tree: the
// flattened triangles and a tree built on the host go up; all that can refuse the call comes before begin_scene.
int upload_host_tree(rtpt_ctx* c, Scene& s, const std::vector<float>& tris, bool leaf_pairs, uint32_t fallback) {
  const uint32_t total = static_cast<uint32_t>(tris.size() / 9);
  const double t_build = now_ms();
  rt::Bvh bvh;
  rt::build_bvh(tris.data(), total, bvh, 1e-5f, leaf_pairs);
  if (bvh.max_depth >= rt::kBvhMaxDepth) return fail(RTPT_E_INVALID, "BVH deeper than the traversal stack");
  int rc;
  if ((rc = check_record_offsets(total, bvh.nodes.size()))) return rc;
  if (bvh.leaf_order.size() != total) return fail(RTPT_E_INVALID, "internal: BVH lost triangles");
  if (leaf_pairs)  // the pairs-mode leaf test reads one pair record per leaf: a leaf of any other shape would be misread
    for (const rt::BvhNode& nd : bvh.nodes)
      for (int side = 0; side < 2; side++) {
        const uint32_t idx = side ? nd.ridx : nd.lidx, cnt = side ? nd.rcnt : nd.lcnt;
        if (idx != rt::kBvhEmpty && cnt && !rt::pair_leaf_ok(idx, cnt, bvh.leaf_order.data(), total))
          return fail(RTPT_E_INVALID, "internal: a pairs-mode BVH leaf is not one fan pair (2q, 2q + 1) from an even slot");
      }
  std::vector<rt::BvhNodeQ> nodes_h;
  const rt::BvhGrid grid = rt::pack_quantised_nodes(bvh, nodes_h);
  const double build_ms = now_ms() - t_build;
  std::vector<uint32_t> order_h, level_first;
  nodes_by_height(nodes_h, order_h, level_first);
  if ((rc = begin_scene(c, s, total)) || (rc = alloc_tree(s.tree, nodes_h.size(), total))) return rc;
  s.tree.bvh_grid = grid;
  s.tree.n_nodes = static_cast<uint32_t>(nodes_h.size());
  s.tree.refit_level_first.swap(level_first);
  s.tree.leaf_pairs = leaf_pairs;
  s.tree.bvh_depth = bvh.max_depth;
  if ((rc = upload_tris(c, s, tris))) return rc;
  HIP_TRY(hipMemcpyAsync(s.tree.leaf_order.ptr, bvh.leaf_order.data(), static_cast<size_t>(total) * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(s.tree.nodes.ptr, nodes_h.data(), nodes_h.size() * sizeof(rt::BvhNodeQ), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(s.tree.refit_order.ptr, order_h.data(), order_h.size() * 4, hipMemcpyHostToDevice, c->stream));
  float grid_h[8];
  if ((rc = upload_grid(c, s, grid_h))) return rc;
  rt::launch_scene_prepare(scene_prep_args(s), c->stream);
  rebuild_light_table(c, s);
  if ((rc = launch_check("scene_prepare"))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // host staging vectors die at return
  s.tree.bvh_host = std::move(bvh);
  set_build_info(s, RTPT_BVH_BUILDER_HOST_SAH, fallback, static_cast<float>(build_ms));
  return RTPT_OK;
}

// Device tree (RTPT_FLAG_DEVICE_BVH_BUILD): the flattened triangles go up, the tree is built there
int upload_device_tree(rtpt_ctx* c, Scene& s, const std::vector<float>& tris, bool leaf_pairs, bool* too_deep) {
  int rc;
  if ((rc = begin_scene(c, s, static_cast<uint32_t>(tris.size() / 9)))) return rc;
  if ((rc = upload_tris(c, s, tris))) return rc;
  // the builder's readback synchronises behind these copies, so the staging vector may die at return
  return device_build_tree(c, s, leaf_pairs, too_deep);
}

// Device flatten (RTPT_FLAG_DEVICE_FLATTEN too): only the mesh and the transforms go up; triangles and the fan-pair
// decision (*paired_all) are made there (scene_flatten.hip), one word comes back before the build because the primitive
// width depends on it
int upload_device_flatten(rtpt_ctx* c, Scene& s, const MeshIn& in, uint32_t total, bool* paired_all, bool* too_deep) {
  int rc;
  if (!c->pair_word.ptr && (rc = alloc_buf(c->pair_word, 4))) return rc;
  if ((rc = begin_scene(c, s, total)) || (rc = alloc_device_mesh(s.mesh_dev, in.n_verts, in.n_tris, in.ni))) return rc;
  HIP_TRY(hipMemcpyAsync(s.mesh_dev.xyz.ptr, in.xyz, static_cast<size_t>(in.n_verts) * 12, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(s.mesh_dev.idx.ptr, in.idx, static_cast<size_t>(in.n_tris) * 12, hipMemcpyHostToDevice, c->stream));
  if (in.xf) HIP_TRY(hipMemcpyAsync(s.mesh_dev.xf.ptr, in.xf, static_cast<size_t>(in.ni) * 48, hipMemcpyHostToDevice, c->stream));
  c->upload_info[0] += static_cast<uint64_t>(in.n_verts) * 12 + static_cast<uint64_t>(in.n_tris) * 12 + (in.xf ? static_cast<uint64_t>(in.ni) * 48 : 0);
  rt::launch_flatten(flatten_args(s, in.n_tris, in.xf != nullptr), c->stream);
  const bool even = total >= 2 && total % 2 == 0;
  uint32_t word = 0;
  if (even) {
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->pair_word.ptr), 1, 1, c->stream));
    rt::launch_fan_pairs(total / 2, static_cast<const float*>(s.obj_tris_dev.ptr), static_cast<uint32_t*>(c->pair_word.ptr), c->stream);
    HIP_TRY(hipMemcpyAsync(&word, c->pair_word.ptr, 4, hipMemcpyDeviceToHost, c->stream));
  }
  rt::RefitModel rm{};  // a fresh upload stands under the identity model: tris = obj_tris_dev
  rm.identity = 1;
  rt::launch_pose(total * 3, static_cast<const float*>(s.obj_tris_dev.ptr), static_cast<float*>(s.tris.ptr), rm, c->stream);
  if ((rc = launch_check("device flatten"))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // the pair word; the caller's arrays may die at return
  *paired_all = even && word == 1u;
  return device_build_tree(c, s, *paired_all && !c->no_pairing, too_deep);
}

// what is left to say about `s` once its triangles, records and tree stand on the device (any route); `tris` may be empty
// when the triangles were flattened on the device (then nothing on the host reads them).  Model, LUT versions and
// materials are a new scene's defaults
int finish_scene(const rtpt_ctx* c, Scene& s, const MeshIn& in, std::vector<float>& tris, bool paired_all) {
  const bool small = s.n_tris <= static_cast<uint32_t>(rt::kCullMaxTris);
  s.n_instances = in.ni;
  s.has_xf = in.xf != nullptr;
  s.n_base_tris = in.n_tris;
  s.tris_paired = paired_all && small;  // the brute-force loops
  s.use_bvh = (s.n_tris > 64) || (c->cfg.flags & RTPT_FLAG_FORCE_BVH);
  try {
    s.mesh_xyz.assign(in.xyz, in.xyz + 3 * static_cast<size_t>(in.n_verts));
    s.mesh_idx.assign(in.idx, in.idx + 3 * static_cast<size_t>(in.n_tris));
    if (small) s.host_tris = tris;
    // the transforms, where the device mesh does not hold them (a device-flatten upload copied them there): nothing else does,
    // and the cofactor table of rtpt_scene_set_normals is built from them
    if (in.xf && !s.mesh_dev.xf.ptr) s.inst_xf.assign(in.xf, in.xf + 12 * static_cast<size_t>(in.ni));
  } catch (const std::bad_alloc&) {
    return fail(RTPT_E_NOMEM, "host allocation failed (mesh copy)");
  }
  // elsewhere the scene is posed on the device from obj_tris_dev: the host copy is never read
  if (small || !refits_on_device(c, s)) s.obj_tris.swap(tris);
  return RTPT_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------ scene

// validate, choose the route, run it (a device tree deeper than the traversal stack: the host route, flatten included, in
// the same call — the host builder bounds its depth), commit
int rtpt_scene_upload(rtpt_ctx* c, const float* xyz, uint32_t n_verts, const uint32_t* idx, uint32_t n_tris,
                      const float* xf, uint32_t n_instances) {
  if (!c || !xyz || !idx) return fail(RTPT_E_INVALID, "NULL argument");
  if (n_tris == 0 || n_verts == 0) return fail(RTPT_E_INVALID, "empty mesh");
  for (uint32_t i = 0; i < 3 * n_tris; i++)
    if (idx[i] >= n_verts) return fail(RTPT_E_INVALID, "index out of range");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  const double t_call = now_ms();
  if (!(xf && n_instances)) xf = nullptr;
  const uint32_t ni = xf ? n_instances : 1;
  const uint64_t total64 = static_cast<uint64_t>(ni) * n_tris;
  if (total64 >= 0xFFFFFFF0ull) return fail(RTPT_E_INVALID, "too many triangles");
  int rc;
  if ((rc = check_record_offsets(total64, 0))) return rc;
  const uint32_t total = static_cast<uint32_t>(total64);
  const MeshIn in{xyz, n_verts, idx, n_tris, xf, ni};
  c->upload_info[0] = c->upload_info[1] = c->upload_info[2] = 0;
  Scene s;  // assembled here, moved into the context when it is complete
  std::vector<float> tris;  // flattened on the host, unless the device does it
  bool paired_all = false, too_deep = false;
  const bool flatten_there = c->device_bvh && c->device_flatten && total > static_cast<uint32_t>(rt::kCullMaxTris);
  if (flatten_there && (rc = upload_device_flatten(c, s, in, total, &paired_all, &too_deep))) return rc;
  if (!flatten_there || too_deep) {
    tris.resize(static_cast<size_t>(total) * 9);
    host_flatten(xyz, idx, n_tris, xf, ni, tris.data());
    paired_all = host_fan_pairs(tris.data(), total);
    const bool leaf_pairs = paired_all && !c->no_pairing;
    if (c->device_bvh && !too_deep && (rc = upload_device_tree(c, s, tris, leaf_pairs, &too_deep))) return rc;
    if (!c->device_bvh || too_deep)
      if ((rc = upload_host_tree(c, s, tris, leaf_pairs, too_deep ? RTPT_BVH_FALLBACK_DEPTH : RTPT_BVH_FALLBACK_NONE))) return rc;
  }
  if ((rc = finish_scene(c, s, in, tris, paired_all))) return rc;
  s.xf_dev_current = xf && s.mesh_dev.xf.ptr;  // (a device-flatten upload copied them there)
  if (flatten_there && !too_deep) c->upload_info[1] = c->upload_info[2] = 1;
  s.build_info.upload_ms = static_cast<float>(now_ms() - t_call);
  c->scene = std::move(s);
  return RTPT_OK;
}

}  // extern "C"

namespace {

// Pose the scene (visibility.vert.glsl:24 `model * position`; the reference recomputes ubo.model every frame,
// main.cpp:1469, as the identity).  The posed scene follows its inputs: the un-posed triangles (obj_tris_dev / obj_tris —
// they change with rtpt_scene_set_instances) and the model (it changes with ubo.model, rtpt_gbuffer).  Whichever of the
// two changed, this is the one routine that re-poses, REFITS the tree (it keeps its topology) and rebuilds the records, so
// that every pass — K0, K2, the LUT — sees the posed geometry, and marks LUT, tables and frame reuse stale.
int repose_scene(rtpt_ctx* c, const float* model) {
  Scene& s = c->scene;
  const uint32_t total = s.n_tris;
  const bool small = total <= static_cast<uint32_t>(rt::kCullMaxTris), on_device = refits_on_device(c, s);
  if ((small || !on_device) && s.obj_tris.size() != static_cast<size_t>(total) * 9)
    return fail(RTPT_E_INVALID, "internal: the host copy of the un-posed triangles is missing");
  // the posed triangles where the host reads them: the screen bounds of a small scene (unused while it is forced onto the
  // BVH path, but they still follow the pose) and the host refit
  std::vector<float> posed;
  if (small || !on_device) host_pose(model, s.obj_tris, posed);
  int rc;
  if (on_device) {
    // everything on the device and on the context's stream: no upload, no synchronisation (refit.hip)
    rt::RefitModel rm;
    std::memcpy(rm.m, model, sizeof rm.m);
    rm.identity = is_identity(model) ? 1 : 0;
    rt::launch_pose(total * 3, static_cast<const float*>(s.obj_tris_dev.ptr), static_cast<float*>(s.tris.ptr), rm, c->stream);
    rt::launch_refit(refit_args(s), s.tree.refit_level_first.data(), static_cast<int>(s.tree.refit_level_first.size()) - 1, s.tree.n_nodes, 1e-5f, c->stream);
    rt::launch_scene_prepare(scene_prep_args(s), c->stream);
    rebuild_light_table(c, s);
    if ((rc = rebuild_normal_cof(c, s, model, true))) return rc;
    if ((rc = launch_check("device refit"))) return rc;
  } else {
    rt::refit_bvh(posed.data(), total, s.tree.bvh_host);
    std::vector<rt::BvhNodeQ> nodes_h;
    s.tree.bvh_grid = rt::pack_quantised_nodes(s.tree.bvh_host, nodes_h);
    if (nodes_h.size() * sizeof(rt::BvhNodeQ) != s.tree.nodes.bytes) return fail(RTPT_E_INVALID, "internal: refit changed the node count");
    HIP_TRY(hipMemcpyAsync(s.tris.ptr, posed.data(), posed.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(s.tree.nodes.ptr, nodes_h.data(), nodes_h.size() * sizeof(rt::BvhNodeQ), hipMemcpyHostToDevice, c->stream));
    float grid_h[8];
  if ((rc = upload_grid(c, s, grid_h))) return rc;
    rt::launch_scene_prepare(scene_prep_args(s), c->stream);
    rebuild_light_table(c, s);
    if ((rc = rebuild_normal_cof(c, s, model, false))) return rc;
    if ((rc = launch_check("scene_prepare"))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // host staging vectors die at return
  }
  if (small) s.host_tris.swap(posed);
  mark_reposed(c, model);
  return RTPT_OK;
}

// the transforms of one rtpt_scene_set_instances call, to xf_dev through pinned memory: a copy the stream runs in order,
// that neither waits for the stream nor reads the caller's array after the call.  Two staging buffers in turn; the event
// waited for belongs to the call before last (long finished unless the host runs two whole frames ahead)
int stage_transforms(rtpt_ctx* c, const float* xf, size_t bytes) {
  rtpt_ctx::XfStage& st = c->xf_stage[c->xf_stage_cur];
  if (!st.done) HIP_TRY(hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
  if (st.pending) {
    HIP_TRY(hipEventSynchronize(st.done));
    st.pending = false;
  }
  if (st.bytes < bytes) {
    if (st.host) (void)hipHostFree(st.host);
    st.host = nullptr;
    st.bytes = 0;
    if (hipHostMalloc(&st.host, bytes, hipHostMallocDefault) != hipSuccess) return fail(RTPT_E_NOMEM, "pinned host allocation failed");
    st.bytes = bytes;
  }
  std::memcpy(st.host, xf, bytes);
  HIP_TRY(hipMemcpyAsync(c->scene.mesh_dev.xf.ptr, st.host, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(st.done, c->stream));
  st.pending = true;
  c->xf_stage_cur ^= 1;
  return RTPT_OK;
}

}  // namespace

// ubo.model changed (main.cpp:1469 recomputes it every frame; an animated scene passes another one): re-pose the scene
int rtpt_impl::apply_model(rtpt_ctx* c, const float* model) { return repose_scene(c, model); }

extern "C" {

int rtpt_scene_set_instances(rtpt_ctx* c, const float* xf, uint32_t n_instances) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  if (!xf) return fail(RTPT_E_INVALID, "NULL argument");
  if (n_instances != c->scene.n_instances)
    return fail(RTPT_E_INVALID, "the instance count is the upload's (1 for a scene uploaded without transforms): upload again to change it");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  Scene& s = c->scene;
  const uint32_t total = s.n_tris, nt = s.n_base_tris, ni = n_instances;
  const float* mx = s.mesh_xyz.data();
  const uint32_t* mi = s.mesh_idx.data();
  // A refit keeps the topology, pairs included.  A pair inside one instance stays a pair (the same vertices through the
  // same transform and arithmetic); one that straddles two instances (odd triangle count) was a pair by coincidence
  if ((s.tree.leaf_pairs || s.tris_paired) && (nt & 1u))
    for (uint32_t b = 0; b + 1 < ni; b++) {
      if ((static_cast<uint64_t>(b + 1) * nt - 1) & 1u) continue;  // the last triangle of instance b has an odd id: it ends a pair
      float ta[9], tb[9];
      flatten_tri(mx, mi, xf, b, nt - 1, ta);
      flatten_tri(mx, mi, xf, b + 1, 0, tb);
      if (!fan_pair(ta, tb))
        return fail(RTPT_E_INVALID, "these transforms separate a fan pair that straddles two instances: upload the scene again");
    }
  const bool small = total <= static_cast<uint32_t>(rt::kCullMaxTris);
  const bool on_device = refits_on_device(c, s);
  std::vector<float> obj;  // the host's un-posed triangles, where the host reads them (as finish_scene keeps them)
  bool paired = s.tris_paired;
  if (small || !on_device) {
    obj.resize(static_cast<size_t>(total) * 9);
    host_flatten(mx, mi, nt, xf, ni, obj.data());
    paired = host_fan_pairs(obj.data(), total) && small;  // the brute-force loops
  }
  uint64_t bytes = 0;
  if (on_device) {
    int rc;
    if (!s.mesh_dev.xyz.ptr) {  // first move of a scene that was flattened on the host: the mesh goes up, once
      Scene::DeviceMesh m;  // joins the scene when it is complete
      if ((rc = alloc_device_mesh(m, s.mesh_xyz.size() / 3, nt, ni))) return rc;
      HIP_TRY(hipMemcpyAsync(m.xyz.ptr, mx, s.mesh_xyz.size() * 4, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemcpyAsync(m.idx.ptr, mi, s.mesh_idx.size() * 4, hipMemcpyHostToDevice, c->stream));
      s.mesh_dev = std::move(m);
      bytes += s.mesh_xyz.size() * 4 + s.mesh_idx.size() * 4;
    }
    if ((rc = stage_transforms(c, xf, static_cast<size_t>(ni) * 48))) return rc;
    bytes += static_cast<uint64_t>(ni) * 48;
    rt::launch_flatten(flatten_args(s, nt, true), c->stream);
  } else {
    bytes = static_cast<uint64_t>(total) * 36;  // the posed triangles, copied by the host path below
  }
  if (small || !on_device) s.obj_tris.swap(obj);
  if (!on_device && s.obj_tris_dev.ptr) {
    // the device's un-posed triangles follow too: rtpt_scene_rebuild can move this scene onto the device-refit path later
    // (s.obj_tris outlives the copy; the host path below synchronises anyway)
    const hipError_t e = hipMemcpyAsync(s.obj_tris_dev.ptr, s.obj_tris.data(), static_cast<size_t>(total) * 36, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
      s.obj_tris.swap(obj);
      return fail(RTPT_E_DEVICE, std::string("un-posed triangle copy: ") + hipGetErrorString(e));
    }
    bytes += static_cast<uint64_t>(total) * 36;
  }
  const bool paired_before = s.tris_paired;
  s.tris_paired = paired;
  // The transforms the cofactor table of smooth shading is built from (repose_scene: rebuild_normal_cof).  On the device route
  // they are in the device mesh (stage_transforms above) and a scene without normals keeps no host copy: the call allocates what
  // it allocated before there were normals.  The host route, which flattens into a vector of its own anyway, and a scene that
  // holds normals keep one.
  std::vector<float> xf_before;  // the new copy until the swap, the replaced one after it
  if (!on_device || s.normals.records.ptr) {
    try {
      xf_before.assign(xf, xf + 12 * static_cast<size_t>(ni));
    } catch (const std::bad_alloc&) {
      if (!on_device) s.obj_tris.swap(obj);
      s.tris_paired = paired_before;
      return fail(RTPT_E_NOMEM, "host allocation failed (instance transforms)");
    }
  }
  s.inst_xf.swap(xf_before);
  const bool xf_dev_before = s.xf_dev_current, nxf_before = s.normals.xf_current;
  s.xf_dev_current = on_device;
  s.normals.xf_current = false;  // (of the normals' own device copy, which is read only while the device mesh is stale)
  const int rc = repose_scene(c, s.model);
  if (rc) {
    if (!on_device) {  // nothing reached the device: the scene is the one before the call
      s.obj_tris.swap(obj);
      s.tris_paired = paired_before;
      s.inst_xf.swap(xf_before);
      s.xf_dev_current = xf_dev_before;
      s.normals.xf_current = nxf_before;
    }
    return rc;
  }
  s.has_xf = true;
  c->upload_info[0] = bytes;
  c->upload_info[1] = on_device ? 1 : 0;
  c->upload_info[2] = 0;  // the pair decision is the upload's: topology is kept
  if (on_device) c->upload_info[3]++;
  return RTPT_OK;
}

int rtpt_scene_build_info(rtpt_ctx* c, struct rtpt_scene_build_info* out) {
  if (!c || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  if (c->scene.build_ms_pending) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->build_ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->build_ev[0], c->build_ev[1]));
    c->scene.build_info.build_ms = ms;
    c->scene.build_ms_pending = false;
  }
  *out = c->scene.build_info;
  return RTPT_OK;
}

int rtpt_scene_rebuild(rtpt_ctx* c) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!c->scene.n_tris || !c->scene.tree.nodes.ptr) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  const double t_call = now_ms();
  HIP_TRY(hipStreamSynchronize(c->stream));  // the tree's buffers are replaced
  forget_scene(c);  // first: also a build that fails after the swap has replaced the tree
  bool too_deep = false;
  const int rc = device_build_tree(c, c->scene, c->scene.tree.leaf_pairs, &too_deep);
  if (rc) return rc;
  if (too_deep) return fail(RTPT_E_INVALID, "the rebuilt BVH would be deeper than the traversal stack: the tree was kept");
  c->scene.build_info.upload_ms = static_cast<float>(now_ms() - t_call);
  return RTPT_OK;
}

int rtpt_scene_set_materials(rtpt_ctx* c, const uint32_t* tri_material, uint32_t n_tris, const rtpt_material* materials,
                             uint32_t n_materials) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!tri_material || !materials || !n_materials) {  // back to the reference's normal-keyed colours
    free_buf(c->scene.materials);
    c->scene.materials_specular = false;
    drop_lights(c);
    return RTPT_OK;
  }
  if (n_tris != c->scene.n_base_tris) return fail(RTPT_E_INVALID, "one material index per triangle of the uploaded mesh");
  std::vector<float> rec(static_cast<size_t>(n_tris) * 8);
  for (uint32_t t = 0; t < n_tris; t++) {
    if (tri_material[t] >= n_materials) return fail(RTPT_E_INVALID, "material index out of range");
    const rtpt_material& m = materials[tri_material[t]];
    float* r = rec.data() + 8 * static_cast<size_t>(t);
    r[0] = m.albedo[0]; r[1] = m.albedo[1]; r[2] = m.albedo[2]; r[3] = 0.0f;
    r[4] = m.emission[0]; r[5] = m.emission[1]; r[6] = m.emission[2];
    r[7] = (m.emission[0] != 0.0f || m.emission[1] != 0.0f || m.emission[2] != 0.0f) ? 1.0f : 0.0f;
  }
  std::vector<uint32_t> lights;  // RTPT_FLAG_EXT_NEE (empty without): refused, like everything above, before anything is freed
  int rc = host_light_list(c, tri_material, materials, &lights);
  if (rc) return rc;
  free_buf(c->scene.materials);  // never two sets at once; a failure below leaves the reference's colours
  c->scene.materials_specular = false;  // (a set of rtpt_scene_set_materials_ext is replaced like any other)
  drop_lights(c);
  Buf recs, ids;  // join the scene when both are complete
  rc = alloc_buf(recs, rec.size() * sizeof(float));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(recs.ptr, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if ((rc = upload_light_list(c, lights, ids))) return rc;
  Scene::LightTable tab;  // RTPT_FLAG_EXT_NEE_POWER (empty without)
  if ((rc = alloc_light_table(c, lights.size(), tab))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return join_materials(c, recs, ids, lights.size(), tab);
}

int rtpt_scene_set_materials_ext(rtpt_ctx* c, const uint32_t* tri_material, uint32_t n_tris, const rtpt_material_ext* materials,
                                 uint32_t n_materials) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  const bool drop = !tri_material || !materials || !n_materials;
  // everything that can refuse the call comes first: a refused call leaves the scene, and the set it has, untouched
  if (!drop)
    if (const char* why = rtpt_mat::check_materials(tri_material, n_tris, c->scene.n_base_tris, materials, n_materials))
      return fail(RTPT_E_INVALID, why);
  std::vector<float> rec;
  int any_specular = 0;  // rtpt_mat::kMode*
  if (!drop) {
    try {
      rec.resize(static_cast<size_t>(n_tris) * 8);
    } catch (const std::bad_alloc&) {
      return fail(RTPT_E_NOMEM, "host allocation failed (material records)");
    }
    any_specular = rtpt_mat::pack_records_mode(tri_material, n_tris, materials, rec.data());
  }
  std::vector<uint32_t> lights;  // RTPT_FLAG_EXT_NEE (empty without, and for a dropped set)
  if (!drop)
    if (int rcl = host_light_list(c, tri_material, materials, &lights)) return rcl;
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));  // launches that read the set being replaced
  // K0, K1 and the filter read no material: no plane tag, no scene generation changes — frame reuse goes on
  free_buf(c->scene.materials);  // never two sets at once, as in rtpt_scene_set_materials
  c->scene.materials_specular = false;
  drop_lights(c);
  if (drop) return RTPT_OK;
  Buf recs, ids;  // join the scene when both are complete
  int rc = alloc_buf(recs, rec.size() * sizeof(float));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(recs.ptr, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if ((rc = upload_light_list(c, lights, ids))) return rc;
  Scene::LightTable tab;  // RTPT_FLAG_EXT_NEE_POWER (empty without)
  if ((rc = alloc_light_table(c, lights.size(), tab))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  rc = join_materials(c, recs, ids, lights.size(), tab);
  c->scene.materials_specular = any_specular;
  return rc;
}

int rtpt_scene_set_normals(rtpt_ctx* c, const float* tri_normals, const uint32_t* tri_smooth, uint32_t n_tris) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  const bool drop = !tri_normals && n_tris == 0;
  // everything that can refuse the call comes first: a refused call leaves the scene, and the normals it has, untouched
  if (!drop)
    if (const char* why = rtpt_nrm::check_normals(tri_normals, n_tris, c->scene.n_base_tris, c->cfg.flags)) return fail(RTPT_E_INVALID, why);
  std::vector<float> rec;
  if (!drop) {
    try {
      rec.resize(static_cast<size_t>(n_tris) * rtpt_nrm::kRecordFloats);
    } catch (const std::bad_alloc&) {
      return fail(RTPT_E_NOMEM, "host allocation failed (normal records)");
    }
    rtpt_nrm::pack_records(tri_normals, tri_smooth, n_tris, rec.data());
  }
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));  // launches that read the set being replaced
  Scene& s = c->scene;
  if (c->cfg.flags & RTPT_FLAG_EXT_SMOOTH_GUIDE) {
    // the guide normals K0 wrote belong to the set being replaced: the next frame runs K0 again, and until then a filter call
    // takes the triangles' normals (the stale plane)
    reuse_invalidate(c, &c->normals);
    c->frame.normals = Rows();
  }
  const bool bvh_without = (s.n_tris > 64) || (c->cfg.flags & RTPT_FLAG_FORCE_BVH);  // finish_scene's choice
  if (drop) {
    s.normals = Scene::Normals{};
    if ((c->cfg.flags & RTPT_FLAG_EXT_SMOOTH_GUIDE) && s.pair_tab.ptr) free_buf(c->normals);  // (the scene's filter reads its id-pair table again)
    if (s.use_bvh != bvh_without) {
      s.use_bvh = bvh_without;
      c->scene_gen++;  // brute force may resolve a tie between equally near triangles differently
    }
    return RTPT_OK;
  }
  Scene::Normals nn;  // joins the scene when it is complete; the set it replaces stays until then
  const uint32_t ni = s.n_instances ? s.n_instances : 1u;
  // the normals' own device copy of the transforms, only where the device mesh does not hold them
  const bool with_xf = !(s.xf_dev_current && s.mesh_dev.xf.ptr) && !s.inst_xf.empty();
  int rc;
  if ((rc = alloc_buf(nn.records, rec.size() * sizeof(float))) || (rc = alloc_buf(nn.cof, static_cast<size_t>(ni) * 48))) return rc;
  if (with_xf && (rc = alloc_buf(nn.xf, static_cast<size_t>(ni) * 48))) return rc;
  HIP_TRY(hipMemcpyAsync(nn.records.ptr, rec.data(), nn.records.bytes, hipMemcpyHostToDevice, c->stream));
  if (with_xf) HIP_TRY(hipMemcpyAsync(nn.xf.ptr, s.inst_xf.data(), nn.xf.bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's arrays and `rec` may die at return
  nn.xf_current = with_xf;
  std::swap(s.normals, nn);
  const bool bvh_before = s.use_bvh;
  s.use_bvh = true;  // (refits_on_device reads it: the table below is built by the route the next re-pose takes)
  if ((rc = rebuild_normal_cof(c, s, s.model, refits_on_device(c, s))) || (rc = launch_check("normal cofactors"))) {
    std::swap(s.normals, nn);  // the scene is the one before the call
    s.use_bvh = bvh_before;
    return rc;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!bvh_before) c->scene_gen++;  // the tree may resolve a tie between equally near triangles differently
  return RTPT_OK;
}

int rtpt_scene_set_textures(rtpt_ctx* c, const float* tri_uv, const uint32_t* tri_texture, uint32_t n_tris, const rtpt_texture* textures,
                            uint32_t n_textures, const float* texels, size_t n_texels) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  const bool drop = !tri_uv || !tri_texture || !textures || !texels || !n_textures || !n_texels;
  // everything that can refuse the call comes first: a refused call leaves the scene, and the textures it has, untouched
  if (!drop)
    if (const char* why = rtpt_tex::check_textures(tri_uv, tri_texture, n_tris, c->scene.n_base_tris, textures, n_textures, n_texels))
      return fail(RTPT_E_INVALID, why);
  std::vector<float> rec;
  std::vector<uint32_t> levels;  // the level table, when some texture has RTPT_TEX_MIPMAP
  size_t generated = 0;          // texels of the levels built here, appended to the atlas
  if (!drop) {
    try {
      rec.resize(static_cast<size_t>(n_tris) * 8);
      if (rtpt_tex::any_mipmap(textures, n_textures)) levels.resize(static_cast<size_t>(n_textures) * rtpt_tex::kLevelRow);
    } catch (const std::bad_alloc&) {
      return fail(RTPT_E_NOMEM, "host allocation failed (texture records)");
    }
    rtpt_tex::pack_records(tri_uv, tri_texture, n_tris, rec.data());
    if (!levels.empty()) {
      rtpt_tex::build_level_table(textures, n_textures, n_texels, levels.data());
      generated = static_cast<size_t>(rtpt_tex::generated_texels(textures, n_textures));  // check_textures: the atlas stays below 2^32
    }
  }
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));  // launches that read the set being replaced
  // K0, K1 and the filter read no texture: no plane tag, no scene generation changes — frame reuse goes on
  if (drop) {
    c->scene.textures = Scene::Textures{};
    return RTPT_OK;
  }
  static_assert(sizeof(rtpt_texture) == sizeof(rt::TexDesc), "the descriptors are copied as they are");
  Scene::Textures t;  // joins the scene when it is complete; the set it replaces stays until then
  int rc;
  if ((rc = alloc_buf(t.records, rec.size() * sizeof(float))) || (rc = alloc_buf(t.desc, static_cast<size_t>(n_textures) * sizeof(rtpt_texture))) ||
      (rc = alloc_buf(t.texels, (n_texels + generated) * 16)) || (!levels.empty() && (rc = alloc_buf(t.levels, levels.size() * sizeof(uint32_t)))))
    return rc;
  HIP_TRY(hipMemcpyAsync(t.records.ptr, rec.data(), t.records.bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t.desc.ptr, textures, t.desc.bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(t.texels.ptr, texels, n_texels * 16, hipMemcpyHostToDevice, c->stream));
  if (!levels.empty()) {
    HIP_TRY(hipMemcpyAsync(t.levels.ptr, levels.data(), t.levels.bytes, hipMemcpyHostToDevice, c->stream));
    // the generated chains: level l + 1 from level l, one launch each, at the offsets of the table
    for (uint32_t i = 0; i < n_textures; i++) {
      if (!rtpt_tex::generates_chain(textures[i])) continue;
      const uint32_t* row = levels.data() + static_cast<size_t>(rtpt_tex::kLevelRow) * i;
      for (uint32_t l = 0; l + 1 < row[rtpt_tex::kLevelRowCount]; l++)
        rt::launch_mip_downsample(static_cast<float4*>(t.texels.ptr), row[l], rtpt_tex::level_dim(textures[i].width, l),
                                  rtpt_tex::level_dim(textures[i].height, l), row[l + 1], c->stream);
    }
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(c->stream));  // the caller's arrays and `rec` may die at return
  t.n_textures = n_textures;
  c->scene.textures = std::move(t);
  return RTPT_OK;
}

}  // extern "C"
