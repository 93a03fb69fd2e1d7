// api_scene.hip — the scene side of the C ABI: rtpt_scene_upload (loadMesh + buildAccelerationStructure, main.cpp:409-462,
// :687-742; flattened on the host, or on the device: scene_flatten.hip), instances that move between frames
// (rtpt_scene_set_instances), the posed scene of a changed ubo.model (device-side refit, refit.hip), materials.
#include "api_internal.hpp"

#include <chrono>

namespace {

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

rt::ScenePrepArgs scene_prep_args(const rtpt_ctx* c, uint32_t total, bool leaf_pairs) {
  rt::ScenePrepArgs sp;
  sp.n_tris = total;
  sp.tris = static_cast<const float*>(c->tris.ptr);
  sp.leaf_order = static_cast<const uint32_t*>(c->leaf_order.ptr);
  sp.isect_id = static_cast<float4*>(c->isect_id.ptr);
  sp.isect_leaf = static_cast<float4*>(c->isect_leaf.ptr);
  sp.shade = static_cast<float4*>(c->shade.ptr);
  sp.leaf_pairs = leaf_pairs ? 1u : 0u;
  return sp;
}

rt::RefitArgs refit_args(const rtpt_ctx* c) {
  rt::RefitArgs ra;
  ra.tris = static_cast<const float*>(c->tris.ptr);
  ra.leaf_order = static_cast<const uint32_t*>(c->leaf_order.ptr);
  ra.order = static_cast<const uint32_t*>(c->refit_order.ptr);
  ra.nodes = static_cast<rt::BvhNodeQ*>(c->nodes.ptr);
  ra.fbox = static_cast<float*>(c->refit_fbox.ptr);
  ra.grid = static_cast<float*>(c->bvh_grid_dev.ptr);
  return ra;
}

// The tree over c->tris (`total` triangles as they stand on the device) built on the device (bvh_build.hip, or
// bvh_build_sah.hip with c->device_bvh_sah: fewer nodes than primitives - 1 where a leaf holds two triangles) and swapped
// into the context: nodes, leaf order, nodes by height, depth; then the refit that fills boxes and grid and the leaf
// records.  Built aside, so a tree deeper than the traversal stack (*too_deep, RTPT_OK) or an error leaves the context's
// tree as it was.  The stream must be idle on entry (buffers are replaced).  The LBVH synchronises ONCE, for the
// readback of kLbvhHeaderWords dwords; the SAH build also synchronises inside launch_sah_build, once at its start and one to
// three times per level of the tree (its segment counts come back to the host).  Needs c->tris, c->isect_*, c->shade and c->bvh_grid_dev allocated for `total`.
int device_build_tree(rtpt_ctx* c, uint32_t total, bool leaf_pairs, bool* too_deep) {
  *too_deep = false;
  const bool sah = c->device_bvh_sah;
  const uint32_t w = leaf_pairs ? 2u : 1u, n_prims = total / w;
  uint32_t n_nodes = n_prims > 1 ? n_prims - 1 : 1;  // the SAH builder may write fewer: its header says how many
  // the traversal addresses leaf records and nodes as base + 32-bit byte offset (48 bytes per triangle at most, 32 per node)
  if (static_cast<uint64_t>(total) * 48u >= (1ull << 32) || n_nodes >= (1u << 27))
    return fail(RTPT_E_INVALID, "scene too large for the traversal's 32-bit record offsets (more than 89,478,485 triangles)");
  const size_t need = sah ? rt::sah_scratch_bytes(n_prims) : rt::lbvh_scratch_bytes(n_prims, c->lbvh_by_height);
  if (!need) return fail(RTPT_E_DEVICE, "device BVH build: the sort's temporary-storage query failed");
  int rc;
  if (c->bvh_build_scratch.bytes < need && (rc = alloc_buf(c->bvh_build_scratch, need))) return rc;
  if (!c->bvh_build_header.ptr && (rc = alloc_buf(c->bvh_build_header, rt::kLbvhHeaderWords * 4))) return rc;
  for (hipEvent_t& e : c->build_ev)
    if (!e) HIP_TRY(hipEventCreate(&e));
  Buf nodes, leaf_order, refit_order, fbox;
  auto drop = [&]() {
    for (Buf* b : {&nodes, &leaf_order, &refit_order, &fbox}) free_buf(*b);
  };
  if ((rc = alloc_buf(nodes, static_cast<size_t>(n_nodes) * sizeof(rt::BvhNodeQ))) || (rc = alloc_buf(leaf_order, static_cast<size_t>(total) * 4)) ||
      (rc = alloc_buf(refit_order, static_cast<size_t>(n_nodes) * 4)) || (rc = alloc_buf(fbox, static_cast<size_t>(n_nodes) * 12 * sizeof(float)))) {
    drop();
    return rc;
  }
  rt::LbvhArgs la;
  la.n_prims = n_prims;
  la.prim_w = w;
  la.tris = static_cast<const float*>(c->tris.ptr);
  la.nodes = static_cast<rt::BvhNodeQ*>(nodes.ptr);
  la.leaf_order = static_cast<uint32_t*>(leaf_order.ptr);
  la.refit_order = static_cast<uint32_t*>(refit_order.ptr);
  la.header = static_cast<uint32_t*>(c->bvh_build_header.ptr);
  la.by_height = c->lbvh_by_height ? 1u : 0u;
  uint32_t header[rt::kLbvhHeaderWords];
  hipError_t e = hipEventRecord(c->build_ev[0], c->stream);
  if (e == hipSuccess)
    e = sah ? rt::launch_sah_build(la, c->bvh_build_scratch.ptr, c->bvh_build_scratch.bytes, c->stream)
            : rt::launch_lbvh_build(la, c->bvh_build_scratch.ptr, c->bvh_build_scratch.bytes, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(header, c->bvh_build_header.ptr, sizeof header, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    drop();
    return fail(RTPT_E_DEVICE, std::string("device BVH build: ") + hipGetErrorString(e));
  }
  const uint32_t depth = header[0];
  uint32_t counted = 0, levels = 0;
  for (uint32_t h = 0; h < rt::kLbvhMaxLevels; h++) {
    counted += header[2 + h];
    if (header[2 + h]) levels = h + 1;
  }
  if (depth >= static_cast<uint32_t>(rt::kBvhMaxDepth)) {
    drop();
    *too_deep = true;
    return RTPT_OK;
  }
  if (sah && header[1] >= 1 && header[1] <= n_nodes) n_nodes = header[1];
  if (header[1] != n_nodes || counted != n_nodes || levels != std::max(depth, 1u)) {
    drop();
    return fail(RTPT_E_INVALID, "internal: the device BVH build lost nodes");
  }
  // the replaced tree is freed at the end: hipFree waits for the device, and the refit below should not wait behind it
  Buf old[4] = {c->nodes, c->leaf_order, c->refit_order, c->refit_fbox};
  c->nodes = nodes;
  c->leaf_order = leaf_order;
  c->refit_order = refit_order;
  c->refit_fbox = fbox;
  c->n_nodes = n_nodes;
  c->refit_level_first.assign(static_cast<size_t>(levels) + 1, 0);
  for (uint32_t h = 0; h < levels; h++) c->refit_level_first[h + 1] = c->refit_level_first[h] + header[2 + h];
  c->bvh_depth = static_cast<int>(depth);
  c->leaf_pairs = leaf_pairs;
  c->device_tree = true;
  rt::launch_refit(refit_args(c), c->refit_level_first.data(), static_cast<int>(levels), n_nodes, 1e-5f, c->stream);
  rt::launch_scene_prepare(scene_prep_args(c, total, leaf_pairs), c->stream);
  const int rcl = launch_check("device BVH build");
  const hipError_t ee = hipEventRecord(c->build_ev[1], c->stream);
  for (Buf& b : old) free_buf(b);
  c->bvh_host = rt::Bvh{};  // a device-built tree has no host copy (tens of megabytes to unmap for a large scene: after the events)
  free_buf(c->stack_spill);  // sized by the depth of the tree that was replaced
  c->stack_spill_blocks = 0;
  if (rcl) return rcl;
  HIP_TRY(ee);
  c->build_ms_pending = true;
  c->build_info.builder = sah ? static_cast<uint32_t>(RTPT_BUILDER_DEVICE_SAH) : static_cast<uint32_t>(RTPT_BVH_BUILDER_DEVICE_LBVH);
  c->build_info.fallback = RTPT_BVH_FALLBACK_NONE;
  c->build_info.n_primitives = n_prims;
  c->build_info.n_nodes = n_nodes;
  c->build_info.depth = depth;
  c->build_info.leaf_pairs = leaf_pairs ? 1u : 0u;
  c->build_info.build_ms = 0.f;
  return RTPT_OK;
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

// what rtpt_scene_upload leaves behind once the new scene is on the device (either builder); `tris` may be empty when
// the triangles were flattened on the device (then nothing on the host reads them)
int commit_uploaded_scene(rtpt_ctx* c, const MeshIn& in, std::vector<float>& tris, uint32_t total, bool paired_all) {
  try {
    c->mesh_xyz.assign(in.xyz, in.xyz + 3 * static_cast<size_t>(in.n_verts));
    c->mesh_idx.assign(in.idx, in.idx + 3 * static_cast<size_t>(in.n_tris));
  } catch (const std::bad_alloc&) {
    c->n_tris = 0;
    return fail(RTPT_E_NOMEM, "host allocation failed (mesh copy)");
  }
  c->n_instances = in.ni;
  c->has_xf = in.xf != nullptr;
  c->n_tris = total;
  c->n_base_tris = in.n_tris;
  free_buf(c->materials);  // materials belong to the mesh that was replaced
  if (total <= static_cast<uint32_t>(rt::kCullMaxTris))
    c->host_tris = tris;
  else
    c->host_tris.clear();
  c->tris_paired = paired_all && total <= static_cast<uint32_t>(rt::kCullMaxTris);  // the brute-force loops
  for (int i = 0; i < 16; i++) c->model[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  c->model_version++;
  c->scene_gen++;
  c->use_bvh = (total > 64) || (c->cfg.flags & RTPT_FLAG_FORCE_BVH);
  if (total <= static_cast<uint32_t>(rt::kCullMaxTris) || !refits_on_device(c))
    c->obj_tris.swap(tris);
  else
    std::vector<float>().swap(c->obj_tris);  // posed on the device from obj_tris_dev: the host copy is never read
  c->lut_prev_valid = false;
  c->lut_version[0] = c->lut_version[1] = ~0ull;
  c->tables_valid = false;
  c->normals_y0 = c->normals_y1 = 0;  // the per-pixel normal plane belongs to the previous scene
  return RTPT_OK;
}

// the device buffers of a scene of `total` triangles whose tree is built on the device
int alloc_device_scene(rtpt_ctx* c, uint32_t total) {
  int rc;
  const size_t tri_bytes = static_cast<size_t>(total) * 9 * sizeof(float);
  if ((rc = alloc_buf(c->tris, tri_bytes))) return rc;
  if ((rc = alloc_buf(c->obj_tris_dev, tri_bytes))) return rc;
  if ((rc = alloc_buf(c->isect_id, static_cast<size_t>(total) * 48))) return rc;
  if ((rc = alloc_buf(c->isect_leaf, static_cast<size_t>(total) * 48))) return rc;
  if ((rc = alloc_buf(c->shade, static_cast<size_t>(total) * 48))) return rc;
  if ((rc = alloc_buf(c->normal_tab, (static_cast<size_t>(total) + 1) * 32))) return rc;  // normals, then per-id areas
  if ((rc = alloc_buf(c->pair_tab, total + 1 <= 64 ? (static_cast<size_t>(total) + 1) * (total + 1) * 4 : 0))) return rc;
  for (int i = 0; i < 2; i++)
    if ((rc = alloc_buf(c->lut[i], (static_cast<size_t>(total) + 1) * sizeof(rtpt_visibility_data)))) return rc;
  return alloc_buf(c->bvh_grid_dev, 8 * sizeof(float));
}

// the mesh and room for its transforms, resident on the device: what k_flatten reads
int alloc_device_mesh(rtpt_ctx* c, uint32_t n_verts, uint32_t n_tris, uint32_t ni) {
  int rc;
  if ((rc = alloc_buf(c->mesh_xyz_dev, static_cast<size_t>(n_verts) * 12))) return rc;
  if ((rc = alloc_buf(c->mesh_idx_dev, static_cast<size_t>(n_tris) * 12))) return rc;
  return alloc_buf(c->xf_dev, static_cast<size_t>(ni) * 48);
}

void drop_device_mesh(rtpt_ctx* c) {
  for (Buf* b : {&c->mesh_xyz_dev, &c->mesh_idx_dev, &c->xf_dev}) free_buf(*b);
}

rt::FlattenArgs flatten_args(const rtpt_ctx* c, uint32_t n_tris, uint32_t total, bool with_xf) {
  rt::FlattenArgs fa;
  fa.n_tris = n_tris;
  fa.n_out_verts = total * 3;
  fa.xyz = static_cast<const float*>(c->mesh_xyz_dev.ptr);
  fa.idx = static_cast<const uint32_t*>(c->mesh_idx_dev.ptr);
  fa.xf = with_xf ? static_cast<const float*>(c->xf_dev.ptr) : nullptr;
  fa.out = static_cast<float*>(c->obj_tris_dev.ptr);
  return fa;
}

// rtpt_scene_upload with RTPT_FLAG_DEVICE_BVH_BUILD: the flattened triangles go up, the tree is built there
int upload_device_tree(rtpt_ctx* c, const MeshIn& in, std::vector<float>& tris, uint32_t total, bool paired_all, bool leaf_pairs, bool* too_deep) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc;
  if ((rc = alloc_device_scene(c, total))) return rc;
  drop_device_mesh(c);  // of the scene that is replaced
  c->n_tris = 0;  // the previous scene's buffers are gone: no scene until this one is complete
  HIP_TRY(hipMemcpyAsync(c->tris.ptr, tris.data(), tris.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->obj_tris_dev.ptr, tris.data(), tris.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  c->upload_info[0] += 2 * tris.size() * sizeof(float);
  for (int i = 0; i < 2; i++) HIP_TRY(hipMemsetAsync(c->lut[i].ptr, 0, c->lut[i].bytes, c->stream));
  // the builder's readback synchronises behind these copies, so the staging vector may die at return
  if ((rc = device_build_tree(c, total, leaf_pairs, too_deep)) || *too_deep) return rc;
  return commit_uploaded_scene(c, in, tris, total, paired_all);
}

// ... with RTPT_FLAG_DEVICE_FLATTEN too: only the mesh and the transforms go up; triangles and the fan-pair decision are
// made there (scene_flatten.hip), one word comes back before the build because the primitive width depends on it
int upload_device_flatten(rtpt_ctx* c, const MeshIn& in, uint32_t total, bool* too_deep) {
  // every kernel below indexes 3 x total vertices in 32 bits; the traversal's own limit is tighter and is checked first
  if (static_cast<uint64_t>(total) * 48u >= (1ull << 32))
    return fail(RTPT_E_INVALID, "scene too large for the traversal's 32-bit record offsets (more than 89,478,485 triangles)");
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc;
  if ((rc = alloc_device_scene(c, total)) || (rc = alloc_device_mesh(c, in.n_verts, in.n_tris, in.ni))) return rc;
  if (!c->pair_word.ptr && (rc = alloc_buf(c->pair_word, 4))) return rc;
  c->n_tris = 0;  // the previous scene's buffers are gone: no scene until this one is complete
  HIP_TRY(hipMemcpyAsync(c->mesh_xyz_dev.ptr, in.xyz, static_cast<size_t>(in.n_verts) * 12, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->mesh_idx_dev.ptr, in.idx, static_cast<size_t>(in.n_tris) * 12, hipMemcpyHostToDevice, c->stream));
  if (in.xf) HIP_TRY(hipMemcpyAsync(c->xf_dev.ptr, in.xf, static_cast<size_t>(in.ni) * 48, hipMemcpyHostToDevice, c->stream));
  c->upload_info[0] += static_cast<uint64_t>(in.n_verts) * 12 + static_cast<uint64_t>(in.n_tris) * 12 + (in.xf ? static_cast<uint64_t>(in.ni) * 48 : 0);
  rt::launch_flatten(flatten_args(c, in.n_tris, total, in.xf != nullptr), c->stream);
  const bool even = total >= 2 && total % 2 == 0;
  uint32_t word = 0;
  if (even) {
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->pair_word.ptr), 1, 1, c->stream));
    rt::launch_fan_pairs(total / 2, static_cast<const float*>(c->obj_tris_dev.ptr), static_cast<uint32_t*>(c->pair_word.ptr), c->stream);
    HIP_TRY(hipMemcpyAsync(&word, c->pair_word.ptr, 4, hipMemcpyDeviceToHost, c->stream));
  }
  rt::RefitModel rm{};  // a fresh upload stands under the identity model: tris = obj_tris_dev
  rm.identity = 1;
  rt::launch_pose(total * 3, static_cast<const float*>(c->obj_tris_dev.ptr), static_cast<float*>(c->tris.ptr), rm, c->stream);
  for (int i = 0; i < 2; i++) HIP_TRY(hipMemsetAsync(c->lut[i].ptr, 0, c->lut[i].bytes, c->stream));
  if ((rc = launch_check("device flatten"))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // the pair word; the caller's arrays may die at return
  const bool paired_all = even && word == 1u;
  if ((rc = device_build_tree(c, total, paired_all && !c->no_pairing, too_deep)) || *too_deep) return rc;
  std::vector<float> none;
  if ((rc = commit_uploaded_scene(c, in, none, total, paired_all))) return rc;
  c->upload_info[1] = c->upload_info[2] = 1;
  return RTPT_OK;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------ scene

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
  const uint32_t total = static_cast<uint32_t>(total64);
  const MeshIn in{xyz, n_verts, idx, n_tris, xf, ni};
  c->upload_info[0] = c->upload_info[1] = c->upload_info[2] = 0;
  uint32_t fallback = RTPT_BVH_FALLBACK_NONE;
  if (c->device_bvh && c->device_flatten && total > static_cast<uint32_t>(rt::kCullMaxTris)) {
    bool too_deep = false;
    const int rcd = upload_device_flatten(c, in, total, &too_deep);
    if (rcd) return rcd;
    if (!too_deep) {
      c->build_info.upload_ms = static_cast<float>(now_ms() - t_call);
      return RTPT_OK;
    }
    fallback = RTPT_BVH_FALLBACK_DEPTH;  // as below: the host path, flatten included, in the same call
  }
  std::vector<float> tris(static_cast<size_t>(total) * 9);
  host_flatten(xyz, idx, n_tris, xf, ni, tris.data());
  const bool paired_all = host_fan_pairs(tris.data(), total);
  const bool leaf_pairs = paired_all && !c->no_pairing;
  if (c->device_bvh && fallback == RTPT_BVH_FALLBACK_NONE) {
    bool too_deep = false;
    const int rcd = upload_device_tree(c, in, tris, total, paired_all, leaf_pairs, &too_deep);
    if (rcd) return rcd;
    if (!too_deep) {
      c->build_info.upload_ms = static_cast<float>(now_ms() - t_call);
      return RTPT_OK;
    }
    fallback = RTPT_BVH_FALLBACK_DEPTH;  // a radix tree deeper than the traversal stack: the host builder bounds its depth
  }
  const double t_build = now_ms();
  rt::Bvh bvh;  // built aside: a failed upload leaves the context's scene (and the topology a later refit uses) untouched
  rt::build_bvh(tris.data(), total, bvh, 1e-5f, leaf_pairs);
  if (bvh.max_depth >= rt::kBvhMaxDepth) return fail(RTPT_E_INVALID, "BVH deeper than the traversal stack");
  // the traversal addresses leaf records and nodes as base + 32-bit byte offset (48 bytes per triangle at most, 32 per node)
  if (static_cast<uint64_t>(total) * 48u >= (1ull << 32) || bvh.nodes.size() >= (1ull << 27))
    return fail(RTPT_E_INVALID, "scene too large for the traversal's 32-bit record offsets (more than 89,478,485 triangles)");
  if (bvh.leaf_order.size() != total) return fail(RTPT_E_INVALID, "internal: BVH lost triangles");
  if (leaf_pairs)  // the pairs-mode leaf test reads one pair record per leaf: a leaf of any other shape would be misread
    for (const rt::BvhNode& nd : bvh.nodes)
      for (int side = 0; side < 2; side++) {
        const uint32_t idx = side ? nd.ridx : nd.lidx, cnt = side ? nd.rcnt : nd.lcnt;
        if (idx != rt::kBvhEmpty && cnt && !rt::pair_leaf_ok(idx, cnt, bvh.leaf_order.data(), total))
          return fail(RTPT_E_INVALID, "internal: a pairs-mode BVH leaf is not one fan pair (2q, 2q + 1) from an even slot");
      }

  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc;
  if ((rc = alloc_buf(c->tris, tris.size() * sizeof(float)))) return rc;
  if ((rc = alloc_buf(c->leaf_order, static_cast<size_t>(total) * 4))) return rc;
  if ((rc = alloc_buf(c->isect_id, static_cast<size_t>(total) * 48))) return rc;
  if ((rc = alloc_buf(c->isect_leaf, static_cast<size_t>(total) * 48))) return rc;
  if ((rc = alloc_buf(c->shade, static_cast<size_t>(total) * 48))) return rc;
  std::vector<rt::BvhNodeQ> nodes_h;
  c->bvh_grid = rt::pack_quantised_nodes(bvh, nodes_h);
  const double build_ms = now_ms() - t_build;
  if ((rc = alloc_buf(c->nodes, nodes_h.size() * sizeof(rt::BvhNodeQ)))) return rc;
  if ((rc = alloc_buf(c->normal_tab, (static_cast<size_t>(total) + 1) * 32))) return rc;  // normals, then per-id areas
  if ((rc = alloc_buf(c->pair_tab, total + 1 <= 64 ? (static_cast<size_t>(total) + 1) * (total + 1) * 4 : 0))) return rc;
  for (int i = 0; i < 2; i++)
    if ((rc = alloc_buf(c->lut[i], (static_cast<size_t>(total) + 1) * sizeof(rtpt_visibility_data)))) return rc;
  drop_device_mesh(c);  // of the scene that is replaced
  c->upload_info[0] += 2 * tris.size() * sizeof(float);  // tris here, obj_tris_dev below
  HIP_TRY(hipMemcpyAsync(c->tris.ptr, tris.data(), tris.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->leaf_order.ptr, bvh.leaf_order.data(), static_cast<size_t>(total) * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->nodes.ptr, nodes_h.data(), nodes_h.size() * sizeof(rt::BvhNodeQ), hipMemcpyHostToDevice, c->stream));
  // the grid of the node boxes, read by the traversal from device memory (a device-side refit rewrites it)
  if ((rc = alloc_buf(c->bvh_grid_dev, 8 * sizeof(float)))) return rc;
  const float grid_h[8] = {c->bvh_grid.origin[0], c->bvh_grid.origin[1], c->bvh_grid.origin[2], c->bvh_grid.cell[0],
                           c->bvh_grid.cell[1], c->bvh_grid.cell[2], 0.f, 0.f};
  HIP_TRY(hipMemcpyAsync(c->bvh_grid_dev.ptr, grid_h, sizeof grid_h, hipMemcpyHostToDevice, c->stream));
  // device-side refit tables: nodes by HEIGHT (a node after both of its subtrees), the un-posed triangles, scratch boxes
  std::vector<uint32_t> order_h;
  c->refit_level_first.clear();
  c->n_nodes = static_cast<uint32_t>(nodes_h.size());
  {
    const size_t nn = nodes_h.size();
    std::vector<int> height(nn, 0);
    int maxh = 0;
    for (size_t ii = nn; ii-- > 0;) {  // pre-order numbering: children carry larger indices than their parent
      int hgt = 0;
      for (uint32_t ref : {nodes_h[ii].lref, nodes_h[ii].rref})
        if (ref != rt::kBvhEmpty && !(ref & 0x80000000u) && ref < nn) hgt = std::max(hgt, height[ref] + 1);
      height[ii] = hgt;
      maxh = std::max(maxh, hgt);
    }
    c->refit_level_first.assign(static_cast<size_t>(maxh) + 2, 0);
    for (size_t ii = 0; ii < nn; ii++) c->refit_level_first[static_cast<size_t>(height[ii]) + 1]++;
    for (size_t h = 1; h < c->refit_level_first.size(); h++) c->refit_level_first[h] += c->refit_level_first[h - 1];
    order_h.resize(nn);
    std::vector<uint32_t> fill(c->refit_level_first.begin(), c->refit_level_first.end() - 1);
    for (size_t ii = 0; ii < nn; ii++) order_h[fill[static_cast<size_t>(height[ii])]++] = static_cast<uint32_t>(ii);
  }
  if ((rc = alloc_buf(c->obj_tris_dev, tris.size() * sizeof(float)))) return rc;
  if ((rc = alloc_buf(c->refit_order, order_h.size() * 4))) return rc;
  if ((rc = alloc_buf(c->refit_fbox, order_h.size() * 12 * sizeof(float)))) return rc;
  HIP_TRY(hipMemcpyAsync(c->obj_tris_dev.ptr, tris.data(), tris.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->refit_order.ptr, order_h.data(), order_h.size() * 4, hipMemcpyHostToDevice, c->stream));
  for (int i = 0; i < 2; i++) HIP_TRY(hipMemsetAsync(c->lut[i].ptr, 0, c->lut[i].bytes, c->stream));
  rt::launch_scene_prepare(scene_prep_args(c, total, leaf_pairs), c->stream);
  if ((rc = launch_check("scene_prepare"))) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // host staging vectors die at return
  free_buf(c->stack_spill);  // sized by the depth of the tree that was replaced
  c->stack_spill_blocks = 0;
  c->leaf_pairs = leaf_pairs;  // the tree that was just built
  c->bvh_depth = bvh.max_depth;
  c->device_tree = false;
  c->build_ms_pending = false;
  c->build_info.builder = RTPT_BVH_BUILDER_HOST_SAH;
  c->build_info.fallback = fallback;
  c->build_info.n_primitives = leaf_pairs ? total / 2 : total;
  c->build_info.n_nodes = c->n_nodes;
  c->build_info.depth = static_cast<uint32_t>(bvh.max_depth);
  c->build_info.leaf_pairs = leaf_pairs ? 1u : 0u;
  c->build_info.build_ms = static_cast<float>(build_ms);
  c->bvh_host = std::move(bvh);  // only now: the upload succeeded
  if ((rc = commit_uploaded_scene(c, in, tris, total, paired_all))) return rc;
  c->build_info.upload_ms = static_cast<float>(now_ms() - t_call);
  return RTPT_OK;
}


// Pose the scene with a new model matrix (visibility.vert.glsl:24 `model * position`; the reference recomputes
// ubo.model every frame, main.cpp:1469, as the identity): world triangle = model * uploaded triangle, in the same
// fixed-order fma arithmetic the LUT uses (mat_row_point), the BVH keeps its topology and is REFIT to the moved
// triangles, the device records are rebuilt.  Every pass — K0, K2, the LUT — sees the posed geometry.
}  // extern "C"

// a device-built tree has no host copy (bvh_host is empty): it is refit on the device whatever traces the scene —
// also the small scenes that trace by brute force, whose host_tris are still re-posed on the host
bool rtpt_impl::refits_on_device(const rtpt_ctx* c) {
  return ((c->use_bvh && !c->host_refit) || c->device_tree) && c->obj_tris_dev.ptr && c->refit_order.ptr;
}

namespace {

// The posed scene follows its inputs: the un-posed triangles (obj_tris_dev / obj_tris — they change with
// rtpt_scene_set_instances) and the model (it changes with ubo.model, rtpt_gbuffer).  Whichever of the two changed, this is
// the one routine that re-poses, refits and rebuilds the records, and marks LUT, tables and frame reuse stale.
int repose_scene(rtpt_ctx* c, const float* model) {
  const uint32_t total = c->n_tris;
  const bool ident = is_identity(model);
  const bool small = total <= static_cast<uint32_t>(rt::kCullMaxTris);
  if ((small || !refits_on_device(c)) && c->obj_tris.size() != static_cast<size_t>(total) * 9)
    return fail(RTPT_E_INVALID, "internal: the host copy of the un-posed triangles is missing");
  if (refits_on_device(c)) {
    // everything on the device and on the context's stream: no upload, no synchronisation (refit.hip)
    rt::RefitModel rm;
    std::memcpy(rm.m, model, sizeof rm.m);
    rm.identity = ident ? 1 : 0;
    rt::launch_pose(total * 3, static_cast<const float*>(c->obj_tris_dev.ptr), static_cast<float*>(c->tris.ptr), rm, c->stream);
    rt::launch_refit(refit_args(c), c->refit_level_first.data(), static_cast<int>(c->refit_level_first.size()) - 1, c->n_nodes, 1e-5f, c->stream);
    rt::launch_scene_prepare(scene_prep_args(c, total, c->leaf_pairs), c->stream);
    int rcd = launch_check("device refit");
    if (rcd) return rcd;
    if (small) {
      // a small scene forced onto the BVH path: the screen bounds (unused while it is) still follow the pose
      c->host_tris.resize(static_cast<size_t>(total) * 9);
      for (size_t v = 0; v < static_cast<size_t>(total) * 3; v++) {
        const float* p = c->obj_tris.data() + 3 * v;
        const rt::f3 q{p[0], p[1], p[2]};
        float* o = c->host_tris.data() + 3 * v;
        o[0] = ident ? p[0] : rt::exact::mat_row_point(model, 0, q);
        o[1] = ident ? p[1] : rt::exact::mat_row_point(model, 1, q);
        o[2] = ident ? p[2] : rt::exact::mat_row_point(model, 2, q);
      }
    }
    std::memcpy(c->model, model, sizeof c->model);
    c->model_version++;
    c->scene_gen++;
    c->tables_valid = false;
    return RTPT_OK;
  }
  std::vector<float> tris(static_cast<size_t>(total) * 9);
  for (size_t v = 0; v < static_cast<size_t>(total) * 3; v++) {
    const float* p = c->obj_tris.data() + 3 * v;
    float* o = tris.data() + 3 * v;
    if (ident) {
      o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    } else {
      const rt::f3 q{p[0], p[1], p[2]};
      o[0] = rt::exact::mat_row_point(model, 0, q);
      o[1] = rt::exact::mat_row_point(model, 1, q);
      o[2] = rt::exact::mat_row_point(model, 2, q);
    }
  }
  rt::refit_bvh(tris.data(), total, c->bvh_host);
  std::vector<rt::BvhNodeQ> nodes_h;
  c->bvh_grid = rt::pack_quantised_nodes(c->bvh_host, nodes_h);
  if (nodes_h.size() * sizeof(rt::BvhNodeQ) != c->nodes.bytes) return fail(RTPT_E_INVALID, "internal: refit changed the node count");
  HIP_TRY(hipMemcpyAsync(c->tris.ptr, tris.data(), tris.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->nodes.ptr, nodes_h.data(), nodes_h.size() * sizeof(rt::BvhNodeQ), hipMemcpyHostToDevice, c->stream));
  const float grid_h[8] = {c->bvh_grid.origin[0], c->bvh_grid.origin[1], c->bvh_grid.origin[2], c->bvh_grid.cell[0],
                           c->bvh_grid.cell[1], c->bvh_grid.cell[2], 0.f, 0.f};
  HIP_TRY(hipMemcpyAsync(c->bvh_grid_dev.ptr, grid_h, sizeof grid_h, hipMemcpyHostToDevice, c->stream));
  rt::launch_scene_prepare(scene_prep_args(c, total, c->leaf_pairs), c->stream);
  int rc = launch_check("scene_prepare");
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));  // host staging vectors die at return
  if (small) c->host_tris.swap(tris);
  std::memcpy(c->model, model, sizeof c->model);
  c->model_version++;
  c->scene_gen++;
  c->tables_valid = false;  // per-id normals and pair weights follow the posed triangles
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
  HIP_TRY(hipMemcpyAsync(c->xf_dev.ptr, st.host, bytes, hipMemcpyHostToDevice, c->stream));
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
  if (!c->n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  if (!xf) return fail(RTPT_E_INVALID, "NULL argument");
  if (n_instances != c->n_instances)
    return fail(RTPT_E_INVALID, "the instance count is the upload's (1 for a scene uploaded without transforms): upload again to change it");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  const uint32_t total = c->n_tris, nt = c->n_base_tris, ni = n_instances;
  const float* mx = c->mesh_xyz.data();
  const uint32_t* mi = c->mesh_idx.data();
  // A refit keeps the topology, pairs included.  A pair inside one instance stays a pair (the same vertices through the
  // same transform and arithmetic); one that straddles two instances (odd triangle count) was a pair by coincidence
  if ((c->leaf_pairs || c->tris_paired) && (nt & 1u))
    for (uint32_t b = 0; b + 1 < ni; b++) {
      if ((static_cast<uint64_t>(b + 1) * nt - 1) & 1u) continue;  // the last triangle of instance b has an odd id: it ends a pair
      float ta[9], tb[9];
      flatten_tri(mx, mi, xf, b, nt - 1, ta);
      flatten_tri(mx, mi, xf, b + 1, 0, tb);
      if (!fan_pair(ta, tb))
        return fail(RTPT_E_INVALID, "these transforms separate a fan pair that straddles two instances: upload the scene again");
    }
  const bool small = total <= static_cast<uint32_t>(rt::kCullMaxTris);
  const bool on_device = refits_on_device(c);
  std::vector<float> obj;  // the host's un-posed triangles, where the host reads them (as commit_uploaded_scene keeps them)
  bool paired = c->tris_paired;
  if (small || !on_device) {
    obj.resize(static_cast<size_t>(total) * 9);
    host_flatten(mx, mi, nt, xf, ni, obj.data());
    paired = host_fan_pairs(obj.data(), total) && small;  // the brute-force loops
  }
  uint64_t bytes = 0;
  if (on_device) {
    int rc;
    if (!c->mesh_xyz_dev.ptr) {  // first move of a scene that was flattened on the host: the mesh goes up, once
      if ((rc = alloc_device_mesh(c, static_cast<uint32_t>(c->mesh_xyz.size() / 3), nt, ni))) {
        drop_device_mesh(c);
        return rc;
      }
      hipError_t e = hipMemcpyAsync(c->mesh_xyz_dev.ptr, mx, c->mesh_xyz.size() * 4, hipMemcpyHostToDevice, c->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(c->mesh_idx_dev.ptr, mi, c->mesh_idx.size() * 4, hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) {
        drop_device_mesh(c);
        return fail(RTPT_E_DEVICE, std::string("mesh copy: ") + hipGetErrorString(e));
      }
      bytes += c->mesh_xyz.size() * 4 + c->mesh_idx.size() * 4;
    }
    if ((rc = stage_transforms(c, xf, static_cast<size_t>(ni) * 48))) return rc;
    bytes += static_cast<uint64_t>(ni) * 48;
    rt::launch_flatten(flatten_args(c, nt, total, true), c->stream);
  } else {
    bytes = static_cast<uint64_t>(total) * 36;  // the posed triangles, copied by the host path below
  }
  if (small || !on_device) c->obj_tris.swap(obj);
  if (!on_device && c->obj_tris_dev.ptr) {
    // the device's un-posed triangles follow too: rtpt_scene_rebuild can move this scene onto the device-refit path later
    // (c->obj_tris outlives the copy; the host path below synchronises anyway)
    const hipError_t e = hipMemcpyAsync(c->obj_tris_dev.ptr, c->obj_tris.data(), static_cast<size_t>(total) * 36, hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
      c->obj_tris.swap(obj);
      return fail(RTPT_E_DEVICE, std::string("un-posed triangle copy: ") + hipGetErrorString(e));
    }
    bytes += static_cast<uint64_t>(total) * 36;
  }
  const bool paired_before = c->tris_paired;
  c->tris_paired = paired;
  const int rc = repose_scene(c, c->model);
  if (rc) {
    if (!on_device) {  // nothing reached the device: the scene is the one before the call
      c->obj_tris.swap(obj);
      c->tris_paired = paired_before;
    }
    return rc;
  }
  c->has_xf = true;
  c->upload_info[0] = bytes;
  c->upload_info[1] = on_device ? 1 : 0;
  c->upload_info[2] = 0;  // the pair decision is the upload's: topology is kept
  if (on_device) c->upload_info[3]++;
  return RTPT_OK;
}

int rtpt_scene_build_info(rtpt_ctx* c, struct rtpt_scene_build_info* out) {
  if (!c || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  if (c->build_ms_pending) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->build_ev[1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->build_ev[0], c->build_ev[1]));
    c->build_info.build_ms = ms;
    c->build_ms_pending = false;
  }
  *out = c->build_info;
  return RTPT_OK;
}

int rtpt_scene_rebuild(rtpt_ctx* c) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!c->n_tris || !c->nodes.ptr) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  const double t_call = now_ms();
  HIP_TRY(hipStreamSynchronize(c->stream));  // the tree's buffers are replaced
  c->scene_gen++;  // another tree may resolve a tie between equally near triangles differently
  bool too_deep = false;
  const int rc = device_build_tree(c, c->n_tris, c->leaf_pairs, &too_deep);
  if (rc) return rc;
  if (too_deep) return fail(RTPT_E_INVALID, "the rebuilt BVH would be deeper than the traversal stack: the tree was kept");
  c->build_info.upload_ms = static_cast<float>(now_ms() - t_call);
  return RTPT_OK;
}

int rtpt_scene_set_materials(rtpt_ctx* c, const uint32_t* tri_material, uint32_t n_tris, const rtpt_material* materials,
                             uint32_t n_materials) {
  if (!c) return fail(RTPT_E_INVALID, "ctx is NULL");
  if (!c->n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (!tri_material || !materials || !n_materials) {  // back to the reference's normal-keyed colours
    free_buf(c->materials);
    return RTPT_OK;
  }
  if (n_tris != c->n_base_tris) return fail(RTPT_E_INVALID, "one material index per triangle of the uploaded mesh");
  std::vector<float> rec(static_cast<size_t>(n_tris) * 8);
  for (uint32_t t = 0; t < n_tris; t++) {
    if (tri_material[t] >= n_materials) return fail(RTPT_E_INVALID, "material index out of range");
    const rtpt_material& m = materials[tri_material[t]];
    float* r = rec.data() + 8 * static_cast<size_t>(t);
    r[0] = m.albedo[0]; r[1] = m.albedo[1]; r[2] = m.albedo[2]; r[3] = 0.0f;
    r[4] = m.emission[0]; r[5] = m.emission[1]; r[6] = m.emission[2];
    r[7] = (m.emission[0] != 0.0f || m.emission[1] != 0.0f || m.emission[2] != 0.0f) ? 1.0f : 0.0f;
  }
  int rc = alloc_buf(c->materials, rec.size() * sizeof(float));
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->materials.ptr, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return RTPT_OK;
}

}  // extern "C"
