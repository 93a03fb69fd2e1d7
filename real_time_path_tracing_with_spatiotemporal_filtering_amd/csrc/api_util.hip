// api_util.hip — the entry points that take no context and touch no device (rtpt_util_*): the host-side stand-ins for glm and
// tinyobjloader, the host BVH checker and the mip-chain arithmetic.  No kernels.  The OBJ loaders are projections of
// obj_host.hpp's one parse: argument checks, the parse, the arrays, the hand-out.
#include "api_internal.hpp"
#include "env_host.hpp"
#include "obj_host.hpp"
#include "texture_host.hpp"

namespace {

int parse_obj(const char* path, rtpt_obj::Obj& o) {
  std::string err;
  return rtpt_obj::parse(path, &o, &err) ? fail(RTPT_E_INVALID, err) : RTPT_OK;
}

// The second half of the two-call pattern: without an array the count alone; with one, *count in is its capacity.
template <class T, class Count>
int hand_out(const T* src, size_t n, T* dst, Count* count, const char* too_small) {
  if (dst) {
    if (*count < n) return fail(RTPT_E_INVALID, too_small);
    std::copy(src, src + n, dst);
  }
  *count = static_cast<Count>(n);
  return RTPT_OK;
}

// `mtllib` files are looked up next to the OBJ; `usemtl` selects the material of the faces that follow; tri_material lines up
// with rtpt_util_load_obj's index array.  Material 0 is the default for faces without a usable `usemtl`.  A missing library is
// not an error: *n_materials comes back 0 (and *n_tris is still set) and the caller keeps the normal-keyed colours.
template <class Record>
int load_obj_materials(const char* path, uint32_t* tri_material, uint32_t* n_tris, Record* materials, uint32_t* n_materials,
                       Record (*rule)(const rtpt_obj::Material&)) {
  if (!path || !n_tris || !n_materials) return fail(RTPT_E_INVALID, "NULL argument");
  rtpt_obj::Obj o;
  if (int rc = parse_obj(path, o)) return rc;
  if (tri_material) rtpt_obj::copy_tri_material(o, tri_material);
  *n_tris = rtpt_obj::n_tris(o);
  if (!o.any_library) {
    *n_materials = 0;
    return RTPT_OK;
  }
  const std::vector<Record> records = rtpt_obj::records(o, rule);
  return hand_out(records.data(), records.size(), materials, n_materials, "materials array too small");
}

}  // namespace

extern "C" {

void rtpt_util_look_at(const float eye[3], const float center[3], const float up[3], float m[16]) {
  // glm::lookAtRH (main.cpp:482, :1470)
  using namespace rt;
  f3 e{eye[0], eye[1], eye[2]};
  f3 f = exact::normalize(f3{center[0], center[1], center[2]} - e);
  f3 s = exact::normalize(exact::cross(f, f3{up[0], up[1], up[2]}));
  f3 u = exact::cross(s, f);
  std::memset(m, 0, 16 * sizeof(float));
  m[0] = s.x; m[4] = s.y; m[8] = s.z;
  m[1] = u.x; m[5] = u.y; m[9] = u.z;
  m[2] = -f.x; m[6] = -f.y; m[10] = -f.z;
  m[12] = -exact::dot(s, e);
  m[13] = -exact::dot(u, e);
  m[14] = exact::dot(f, e);
  m[15] = 1.0f;
}

void rtpt_util_perspective(float fovy, float aspect, float zn, float zf, float m[16]) {
  // glm::perspectiveRH_ZO (D6; main.cpp:483, :1471)
  const float t = static_cast<float>(std::tan(static_cast<double>(fovy) * 0.5));
  std::memset(m, 0, 16 * sizeof(float));
  m[0] = 1.0f / (aspect * t);
  m[5] = 1.0f / t;
  m[10] = zf / (zn - zf);
  m[11] = -1.0f;
  m[14] = -(zf * zn) / (zf - zn);
}

static int bvh_check_impl(const float* build_tris, const float* tris, uint32_t n, bool pairs, uint64_t stats[8]) {
  if (!tris || !stats || n == 0) return fail(RTPT_E_INVALID, "NULL argument / empty scene");
  if (pairs && n % 2) return fail(RTPT_E_INVALID, "pairs mode needs an even triangle count (fan pairs 2q, 2q + 1)");
  rt::Bvh bvh;
  rt::build_bvh(build_tris ? build_tris : tris, n, bvh, 1e-5f, pairs);
  if (build_tris) rt::refit_bvh(tris, n, bvh);  // same topology, boxes recomputed for the moved triangles
  std::vector<rt::BvhNodeQ> q;
  const rt::BvhGrid g = rt::pack_quantised_nodes(bvh, q);
  for (int i = 0; i < 8; i++) stats[i] = 0;
  stats[0] = bvh.nodes.size();
  stats[2] = static_cast<uint64_t>(bvh.max_depth);
  std::vector<uint32_t> seen(n, 0);
  if (bvh.leaf_order.size() != n) stats[4] += 1;
  for (uint32_t id : bvh.leaf_order) {
    if (id >= n) {
      stats[4]++;
      continue;
    }
    seen[id]++;
  }
  for (uint32_t i = 0; i < n; i++)
    if (seen[i] != 1) stats[4]++;
  struct Item { uint32_t node; };
  // bounds of a subtree = union of the triangles below it: computed bottom-up by recursion with an explicit stack
  struct Bounds { float mn[3], mx[3]; };
  auto tri_bounds = [&](uint32_t first, uint32_t cnt) {
    Bounds b{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
    for (uint32_t j = 0; j < cnt; j++) {
      const uint32_t id = bvh.leaf_order[first + j];
      for (int v = 0; v < 3; v++)
        for (int a = 0; a < 3; a++) {
          const float x = tris[9 * static_cast<size_t>(id) + 3 * v + a];
          b.mn[a] = std::min(b.mn[a], x);
          b.mx[a] = std::max(b.mx[a], x);
        }
    }
    return b;
  };
  std::vector<Bounds> sub(bvh.nodes.size());
  std::vector<uint8_t> done(bvh.nodes.size(), 0);
  std::vector<uint32_t> st{0};
  while (!st.empty()) {
    const uint32_t ni = st.back();
    const rt::BvhNode& nd = bvh.nodes[ni];
    bool ready = true;
    for (int side = 0; side < 2; side++) {
      const uint32_t idx = side ? nd.ridx : nd.lidx, cnt = side ? nd.rcnt : nd.lcnt;
      if (idx == rt::kBvhEmpty || cnt) continue;
      if (idx >= bvh.nodes.size()) {
        stats[7]++;
        continue;
      }
      if (!done[idx]) {
        st.push_back(idx);
        ready = false;
      }
    }
    if (!ready) continue;
    st.pop_back();
    Bounds me{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
    for (int side = 0; side < 2; side++) {
      const uint32_t idx = side ? nd.ridx : nd.lidx, cnt = side ? nd.rcnt : nd.lcnt;
      const float* bmn = side ? nd.rmin : nd.lmin;
      const float* bmx = side ? nd.rmax : nd.lmax;
      if (idx == rt::kBvhEmpty) continue;
      Bounds cb;
      if (cnt) {
        stats[1]++;
        stats[3] = std::max<uint64_t>(stats[3], cnt);
        if (cnt > static_cast<uint32_t>(rt::kBvhMaxLeaf) || static_cast<uint64_t>(idx) + cnt > n) {
          stats[7]++;
          continue;
        }
        if (pairs && !rt::pair_leaf_ok(idx, cnt, bvh.leaf_order.data(), bvh.leaf_order.size())) stats[7]++;
        cb = tri_bounds(idx, cnt);
      } else {
        if (idx >= bvh.nodes.size()) continue;
        cb = sub[idx];
      }
      for (int a = 0; a < 3; a++) {
        if (!(bmn[a] <= cb.mn[a] && bmx[a] >= cb.mx[a])) stats[5]++;
        // the device box: origin + q * cell, evaluated as the traversal's arithmetic implies (binary32)
        const float qlo = std::fmaf(static_cast<float>(q[ni].box[rt::bvh_box_lo(side, a)]), g.cell[a], g.origin[a]);
        const float qhi = std::fmaf(static_cast<float>(q[ni].box[rt::bvh_box_hi(side, a)]), g.cell[a], g.origin[a]);
        if (!(qlo <= bmn[a] && qhi >= bmx[a])) stats[6]++;
        me.mn[a] = std::min(me.mn[a], cb.mn[a]);
        me.mx[a] = std::max(me.mx[a], cb.mx[a]);
      }
      const uint32_t want = cnt ? (0x80000000u | (idx << 2) | (cnt - 1u)) : idx;
      if ((side ? q[ni].rref : q[ni].lref) != want) stats[7]++;
    }
    sub[ni] = me;
    done[ni] = 1;
  }
  return RTPT_OK;
}

int rtpt_util_bvh_check(const float* tris, uint32_t n, uint64_t stats[8]) { return bvh_check_impl(nullptr, tris, n, false, stats); }
int rtpt_util_bvh_check_pairs(const float* tris, uint32_t n, int pairs, uint64_t stats[8]) {
  return bvh_check_impl(nullptr, tris, n, pairs != 0, stats);
}
int rtpt_util_bvh_refit_check(const float* built_for, const float* moved, uint32_t n, uint64_t stats[8]) {
  if (!built_for) return fail(RTPT_E_INVALID, "NULL argument");
  return bvh_check_impl(built_for, moved, n, false, stats);
}

int rtpt_util_texture_chain(uint32_t width, uint32_t height, uint32_t* n_levels, uint64_t* n_texels) {
  if (!width || !height || width > rtpt_tex::kMaxTexDim || height > rtpt_tex::kMaxTexDim)
    return fail(RTPT_E_INVALID, "a texture dimension is zero or above 65536");
  if (n_levels) *n_levels = rtpt_tex::chain_levels(width, height);
  if (n_texels) *n_texels = rtpt_tex::chain_texels(width, height);
  return RTPT_OK;
}

// ------------------------------------------------------------------------------------------ the OBJ loaders
// `v` and `f` records.  A face index out of range is an error, reported after the counts (and the arrays, when given) are written.
int rtpt_util_environment_from_latlong(const float* rgb, uint32_t width, uint32_t height, uint32_t n, float* texels_rgba_out) {
  if (const char* why = rtpt_env::from_latlong(rgb, width, height, n, texels_rgba_out)) return fail(RTPT_E_INVALID, why);
  return RTPT_OK;
}

int rtpt_util_load_obj(const char* path, float* xyz, uint32_t* n_verts, uint32_t* idx, uint32_t* n_tris) {
  if (!path || !n_verts || !n_tris) return fail(RTPT_E_INVALID, "NULL argument");
  rtpt_obj::Obj o;
  if (int rc = parse_obj(path, o)) return rc;
  if (xyz) std::copy(o.v.begin(), o.v.end(), xyz);
  if (idx) rtpt_obj::copy_indices(o, idx);
  *n_verts = rtpt_obj::n_verts(o);
  *n_tris = rtpt_obj::n_tris(o);
  return o.bad_vertex_index ? fail(RTPT_E_INVALID, rtpt_obj::kBadVertexIndex) : RTPT_OK;
}

// Materials of an OBJ (tinyobjloader hands main.cpp:416-428 the same information, which the
// reference ignores — its colours are keyed on the normal, raytrace.comp.glsl:155-163, and the .mtl its OBJ names is
// missing upstream).  Kd and Ke; with _ext also Ks, Ns and illum; with _ni also Ni and Tf: the rules of obj_host.hpp.
int rtpt_util_load_obj_materials(const char* path, uint32_t* tri_material, uint32_t* n_tris, rtpt_material* materials,
                                 uint32_t* n_materials) {
  return load_obj_materials(path, tri_material, n_tris, materials, n_materials, rtpt_obj::material_of);
}
int rtpt_util_load_obj_materials_ext(const char* path, uint32_t* tri_material, uint32_t* n_tris, rtpt_material_ext* materials,
                                     uint32_t* n_materials) {
  return load_obj_materials(path, tri_material, n_tris, materials, n_materials, rtpt_obj::material_ext_of);
}
int rtpt_util_load_obj_materials_ni(const char* path, uint32_t* tri_material, uint32_t* n_tris, rtpt_material_ext* materials,
                                    uint32_t* n_materials) {
  return load_obj_materials(path, tri_material, n_tris, materials, n_materials, rtpt_obj::material_ni_of);
}

// `vt` records and the vt of the corners.  A texcoord index out of range is an error, reported like rtpt_util_load_obj's.
int rtpt_util_load_obj_texcoords(const char* path, float* tri_uv, uint32_t* n_tris) {
  if (!path || !n_tris) return fail(RTPT_E_INVALID, "NULL argument");
  rtpt_obj::Obj o;
  if (int rc = parse_obj(path, o)) return rc;
  if (tri_uv) rtpt_obj::copy_tri_uv(o, tri_uv);
  *n_tris = rtpt_obj::n_tris(o);
  return o.bad_texcoord_index ? fail(RTPT_E_INVALID, rtpt_obj::kBadTexcoordIndex) : RTPT_OK;
}

// the vn side of the same parse (rtpt_scene_set_normals takes the two arrays as they are); a vn index out of range is not refused:
// its face is not smooth
int rtpt_util_load_obj_normals(const char* path, float* tri_normals, uint32_t* tri_smooth, uint32_t* n_tris) {
  if (!path || !n_tris) return fail(RTPT_E_INVALID, "NULL argument");
  rtpt_obj::Obj o;
  if (int rc = parse_obj(path, o)) return rc;
  if (tri_normals) rtpt_obj::copy_tri_normals(o, tri_normals, tri_smooth);
  *n_tris = rtpt_obj::n_tris(o);
  return RTPT_OK;
}

// the `map_Kd` names, NUL-terminated, one after the other; none without a readable library
int rtpt_util_load_obj_map_kd(const char* path, char* names, size_t* names_bytes, uint32_t* n_materials) {
  if (!path || !names_bytes || !n_materials) return fail(RTPT_E_INVALID, "NULL argument");
  rtpt_obj::Obj o;
  if (int rc = parse_obj(path, o)) return rc;
  std::string packed;
  uint32_t n = 0;
  if (o.any_library)
    for (const rtpt_obj::Material& m : o.materials) {
      packed.append(m.map_kd.c_str(), m.map_kd.size() + 1);
      n++;
    }
  if (int rc = hand_out(packed.data(), packed.size(), names, names_bytes, "names array too small")) return rc;
  *n_materials = n;
  return RTPT_OK;
}

}  // extern "C"
