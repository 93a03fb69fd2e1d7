// obj_host.hpp — the OBJ / MTL reader, stated once and free of HIP so that a plain C++ program can exercise it under a sanitizer
// (csrc/tests/obj_host_check.cpp).  Two layers: parse() reads the OBJ and every library it names into one Obj value, storing
// what the lines said; the rules below it turn one parsed material into one record.  Every loader of the library
// (rtpt_util_load_obj*, api_util.hip; rtpt_mat::load_obj_materials*, rtpt_tex::load_obj_*) is a projection of the same Obj, which
// is why their arrays line up triangle for triangle and material for material.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtpt.h"

namespace rtpt_obj {

// ------------------------------------------------------------------------------------------ the parse layer
// what the lines of one `newmtl` said (entry 0 of Obj::materials is the default material, which no line describes)
struct Material {
  std::string name;
  float kd[3] = {0.7f, 0.7f, 0.7f};  // the reference's grey
  float ke[3] = {0.0f, 0.0f, 0.0f}, ks[3] = {0.0f, 0.0f, 0.0f};
  bool has_ns = false, has_ni = false, has_tf = false;  // a line of that keyword parsed completely
  float ns = 0.0f, ni = 0.0f, tf[3] = {0.0f, 0.0f, 0.0f};
  int illum = 0;
  std::string map_kd;  // empty: no map
};

struct Triangle {
  uint32_t v[3];      // resolved vertex indices (0-based), in range unless bad_vertex_index
  float uv[6];        // u0 v0 u1 v1 u2 v2; a corner without a usable vt is (0, 0)
  uint32_t material;  // index into Obj::materials, 0 without a usable `usemtl`
  float n[9];         // the corners' vn records; all 0 unless smooth
  uint32_t smooth;    // 1: every corner of the triangle's FACE names a vn record that exists (rtpt_util_load_obj_normals)
};

struct Obj {
  std::vector<float> v;   // 3 floats per `v` record
  std::vector<float> vt;  // 2 floats per `vt` record
  std::vector<float> vn;  // 3 floats per `vn` record
  std::vector<Triangle> tris;  // polygons fanned (0, k, k + 1) in file order (D5)
  // recorded, not refused: each matters to one loader only
  bool bad_vertex_index = false, bad_texcoord_index = false;
  bool bad_normal_index = false;  // (no loader refuses it: the face is not smooth)
  bool any_library = false;  // some `mtllib` of the OBJ could be read
  std::vector<Material> materials;
};
constexpr const char* kBadVertexIndex = "OBJ face index out of range";
constexpr const char* kBadTexcoordIndex = "OBJ texcoord index out of range";

inline bool blank(char ch) { return ch == ' ' || ch == '\t'; }
inline const char* skip_blank(const char* p) {
  while (blank(*p)) p++;
  return p;
}
inline bool at_end(const char* p) { return *p == '\0' || *p == '\n' || *p == '\r'; }
// a keyword counts only when a blank follows it: the text behind the keyword, or NULL
inline const char* after_keyword(const char* p, const char* keyword) {
  const size_t n = std::strlen(keyword);
  return !std::strncmp(p, keyword, n) && blank(p[n]) ? p + n : nullptr;
}
inline std::string word(const char* q) {
  q = skip_blank(q);
  std::string w;
  while (!at_end(q) && !blank(*q)) w.push_back(*q++);
  return w;
}
// a property line: *out changes only when every number of the line parses
inline bool three_floats(const char* q, float* out) {
  float v[3];
  if (std::sscanf(q, "%f %f %f", &v[0], &v[1], &v[2]) != 3) return false;
  std::memcpy(out, v, sizeof v);
  return true;
}
inline bool one_float(const char* q, float* out) {
  float v;
  if (std::sscanf(q, "%f", &v) != 1) return false;
  *out = v;
  return true;
}
// OBJ indices are 1-based; zero and negative ones count back from the n records read so far
inline long resolve_index(long i, size_t n) { return i > 0 ? i - 1 : static_cast<long>(n) + i; }

// One library: every `newmtl` appends a material; properties before the first one are ignored.  Lines are read into 1024 bytes,
// and the continuation of a longer line is read as a line of its own.
inline void parse_mtl(FILE* mf, Obj* o) {
  char ln[1024];
  Material* cur = nullptr;  // of this file
  while (std::fgets(ln, sizeof ln, mf)) {
    const char* p = skip_blank(ln);
    const char* q;
    if ((q = after_keyword(p, "newmtl"))) {
      o->materials.emplace_back();
      cur = &o->materials.back();
      cur->name = word(q);
    } else if (!cur) {
      continue;
    } else if ((q = after_keyword(p, "Kd"))) {
      three_floats(q, cur->kd);
    } else if ((q = after_keyword(p, "Ke"))) {
      three_floats(q, cur->ke);
    } else if ((q = after_keyword(p, "Ks"))) {
      three_floats(q, cur->ks);
    } else if ((q = after_keyword(p, "Tf"))) {
      if (three_floats(q, cur->tf)) cur->has_tf = true;
    } else if ((q = after_keyword(p, "Ns"))) {
      if (one_float(q, &cur->ns)) cur->has_ns = true;
    } else if ((q = after_keyword(p, "Ni"))) {
      if (one_float(q, &cur->ni)) cur->has_ni = true;
    } else if ((q = after_keyword(p, "illum"))) {
      int v;
      if (std::sscanf(q, "%d", &v) == 1) cur->illum = v;
    } else if ((q = after_keyword(p, "map_Kd"))) {
      // options before the name (`-s 1 1 1 file`) are not supported: the last word of the line is the name
      cur->map_kd.clear();
      for (q = skip_blank(q); !at_end(q); q = skip_blank(q)) {
        cur->map_kd = word(q);
        q += cur->map_kd.size();
      }
    }
  }
}

// The OBJ at `path` and the libraries it names, which are looked up next to it; a library that cannot be opened is not an
// error.  Lines are read into 2048 bytes, and the continuation of a longer line is read as a line of its own.
// Returns 0, or -1 with *err set ("cannot open <path>").
inline int parse(const char* path, Obj* o, std::string* err) {
  FILE* fp = std::fopen(path, "r");
  if (!fp) {
    *err = std::string("cannot open ") + path;
    return -1;
  }
  *o = Obj();
  o->materials.emplace_back();
  o->materials[0].name = "<default>";
  std::string dir(path);
  const size_t slash = dir.find_last_of('/');
  dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);
  struct Corner {
    uint32_t v;
    float uv[2];
    bool has_n;
    float n[3];
  };
  std::vector<Corner> poly;
  uint32_t cur_mat = 0;
  char line[2048];
  while (std::fgets(line, sizeof line, fp)) {
    const char* p = skip_blank(line);
    const char* q;
    if ((q = after_keyword(p, "v"))) {
      char* end = nullptr;
      float v[3];
      bool ok = true;
      for (int k = 0; k < 3; k++) {
        v[k] = std::strtof(q, &end);
        if (end == q) ok = false;
        q = end;
      }
      if (ok) o->v.insert(o->v.end(), v, v + 3);  // a `v` with fewer than three numbers takes no index
    } else if ((q = after_keyword(p, "vt"))) {
      char* end = nullptr;
      const float u = std::strtof(q, &end);
      if (end == q) continue;
      q = end;
      float v = std::strtof(q, &end);
      if (end == q) v = 0.0f;  // `vt u` is legal: v defaults to 0
      o->vt.push_back(u);
      o->vt.push_back(v);
    } else if ((q = after_keyword(p, "vn"))) {
      char* end = nullptr;
      float v[3];
      bool ok = true;
      for (int k = 0; k < 3; k++) {
        v[k] = std::strtof(q, &end);
        if (end == q) ok = false;
        q = end;
      }
      if (ok) o->vn.insert(o->vn.end(), v, v + 3);  // a `vn` with fewer than three numbers takes no index, like such a `v`
    } else if ((q = after_keyword(p, "mtllib"))) {
      if (FILE* mf = std::fopen((dir + word(q)).c_str(), "r")) {
        o->any_library = true;
        parse_mtl(mf, o);
        std::fclose(mf);
      }
    } else if ((q = after_keyword(p, "usemtl"))) {
      const std::string name = word(q);
      cur_mat = 0;  // an unknown name is the default material; of several materials of one name the last wins
      for (size_t i = 1; i < o->materials.size(); i++)
        if (o->materials[i].name == name) cur_mat = static_cast<uint32_t>(i);
    } else if ((q = after_keyword(p, "f"))) {
      // corners `v`, `v/vt`, `v/vt/vn`, `v//vn`; the walk stops at the first corner that does not start with a number
      poly.clear();
      while (*q) {
        q = skip_blank(q);
        if (at_end(q)) break;
        char* end = nullptr;
        const long vi = std::strtol(q, &end, 10);
        if (end == q) break;
        const long rv = resolve_index(vi, o->v.size() / 3);
        if (rv < 0 || rv >= static_cast<long>(o->v.size() / 3)) o->bad_vertex_index = true;
        Corner c{static_cast<uint32_t>(rv), {0.0f, 0.0f}, false, {0.0f, 0.0f, 0.0f}};
        q = end;
        // the vt number follows the slash at once (strtol would skip a blank and take the next corner's vertex number)
        if (*q == '/' && (q[1] == '-' || q[1] == '+' || (q[1] >= '0' && q[1] <= '9'))) {
          const long ti = std::strtol(q + 1, &end, 10);
          if (end != q + 1) {
            const long rt = resolve_index(ti, o->vt.size() / 2);
            if (rt < 0 || rt >= static_cast<long>(o->vt.size() / 2)) {
              o->bad_texcoord_index = true;
            } else {
              c.uv[0] = o->vt[2 * static_cast<size_t>(rt)];
              c.uv[1] = o->vt[2 * static_cast<size_t>(rt) + 1];
            }
            q = end;
          }
        }
        // the vn number follows the corner's second slash at once: `v/vt/vn` (q stands behind the vt), `v//vn`
        const char* sl = (*q == '/' && q[1] == '/') ? q + 1 : q;
        if (*sl == '/' && (sl[1] == '-' || sl[1] == '+' || (sl[1] >= '0' && sl[1] <= '9'))) {
          const long ni = std::strtol(sl + 1, &end, 10);
          if (end != sl + 1) {
            const long rn = resolve_index(ni, o->vn.size() / 3);
            if (rn < 0 || rn >= static_cast<long>(o->vn.size() / 3)) {
              o->bad_normal_index = true;
            } else {
              c.has_n = true;
              std::memcpy(c.n, o->vn.data() + 3 * static_cast<size_t>(rn), sizeof c.n);
            }
            q = end;
          }
        }
        poly.push_back(c);
        while (!at_end(q) && !blank(*q)) q++;  // the rest of the corner
      }
      bool face_smooth = true;  // every corner of the face has its vn
      for (const Corner& c : poly) face_smooth = face_smooth && c.has_n;
      for (size_t k = 1; k + 1 < poly.size(); k++) {
        const Corner* c[3] = {&poly[0], &poly[k], &poly[k + 1]};
        Triangle t;
        for (int j = 0; j < 3; j++) {
          t.v[j] = c[j]->v;
          t.uv[2 * j] = c[j]->uv[0];
          t.uv[2 * j + 1] = c[j]->uv[1];
          for (int a = 0; a < 3; a++) t.n[3 * j + a] = face_smooth ? c[j]->n[a] : 0.0f;
        }
        t.smooth = face_smooth ? 1u : 0u;
        t.material = cur_mat;
        o->tris.push_back(t);
      }
    }
  }
  std::fclose(fp);
  return 0;
}

// ------------------------------------------------------------------------------------------ projections
inline uint32_t n_verts(const Obj& o) { return static_cast<uint32_t>(o.v.size() / 3); }
inline uint32_t n_tris(const Obj& o) { return static_cast<uint32_t>(o.tris.size()); }
inline void copy_indices(const Obj& o, uint32_t* idx) {
  for (size_t t = 0; t < o.tris.size(); t++) std::memcpy(idx + 3 * t, o.tris[t].v, sizeof o.tris[t].v);
}
inline void copy_tri_uv(const Obj& o, float* tri_uv) {
  for (size_t t = 0; t < o.tris.size(); t++) std::memcpy(tri_uv + 6 * t, o.tris[t].uv, sizeof o.tris[t].uv);
}
inline void copy_tri_normals(const Obj& o, float* tri_normals, uint32_t* tri_smooth) {  // tri_smooth may be NULL
  for (size_t t = 0; t < o.tris.size(); t++) {
    std::memcpy(tri_normals + 9 * t, o.tris[t].n, sizeof o.tris[t].n);
    if (tri_smooth) tri_smooth[t] = o.tris[t].smooth;
  }
}
inline void copy_tri_material(const Obj& o, uint32_t* tri_material) {
  for (size_t t = 0; t < o.tris.size(); t++) tri_material[t] = o.tris[t].material;
}
// one record per material, entry 0 the default, by one of the rules below
template <class Record>
inline std::vector<Record> records(const Obj& o, Record (*rule)(const Material&)) {
  std::vector<Record> out;
  out.reserve(o.materials.size());
  for (const Material& m : o.materials) out.push_back(rule(m));
  return out;
}

// ------------------------------------------------------------------------------------------ the rule layer
inline bool nonzero3(const float* v) { return v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f; }

// the loader's rule for Ns: min(1, sqrt(2 / (Ns + 2))) in binary32; anything that is not a number in [0, 1] (Ns <= -2) is 1
inline float roughness_of_ns(float ns) {
  const float r = std::sqrt(2.0f / (ns + 2.0f));
  return r <= 1.0f ? r : 1.0f;
}

// Kd and Ke (rtpt_util_load_obj_materials): the default material is Kd 0.7, the reference's grey, and Ke 0
inline rtpt_material material_of(const Material& m) {
  rtpt_material r;
  std::memcpy(r.albedo, m.kd, sizeof r.albedo);
  std::memcpy(r.emission, m.ke, sizeof r.emission);
  return r;
}

// ... plus Ks, Ns and illum (rtpt_util_load_obj_materials_ext).  The rule, a definition:
//   specular[] = Ks (0 without one); roughness = roughness_of_ns(Ns), 0 without an Ns line;
//   flags = RTPT_MAT_SPECULAR exactly when illum >= 3, Ks != 0 and Ke == 0 (an emitter stays diffuse: it ends the path anyway).
inline rtpt_material_ext material_ext_of(const Material& m) {
  rtpt_material_ext r;
  std::memset(&r, 0, sizeof r);
  std::memcpy(r.albedo, m.kd, sizeof r.albedo);
  std::memcpy(r.emission, m.ke, sizeof r.emission);
  std::memcpy(r.specular, m.ks, sizeof r.specular);
  if (m.has_ns) r.roughness = roughness_of_ns(m.ns);
  if (m.illum >= 3 && nonzero3(m.ks) && !nonzero3(m.ke)) r.flags = RTPT_MAT_SPECULAR;
  return r;
}

// ... plus Ni and Tf (rtpt_util_load_obj_materials_ni): a material is a DIELECTRIC instead of what the rule above makes it exactly
// when illum is 4, 6, 7 or 9, it has an `Ni` line with a finite value >= 1, Ke == 0 and its colour is not 0 — the colour is Tf
// where a complete `Tf r g b` line exists, else Ks.  Such a material gets specular[] = colour, ior = Ni, roughness 0 and
// flags = RTPT_MAT_DIELECTRIC; every other material is the rule's above, the word of ior 0.
inline rtpt_material_ext material_ni_of(const Material& m) {
  rtpt_material_ext r = material_ext_of(m);
  const float* colour = m.has_tf ? m.tf : m.ks;
  const bool glassy = m.illum == 4 || m.illum == 6 || m.illum == 7 || m.illum == 9;
  if (glassy && m.has_ni && std::isfinite(m.ni) && m.ni >= 1.0f && !nonzero3(m.ke) && nonzero3(colour)) {
    std::memcpy(r.specular, colour, sizeof r.specular);
    r.ior = m.ni;
    r.roughness = 0.0f;
    r.flags = RTPT_MAT_DIELECTRIC;
  }
  return r;
}

}  // namespace rtpt_obj
