// material_host.hpp — the host side of the extended materials (rtpt_scene_set_materials_ext), free of HIP so that a plain C++
// program can exercise it under a sanitizer (csrc/tests/material_host_check.cpp): the checks the call applies before anything
// reaches the device, and the record packing — of the specular materials and of the smooth dielectrics (RTPT_MAT_DIELECTRIC,
// csrc/tests/dielectric_host_check.cpp).  The OBJ / MTL reader and its rules for Ks, Ns, illum, Ni and Tf are obj_host.hpp's; the
// two loaders at the end of this file call it.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtpt.h"
#include "obj_host.hpp"

namespace rtpt_mat {

using rtpt_obj::nonzero3;
using rtpt_obj::roughness_of_ns;  // the loader's rule for Ns, stated with the other rules of the reader

constexpr uint32_t kMatFlags = RTPT_MAT_SPECULAR | RTPT_MAT_DIELECTRIC;

inline bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// Everything rtpt_scene_set_materials_ext refuses, decided on arguments alone.  Every material of the table is checked, also
// one no triangle uses.  NULL: the arguments are fine.
inline const char* check_materials(const uint32_t* tri_material, uint32_t n_tris, uint32_t n_base_tris, const rtpt_material_ext* materials,
                                   uint32_t n_materials) {
  if (n_tris != n_base_tris) return "one material index per triangle of the uploaded mesh";
  for (uint32_t i = 0; i < n_materials; i++) {
    const rtpt_material_ext& m = materials[i];
    if (m.flags & ~kMatFlags) return "unknown material flag";
    if (!finite3(m.albedo) || !finite3(m.emission) || !finite3(m.specular) || !std::isfinite(m.roughness))
      return "a material component is not finite";
    if (m.flags & RTPT_MAT_SPECULAR) {
      if (!(m.roughness >= 0.0f && m.roughness <= 1.0f)) return "the roughness of a specular material lies outside [0, 1]";
      if (nonzero3(m.emission)) return "a specular material with a non-zero emission";
      if (m.flags & RTPT_MAT_DIELECTRIC) return "a material that is specular and dielectric";
    }
    if (m.flags & RTPT_MAT_DIELECTRIC) {  // (without the flag the word that carries ior is ignored)
      if (m.roughness != 0.0f) return "a dielectric material with a roughness other than 0";
      if (nonzero3(m.emission)) return "a dielectric material with a non-zero emission";
      if (!(std::isfinite(m.ior) && m.ior >= 1.0f)) return "the ior of a dielectric material is not a finite number >= 1";
    }
  }
  for (uint32_t t = 0; t < n_tris; t++)
    if (tri_material[t] >= n_materials) return "material index out of range";
  return nullptr;
}

// n_tris records of 8 floats (SceneView::materials): (Kd, 0) (Ke, emissive ? 1 : 0) — what rtpt_scene_set_materials packs — or,
// for a specular material, (Ks, -roughness) (0, 0, 0, 0): the spare word is 0 exactly for a diffuse one, -0.0f for the mirror.
// For a dielectric one (dielectric.hpp), (colour, ior) (inv, R0, 0, 0) with, in binary32, inv = 1 / ior, q = (ior - 1) / (ior + 1),
// R0 = q * q: ior >= 1 keeps the spare word positive.
// Returns what selects the SPEC kernels: kModeDielectric when some TRIANGLE's material is a dielectric, else kModeSpecular when
// some triangle's is specular, else kModeDiffuse.  Of checked arguments.
constexpr int kModeDiffuse = 0, kModeSpecular = 1, kModeDielectric = 2;
inline int pack_records_mode(const uint32_t* tri_material, uint32_t n_tris, const rtpt_material_ext* materials, float* out) {
  int mode = kModeDiffuse;
  for (uint32_t t = 0; t < n_tris; t++) {
    const rtpt_material_ext& m = materials[tri_material[t]];
    float* r = out + 8 * static_cast<size_t>(t);
    if (m.flags & RTPT_MAT_DIELECTRIC) {
      mode = kModeDielectric;
      const float q = (m.ior - 1.0f) / (m.ior + 1.0f);
      r[0] = m.specular[0]; r[1] = m.specular[1]; r[2] = m.specular[2]; r[3] = m.ior;
      r[4] = 1.0f / m.ior; r[5] = q * q; r[6] = r[7] = 0.0f;
    } else if (m.flags & RTPT_MAT_SPECULAR) {
      if (mode == kModeDiffuse) mode = kModeSpecular;
      r[0] = m.specular[0]; r[1] = m.specular[1]; r[2] = m.specular[2]; r[3] = -m.roughness;
      r[4] = r[5] = r[6] = r[7] = 0.0f;
    } else {
      r[0] = m.albedo[0]; r[1] = m.albedo[1]; r[2] = m.albedo[2]; r[3] = 0.0f;
      r[4] = m.emission[0]; r[5] = m.emission[1]; r[6] = m.emission[2];
      r[7] = nonzero3(m.emission) ? 1.0f : 0.0f;
    }
  }
  return mode;
}
// ... as a yes / no: some triangle's material is not diffuse
inline bool pack_records(const uint32_t* tri_material, uint32_t n_tris, const rtpt_material_ext* materials, float* out) {
  return pack_records_mode(tri_material, n_tris, materials, out) != kModeDiffuse;
}

// The material side of the OBJ / MTL reader (obj_host.hpp) as extended records: rtpt_util_load_obj_materials' numbering and
// tri_material, one record per material by the rule rtpt_obj::material_ext_of states.  tri_material may be NULL (count only).
// *any_library: some `mtllib` of the OBJ could be read.  Returns 0, or -1 with *err set.
inline int load_obj_materials_rule(const char* path, uint32_t* tri_material, uint32_t* n_tris, std::vector<rtpt_material_ext>* out,
                                   bool* any_library, std::string* err, rtpt_material_ext (*rule)(const rtpt_obj::Material&)) {
  rtpt_obj::Obj o;
  if (rtpt_obj::parse(path, &o, err)) return -1;
  if (tri_material) rtpt_obj::copy_tri_material(o, tri_material);
  *n_tris = rtpt_obj::n_tris(o);
  *any_library = o.any_library;
  *out = rtpt_obj::records(o, rule);
  return 0;
}
inline int load_obj_materials(const char* path, uint32_t* tri_material, uint32_t* n_tris, std::vector<rtpt_material_ext>* out,
                              bool* any_library, std::string* err) {
  return load_obj_materials_rule(path, tri_material, n_tris, out, any_library, err, rtpt_obj::material_ext_of);
}
// ... with Ni and Tf: the rule of rtpt_obj::material_ni_of (rtpt_util_load_obj_materials_ni)
inline int load_obj_materials_ni(const char* path, uint32_t* tri_material, uint32_t* n_tris, std::vector<rtpt_material_ext>* out,
                                 bool* any_library, std::string* err) {
  return load_obj_materials_rule(path, tri_material, n_tris, out, any_library, err, rtpt_obj::material_ni_of);
}

}  // namespace rtpt_mat
