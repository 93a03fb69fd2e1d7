// material_host.hpp — the host side of the extended materials (rtpt_scene_set_materials_ext), free of HIP so that a plain C++
// program can exercise it under a sanitizer (csrc/tests/material_host_check.cpp): the checks the call applies before anything
// reaches the device, the record packing, and the OBJ / MTL reader that also takes Ks, Ns and illum — and, for the smooth
// dielectrics (RTPT_MAT_DIELECTRIC, csrc/tests/dielectric_host_check.cpp), Ni and Tf.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rtpt.h"

namespace rtpt_mat {

constexpr uint32_t kMatFlags = RTPT_MAT_SPECULAR | RTPT_MAT_DIELECTRIC;

inline bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
inline bool nonzero3(const float* v) { return v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f; }

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

// the loader's rule for Ns: min(1, sqrt(2 / (Ns + 2))) in binary32; anything that is not a number in [0, 1] (Ns <= -2) is 1
inline float roughness_of_ns(float ns) {
  const float r = std::sqrt(2.0f / (ns + 2.0f));
  return r <= 1.0f ? r : 1.0f;
}

// rtpt_util_load_obj_materials' reader (same numbering, same tri_material, same Kd / Ke) that also takes Ks, Ns and illum of
// every `newmtl`.  The rule, a definition:
//   specular[] = Ks (0 without one); roughness = roughness_of_ns(Ns), 0 without an Ns line;
//   flags = RTPT_MAT_SPECULAR exactly when illum >= 3, Ks != 0 and Ke == 0 (an emitter stays diffuse: it ends the path anyway).
// tri_material may be NULL (count only).  *any_library: some `mtllib` of the OBJ could be read.  Returns 0, or -1 with *err set.
// with_ni (rtpt_util_load_obj_materials_ni): Ni and Tf are read too, and a material is a DIELECTRIC instead of what the rule above
// makes it exactly when illum is 4, 6, 7 or 9, it has an `Ni` line with a finite value >= 1, Ke == 0 and its colour is not 0 —
// the colour is Tf where a complete `Tf r g b` line exists, else Ks.  Such a material gets specular[] = colour, ior = Ni,
// roughness 0 and flags = RTPT_MAT_DIELECTRIC; every other material is the rule's above, the word of ior 0.
inline int load_obj_materials_rule(const char* path, uint32_t* tri_material, uint32_t* n_tris, std::vector<rtpt_material_ext>* out,
                                   bool* any_library, std::string* err, bool with_ni) {
  FILE* fp = std::fopen(path, "r");
  if (!fp) {
    *err = std::string("cannot open ") + path;
    return -1;
  }
  std::string dir(path);
  const size_t slash = dir.find_last_of('/');
  dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);
  auto fresh = []() {
    rtpt_material_ext m;
    std::memset(&m, 0, sizeof m);
    m.albedo[0] = m.albedo[1] = m.albedo[2] = 0.7f;
    return m;
  };
  std::vector<std::string> names{"<default>"};
  std::vector<rtpt_material_ext> mats{fresh()};
  std::vector<int> illum{0};
  struct Glass {  // with_ni: what the Ni and Tf lines of a material said
    bool has_ni = false, has_tf = false;
    float ni = 0.0f, tf[3] = {0.0f, 0.0f, 0.0f};
  };
  std::vector<Glass> glass{Glass{}};
  *any_library = false;
  auto blank = [](char ch) { return ch == ' ' || ch == '\t'; };
  auto word = [&](const char* q, std::string& w) {
    while (blank(*q)) q++;
    w.clear();
    while (*q && !blank(*q) && *q != '\n' && *q != '\r') w.push_back(*q++);
  };
  auto load_mtl = [&](const std::string& file) {
    FILE* mf = std::fopen((dir + file).c_str(), "r");
    if (!mf) return;
    *any_library = true;
    char ln[1024];
    int cur = -1;
    while (std::fgets(ln, sizeof ln, mf)) {
      const char* p = ln;
      while (blank(*p)) p++;
      if (!std::strncmp(p, "newmtl", 6) && blank(p[6])) {
        std::string nm;
        word(p + 6, nm);
        names.push_back(nm);
        mats.push_back(fresh());
        illum.push_back(0);
        glass.push_back(Glass{});
        cur = static_cast<int>(mats.size()) - 1;
      } else if (cur >= 0 && p[0] == 'K' && (p[1] == 'd' || p[1] == 'e' || p[1] == 's') && blank(p[2])) {
        float v[3];
        if (std::sscanf(p + 2, "%f %f %f", &v[0], &v[1], &v[2]) == 3) {
          rtpt_material_ext& m = mats[static_cast<size_t>(cur)];
          std::memcpy(p[1] == 'd' ? m.albedo : (p[1] == 'e' ? m.emission : m.specular), v, sizeof v);
        }
      } else if (cur >= 0 && p[0] == 'N' && p[1] == 's' && blank(p[2])) {
        float ns;
        if (std::sscanf(p + 2, "%f", &ns) == 1) mats[static_cast<size_t>(cur)].roughness = roughness_of_ns(ns);
      } else if (cur >= 0 && !std::strncmp(p, "illum", 5) && blank(p[5])) {
        int v;
        if (std::sscanf(p + 5, "%d", &v) == 1) illum[static_cast<size_t>(cur)] = v;
      } else if (with_ni && cur >= 0 && p[0] == 'N' && p[1] == 'i' && blank(p[2])) {
        float ni;
        if (std::sscanf(p + 2, "%f", &ni) == 1) {
          glass[static_cast<size_t>(cur)].has_ni = true;
          glass[static_cast<size_t>(cur)].ni = ni;
        }
      } else if (with_ni && cur >= 0 && p[0] == 'T' && p[1] == 'f' && blank(p[2])) {
        float v[3];
        if (std::sscanf(p + 2, "%f %f %f", &v[0], &v[1], &v[2]) == 3) {
          glass[static_cast<size_t>(cur)].has_tf = true;
          std::memcpy(glass[static_cast<size_t>(cur)].tf, v, sizeof v);
        }
      }
    }
    std::fclose(mf);
  };
  uint32_t nt = 0, cur_mat = 0;
  char line[2048];
  while (std::fgets(line, sizeof line, fp)) {
    const char* p = line;
    while (blank(*p)) p++;
    if (!std::strncmp(p, "mtllib", 6) && blank(p[6])) {
      std::string file;
      word(p + 6, file);
      load_mtl(file);
    } else if (!std::strncmp(p, "usemtl", 6) && blank(p[6])) {
      std::string nm;
      word(p + 6, nm);
      cur_mat = 0;
      for (size_t i = 1; i < names.size(); i++)
        if (names[i] == nm) cur_mat = static_cast<uint32_t>(i);
    } else if (p[0] == 'f' && blank(p[1])) {
      size_t corners = 0;
      const char* q = p + 2;
      while (*q) {
        while (blank(*q)) q++;
        if (*q == '\0' || *q == '\n' || *q == '\r') break;
        char* end = nullptr;
        (void)std::strtol(q, &end, 10);
        if (end == q) break;
        corners++;
        q = end;
        while (*q && !blank(*q) && *q != '\n' && *q != '\r') q++;
      }
      for (size_t k = 1; k + 1 < corners; k++) {
        if (tri_material) tri_material[nt] = cur_mat;
        nt++;
      }
    }
  }
  std::fclose(fp);
  for (size_t i = 0; i < mats.size(); i++)
    if (illum[i] >= 3 && nonzero3(mats[i].specular) && !nonzero3(mats[i].emission)) mats[i].flags = RTPT_MAT_SPECULAR;
  for (size_t i = 0; with_ni && i < mats.size(); i++) {
    const Glass& g = glass[i];
    const float* colour = g.has_tf ? g.tf : mats[i].specular;
    const bool glassy = illum[i] == 4 || illum[i] == 6 || illum[i] == 7 || illum[i] == 9;
    if (glassy && g.has_ni && std::isfinite(g.ni) && g.ni >= 1.0f && !nonzero3(mats[i].emission) && nonzero3(colour)) {
      std::memcpy(mats[i].specular, colour, 3 * sizeof(float));
      mats[i].ior = g.ni;
      mats[i].roughness = 0.0f;
      mats[i].flags = RTPT_MAT_DIELECTRIC;
    }
  }
  *n_tris = nt;
  out->swap(mats);
  return 0;
}
inline int load_obj_materials(const char* path, uint32_t* tri_material, uint32_t* n_tris, std::vector<rtpt_material_ext>* out,
                              bool* any_library, std::string* err) {
  return load_obj_materials_rule(path, tri_material, n_tris, out, any_library, err, false);
}
inline int load_obj_materials_ni(const char* path, uint32_t* tri_material, uint32_t* n_tris, std::vector<rtpt_material_ext>* out,
                                 bool* any_library, std::string* err) {
  return load_obj_materials_rule(path, tri_material, n_tris, out, any_library, err, true);
}

}  // namespace rtpt_mat
