// texture_host.hpp — the host side of the albedo textures, free of HIP so that a plain C++ program can exercise it (and a
// sanitizer build of that program can: csrc/tests/texture_host_check.cpp): the checks rtpt_scene_set_textures applies before
// anything reaches the device, the record packing, and the layout of the mip chains (csrc/tests/texture_mips_host_check.cpp
// exercises that part).  The OBJ / MTL reader is obj_host.hpp's; the texcoord and map_Kd loaders at the end of this file call it.
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

namespace rtpt_tex {

// limits a descriptor must meet so that the sampler's 32-bit index arithmetic (texture.hpp) cannot wrap
constexpr uint32_t kMaxTexDim = 65536u;
constexpr float kMaxUv = 18446744073709551616.0f;  // 2^64: interpolated coordinates of such corners stay finite

// The mip chain of a W x H texture (RTPT_TEX_MIPMAP), stated here once:
//   level l is max(1, W >> l) x max(1, H >> l) texels; there are floor(log2(max(W, H))) + 1 levels (the last is 1 x 1);
//   a chain the caller gives (RTPT_TEX_MIPS_GIVEN) holds level l right behind level l - 1, starting at first_texel;
//   a chain the library generates keeps level 0 where the caller put it and appends the other levels to the device atlas,
//   texture after texture in descriptor order, starting at texel n_texels.
// All of it in 64 bits: the 17 levels of a 65536 x 65536 texture hold 5,726,623,061 texels.
constexpr uint32_t kMaxTexLevels = 17u;  // kMaxTexDim = 2^16
// The device's per-texture level table (TexView::levels, one row per texture, only when some texture has RTPT_TEX_MIPMAP):
// kLevelRow dwords — [l] first texel of level l in the device atlas, l < 17; [17] the number of levels (1 without the flag);
// [18], [19] zero.
constexpr uint32_t kLevelRow = 20u, kLevelRowCount = 17u;

inline uint32_t level_dim(uint32_t n, uint32_t l) {
  const uint32_t d = l < 32u ? n >> l : 0u;
  return d ? d : 1u;
}
inline uint32_t chain_levels(uint32_t w, uint32_t h) {
  uint32_t m = w > h ? w : h, n = 0;
  for (; m; m >>= 1) n++;
  return n;  // 0 for a 0 x 0 texture, which check_textures refuses
}
inline uint64_t chain_texels(uint32_t w, uint32_t h) {
  uint64_t n = 0;
  for (uint32_t l = 0, levels = chain_levels(w, h); l < levels; l++) n += static_cast<uint64_t>(level_dim(w, l)) * level_dim(h, l);
  return n;
}
constexpr uint32_t kTexFlags = RTPT_TEX_NEAREST | RTPT_TEX_MIPMAP | RTPT_TEX_MIPS_GIVEN;
inline bool generates_chain(const rtpt_texture& t) { return (t.flags & (RTPT_TEX_MIPMAP | RTPT_TEX_MIPS_GIVEN)) == RTPT_TEX_MIPMAP; }
// texels the caller's array holds for this texture, from first_texel on
inline uint64_t given_texels(const rtpt_texture& t) {
  return (t.flags & RTPT_TEX_MIPS_GIVEN) ? chain_texels(t.width, t.height) : static_cast<uint64_t>(t.width) * t.height;
}
// texels the library appends to the device atlas for the generated levels of all textures (of checked descriptors)
inline uint64_t generated_texels(const rtpt_texture* textures, uint32_t n_textures) {
  uint64_t n = 0;
  for (uint32_t i = 0; i < n_textures; i++)
    if (generates_chain(textures[i])) n += chain_texels(textures[i].width, textures[i].height) - static_cast<uint64_t>(textures[i].width) * textures[i].height;
  return n;
}
inline bool any_mipmap(const rtpt_texture* textures, uint32_t n_textures) {
  for (uint32_t i = 0; i < n_textures; i++)
    if (textures[i].flags & RTPT_TEX_MIPMAP) return true;
  return false;
}

// Everything rtpt_scene_set_textures refuses, decided on arguments alone.  NULL: the arguments are fine.
inline const char* check_textures(const float* tri_uv, const uint32_t* tri_texture, uint32_t n_tris, uint32_t n_base_tris,
                                  const rtpt_texture* textures, uint32_t n_textures, size_t n_texels) {
  if (n_tris != n_base_tris) return "one uv record and one texture index per triangle of the uploaded mesh";
  uint64_t atlas = n_texels;  // the device atlas: the caller's texels, then the generated levels
  for (uint32_t i = 0; i < n_textures; i++) {
    const rtpt_texture& t = textures[i];
    if (t.width == 0 || t.height == 0) return "a texture has a zero dimension";
    if (t.width > kMaxTexDim || t.height > kMaxTexDim) return "a texture is larger than 65536 texels along an axis";
    if (t.flags & ~kTexFlags) return "unknown texture flag";
    if ((t.flags & RTPT_TEX_MIPS_GIVEN) && !(t.flags & RTPT_TEX_MIPMAP)) return "RTPT_TEX_MIPS_GIVEN without RTPT_TEX_MIPMAP";
    const uint64_t end = static_cast<uint64_t>(t.first_texel) + given_texels(t);
    if (end > n_texels || end > 0xFFFFFFFFull) return "a texture's rectangle (its whole chain, when given) lies beyond the texel array";
    if (generates_chain(t)) atlas += chain_texels(t.width, t.height) - static_cast<uint64_t>(t.width) * t.height;
    if (atlas > 0xFFFFFFFFull) return "the generated mip levels take the atlas beyond 2^32 - 1 texels";
  }
  for (uint32_t t = 0; t < n_tris; t++) {
    if (tri_texture[t] > n_textures) return "texture index out of range";
    for (int k = 0; k < 6; k++) {
      const float c = tri_uv[6 * static_cast<size_t>(t) + k];
      if (!(std::fabs(c) <= kMaxUv)) return "a uv coordinate is not finite (or beyond 2^64)";
    }
  }
  return nullptr;
}

// The level table of checked descriptors: n_textures rows of kLevelRow dwords (see above).  Every offset it holds, plus its
// level's texels, lies inside the device atlas of n_texels + generated_texels() texels.
inline void build_level_table(const rtpt_texture* textures, uint32_t n_textures, size_t n_texels, uint32_t* table) {
  uint64_t next_generated = n_texels;
  for (uint32_t i = 0; i < n_textures; i++) {
    const rtpt_texture& t = textures[i];
    uint32_t* row = table + static_cast<size_t>(kLevelRow) * i;
    std::memset(row, 0, kLevelRow * sizeof(uint32_t));
    const uint32_t levels = (t.flags & RTPT_TEX_MIPMAP) ? chain_levels(t.width, t.height) : 1u;
    row[kLevelRowCount] = levels;
    uint64_t at = t.first_texel;
    for (uint32_t l = 0; l < levels; l++) {
      row[l] = static_cast<uint32_t>(at);
      at += static_cast<uint64_t>(level_dim(t.width, l)) * level_dim(t.height, l);
      if (l == 0 && generates_chain(t)) at = next_generated;
    }
    if (generates_chain(t)) next_generated = at;
  }
}

// n_tris records of 8 floats: (u0 v0 u1 v1) (u2 v2, texture index as bits, 0) — TexView::records
inline void pack_records(const float* tri_uv, const uint32_t* tri_texture, uint32_t n_tris, float* out) {
  for (uint32_t t = 0; t < n_tris; t++) {
    float* r = out + 8 * static_cast<size_t>(t);
    std::memcpy(r, tri_uv + 6 * static_cast<size_t>(t), 6 * sizeof(float));
    std::memcpy(r + 6, tri_texture + t, sizeof(uint32_t));
    r[7] = 0.0f;
  }
}

// bytes of device memory a set of textures holds (the formula include/rtpt.h documents); without a mip flag the last two
// terms are zero
inline size_t device_bytes(uint32_t n_tris, uint32_t n_textures, size_t n_texels) {
  return 32 * static_cast<size_t>(n_tris) + 16 * static_cast<size_t>(n_textures) + 16 * n_texels;
}
inline size_t device_bytes(uint32_t n_tris, const rtpt_texture* textures, uint32_t n_textures, size_t n_texels) {
  return device_bytes(n_tris, n_textures, n_texels) + 16 * static_cast<size_t>(generated_texels(textures, n_textures)) +
         (any_mipmap(textures, n_textures) ? 4 * static_cast<size_t>(kLevelRow) * n_textures : 0);
}

// The texcoord side of the OBJ reader (obj_host.hpp): 6 floats per triangle, lined up with rtpt_util_load_obj's index array;
// a corner without a vt (`f v`, `f v//vn`) is (0, 0).  tri_uv may be NULL (count only).  Returns 0, or -1 with *err set; after
// a texcoord index out of range the count and the array are written all the same.
inline int load_obj_texcoords(const char* path, float* tri_uv, uint32_t* n_tris, std::string* err) {
  rtpt_obj::Obj o;
  if (rtpt_obj::parse(path, &o, err)) return -1;
  if (tri_uv) rtpt_obj::copy_tri_uv(o, tri_uv);
  *n_tris = rtpt_obj::n_tris(o);
  if (o.bad_texcoord_index) *err = rtpt_obj::kBadTexcoordIndex;
  return o.bad_texcoord_index ? -1 : 0;
}

// The `map_Kd` file name of every material of the OBJ's libraries, in rtpt_util_load_obj_materials' numbering: entry 0 is
// the default material (never textured), entry i the i-th `newmtl` over all `mtllib` files in file order.  Empty string: no
// map.  Returns 0 (names empty when the OBJ names no readable library), or -1 with *err set.
inline int load_obj_map_kd(const char* path, std::vector<std::string>* names, std::string* err) {
  names->clear();
  rtpt_obj::Obj o;
  if (rtpt_obj::parse(path, &o, err)) return -1;
  if (o.any_library)
    for (const rtpt_obj::Material& m : o.materials) names->push_back(m.map_kd);
  return 0;
}

}  // namespace rtpt_tex
