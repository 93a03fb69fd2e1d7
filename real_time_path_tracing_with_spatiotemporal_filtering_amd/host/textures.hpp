// textures.hpp — albedo textures for the C++ host (--textures): image files (binary PPM and PFM only) and the atlas
// rtpt_scene_set_textures takes, from what the OBJ + MTL pair says (`vt`, `map_Kd`).  The Python host's textures.py, restated.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rtpt.h"

namespace rtpt_host {

// RGBA32F, linear, alpha 1, row 0 = the BOTTOM row of the picture (OBJ's v = 0).  `P6` with maxval <= 255 (byte / 255.0f)
// and `PF` / `Pf` of either byte order; anything else throws std::runtime_error naming the formats that work.
struct Image {
  uint32_t width = 0, height = 0;
  std::vector<float> rgba;
};
Image load_image(const std::string& path);

// what rtpt_scene_set_textures takes; empty `textures`: the OBJ's library names no map
struct SceneTextures {
  std::vector<float> tri_uv;
  std::vector<uint32_t> tri_texture;
  std::vector<rtpt_texture> textures;
  std::vector<float> texels;
};
// tri_material: rtpt_util_load_obj_materials' per-triangle indices of the same OBJ (empty: no library, no textures)
// mips: every texture gets RTPT_TEX_MIPMAP, with a chain the library generates (--texture-mips)
SceneTextures load_scene_textures(const std::string& obj_path, const std::vector<uint32_t>& tri_material, bool nearest, bool mips);

}  // namespace rtpt_host
