// textures.cpp — see textures.hpp
#include "textures.hpp"

#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <set>
#include <stdexcept>

namespace rtpt_host {

namespace {

// the next whitespace-separated header token from `pos` on, '#' comments skipped
std::string token(const std::string& d, size_t& pos, const std::string& path) {
  for (;;) {
    while (pos < d.size() && std::isspace(static_cast<unsigned char>(d[pos]))) pos++;
    if (pos < d.size() && d[pos] == '#') {
      while (pos < d.size() && d[pos] != '\n') pos++;
      continue;
    }
    break;
  }
  const size_t b = pos;
  while (pos < d.size() && !std::isspace(static_cast<unsigned char>(d[pos]))) pos++;
  if (pos == b) throw std::runtime_error(path + ": truncated image header");
  return d.substr(b, pos - b);
}

}  // namespace

Image load_image(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot read texture " + path);
  const std::string d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  const std::string magic = d.substr(0, 2);
  if (magic != "P6" && magic != "PF" && magic != "Pf")
    throw std::runtime_error(path + ": unsupported image format — textures are binary PPM (P6) or PFM files; convert other formats first");
  size_t pos = 0;
  (void)token(d, pos, path);
  const long w = std::atol(token(d, pos, path).c_str()), h = std::atol(token(d, pos, path).c_str());
  const std::string third = token(d, pos, path);
  pos++;  // the single whitespace that ends the header
  if (w <= 0 || h <= 0 || w > 65536 || h > 65536) throw std::runtime_error(path + ": bad image size");
  Image im;
  im.width = static_cast<uint32_t>(w);
  im.height = static_cast<uint32_t>(h);
  const size_t n = static_cast<size_t>(w) * static_cast<size_t>(h);
  im.rgba.assign(4 * n, 1.0f);
  if (magic == "P6") {
    const long maxval = std::atol(third.c_str());
    if (maxval <= 0 || maxval > 255) throw std::runtime_error(path + ": only 8-bit P6 images are supported");
    if (d.size() < pos + 3 * n) throw std::runtime_error(path + ": truncated image");
    const unsigned char* px = reinterpret_cast<const unsigned char*>(d.data()) + pos;
    for (long y = 0; y < h; y++)  // PPM stores the top row first
      for (long x = 0; x < w; x++)
        for (int c = 0; c < 3; c++)
          im.rgba[4 * (static_cast<size_t>(h - 1 - y) * w + x) + c] = static_cast<float>(px[3 * (static_cast<size_t>(y) * w + x) + c]) / 255.0f;
    return im;
  }
  const int ch = magic == "PF" ? 3 : 1;
  const bool little = std::atof(third.c_str()) < 0;
  if (d.size() < pos + 4 * n * ch) throw std::runtime_error(path + ": truncated image");
  const unsigned char* px = reinterpret_cast<const unsigned char*>(d.data()) + pos;
  for (size_t i = 0; i < n; i++)  // PFM stores the bottom row first
    for (int c = 0; c < 3; c++) {
      const unsigned char* b = px + 4 * (i * ch + (ch == 3 ? c : 0));
      const uint32_t bits = little ? (b[0] | b[1] << 8 | b[2] << 16 | static_cast<uint32_t>(b[3]) << 24)
                                   : (b[3] | b[2] << 8 | b[1] << 16 | static_cast<uint32_t>(b[0]) << 24);
      std::memcpy(&im.rgba[4 * i + c], &bits, 4);
    }
  return im;
}

SceneTextures load_scene_textures(const std::string& obj_path, const std::vector<uint32_t>& tri_material, bool nearest, bool mips) {
  SceneTextures out;
  if (tri_material.empty()) return out;
  size_t bytes = 0;
  uint32_t nm = 0;
  if (rtpt_util_load_obj_map_kd(obj_path.c_str(), nullptr, &bytes, &nm) != RTPT_OK) throw std::runtime_error(rtpt_last_error(nullptr));
  if (nm == 0) return out;
  std::vector<char> buf(bytes ? bytes : 1);
  if (rtpt_util_load_obj_map_kd(obj_path.c_str(), buf.data(), &bytes, &nm) != RTPT_OK) throw std::runtime_error(rtpt_last_error(nullptr));
  std::vector<std::string> maps;
  for (const char* p = buf.data(); maps.size() < nm; p += maps.back().size() + 1) maps.emplace_back(p);
  std::set<std::string> unique;
  for (const std::string& m : maps)
    if (!m.empty()) unique.insert(m);
  if (unique.empty()) return out;
  const std::vector<std::string> files(unique.begin(), unique.end());
  const size_t slash = obj_path.find_last_of('/');
  const std::string dir = slash == std::string::npos ? std::string() : obj_path.substr(0, slash + 1);
  for (const std::string& file : files) {
    const Image im = load_image(dir + file);
    out.textures.push_back(rtpt_texture{im.width, im.height, static_cast<uint32_t>(out.texels.size() / 4),
                                        (nearest ? RTPT_TEX_NEAREST : 0u) | (mips ? RTPT_TEX_MIPMAP : 0u)});
    out.texels.insert(out.texels.end(), im.rgba.begin(), im.rgba.end());
  }
  std::vector<uint32_t> of_material(maps.size(), 0);
  for (size_t m = 0; m < maps.size(); m++)
    if (!maps[m].empty())
      of_material[m] = static_cast<uint32_t>(std::lower_bound(files.begin(), files.end(), maps[m]) - files.begin()) + 1;
  uint32_t nt = 0;
  if (rtpt_util_load_obj_texcoords(obj_path.c_str(), nullptr, &nt) != RTPT_OK) throw std::runtime_error(rtpt_last_error(nullptr));
  if (nt != tri_material.size()) throw std::runtime_error(obj_path + ": texture coordinates and materials disagree on the triangle count");
  out.tri_uv.resize(6 * static_cast<size_t>(nt));
  if (rtpt_util_load_obj_texcoords(obj_path.c_str(), out.tri_uv.data(), &nt) != RTPT_OK) throw std::runtime_error(rtpt_last_error(nullptr));
  out.tri_texture.resize(nt);
  for (uint32_t t = 0; t < nt; t++) out.tri_texture[t] = tri_material[t] < of_material.size() ? of_material[tri_material[t]] : 0;
  return out;
}

}  // namespace rtpt_host
