// texture_host_check.cpp — a plain C++ program (no HIP, no device) over texture_host.hpp: the texcoord / map_Kd readers on
// files it writes itself, every refusal of check_textures, and the record packing.  `make -C csrc texture-host-check` builds
// it with -fsanitize=address,undefined and runs it: the sanitizer run of the host code of rtpt_scene_set_textures.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../texture_host.hpp"

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

static void write_file(const std::string& path, const std::string& text) {
  FILE* f = std::fopen(path.c_str(), "w");
  CHECK(f);
  std::fputs(text.c_str(), f);
  std::fclose(f);
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string obj = dir + "/texture_host_check.obj", mtl = dir + "/texture_host_check.mtl";
  write_file(mtl, "newmtl a\nKd 1 1 1\nmap_Kd a.ppm\nnewmtl b\nnewmtl c\nmap_Kd -o 1 1 c.pfm\n");
  std::string text = "mtllib texture_host_check.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0.5 1.5 0\n"
                     "vt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvt 0.25 0.75\n"
                     "f 1/1 2/2 3/3\nf 1/1/1 3/3/1 4/4/1\nf 1//1 2//1 3//1\nf 1 2 3\nf -5/-5 -4/-4 -3/-3 -2/-2 -1/-1\n";
  text += "f 1/ 2/2 3/3\n";  // an empty vt: the corner gets (0, 0) and the face keeps its three corners
  text += "f";
  for (int i = 0; i < 900; i++) text += " 1/1";  // 3.6 KB, longer than the reader's 2048-byte line buffer: the line is read in
  text += "\n";                                  // pieces like rtpt_util_load_obj reads it, nothing is written beyond the buffer
  write_file(obj, text);

  std::string err;
  uint32_t nt = 0;
  CHECK(rtpt_tex::load_obj_texcoords(obj.c_str(), nullptr, &nt, &err) == 0);
  CHECK(nt >= 8);
  std::vector<float> uv(6 * static_cast<size_t>(nt), -1.0f);
  uint32_t nt2 = 0;
  CHECK(rtpt_tex::load_obj_texcoords(obj.c_str(), uv.data(), &nt2, &err) == 0 && nt2 == nt);
  const float want0[6] = {0, 0, 1, 0, 1, 1}, want1[6] = {0, 0, 1, 1, 0, 1}, want6[6] = {0, 0, 0, 1, 0.25f, 0.75f};
  for (int k = 0; k < 6; k++) {
    CHECK(uv[k] == want0[k] && uv[6 + k] == want1[k] && uv[12 + k] == 0 && uv[18 + k] == 0);
    CHECK(uv[24 + k] == want0[k] && uv[30 + k] == want1[k] && uv[36 + k] == want6[k]);
  }
  const float want7[6] = {0, 0, 1, 0, 1, 1};  // "1/ 2/2 3/3"
  for (int k = 0; k < 6; k++) CHECK(uv[42 + k] == want7[k]);
  std::vector<std::string> maps;
  CHECK(rtpt_tex::load_obj_map_kd(obj.c_str(), &maps, &err) == 0);
  CHECK(maps.size() == 4 && maps[0].empty() && maps[1] == "a.ppm" && maps[2].empty() && maps[3] == "c.pfm");
  CHECK(rtpt_tex::load_obj_texcoords((dir + "/no_such_file.obj").c_str(), nullptr, &nt2, &err) == -1);
  write_file(obj, "v 0 0 0\nvt 0 0\nf 1/1 1/2 1/1\n");
  CHECK(rtpt_tex::load_obj_texcoords(obj.c_str(), nullptr, &nt2, &err) == -1);
  CHECK(rtpt_tex::load_obj_map_kd(obj.c_str(), &maps, &err) == 0 && maps.empty());

  // check_textures: one accepted set, then every refusal
  const uint32_t n = 3;
  std::vector<float> tri_uv(6 * n, 0.5f);
  std::vector<uint32_t> tri_tex{0, 1, 2};
  std::vector<rtpt_texture> tex{{2, 2, 3, 0}, {3, 5, 10, RTPT_TEX_NEAREST}};
  const size_t n_texels = 25;
  auto check = [&]() { return rtpt_tex::check_textures(tri_uv.data(), tri_tex.data(), n, 3, tex.data(), 2, n_texels); };
  CHECK(check() == nullptr);
  CHECK(rtpt_tex::check_textures(tri_uv.data(), tri_tex.data(), n, 4, tex.data(), 2, n_texels) != nullptr);
  tri_tex[2] = 3;
  CHECK(check() != nullptr);
  tri_tex[2] = 2;
  tex[0].width = 0;
  CHECK(check() != nullptr);
  tex[0].width = 2;
  tex[1].height = 0;
  CHECK(check() != nullptr);
  tex[1].height = 5;
  tex[1].first_texel = 11;  // ends at 26 > 25
  CHECK(check() != nullptr);
  tex[1].first_texel = 0xFFFFFFFFu;  // 32-bit wrap of first_texel + w * h
  CHECK(check() != nullptr);
  tex[1].first_texel = 10;
  tex[1].width = 65536, tex[1].height = 65536;  // w * h = 2^32
  CHECK(check() != nullptr);
  tex[1].width = 70000, tex[1].height = 1;
  CHECK(check() != nullptr);
  tex[1].width = 3, tex[1].height = 5;
  tex[1].flags = 2;
  CHECK(check() != nullptr);
  tex[1].flags = RTPT_TEX_NEAREST;
  for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), 3e38f}) {
    tri_uv[7] = bad;
    CHECK(check() != nullptr);
  }
  tri_uv[7] = -1e6f;
  CHECK(check() == nullptr);

  // the packing: 8 floats per triangle, the index as bits in slot 6
  for (uint32_t i = 0; i < 6 * n; i++) tri_uv[i] = static_cast<float>(i) * 0.125f;
  std::vector<float> rec(8 * n, -1.0f);
  rtpt_tex::pack_records(tri_uv.data(), tri_tex.data(), n, rec.data());
  for (uint32_t t = 0; t < n; t++) {
    for (int k = 0; k < 6; k++) CHECK(rec[8 * t + k] == tri_uv[6 * t + k]);
    uint32_t bits;
    std::memcpy(&bits, &rec[8 * t + 6], 4);
    CHECK(bits == tri_tex[t] && rec[8 * t + 7] == 0.0f);
  }
  CHECK(rtpt_tex::device_bytes(3, 2, 25) == 32 * 3 + 16 * 2 + 16 * 25);
  std::remove(obj.c_str());
  std::remove(mtl.c_str());
  std::puts("texture_host_check ok");
  return 0;
}
