// obj_host_check.cpp — a plain C++ program (no HIP, no device) over obj_host.hpp and the loaders built on it: the parse, the three
// material rules and every projection, count-only and filling, over every OBJ of the corpus directory given as argv[1]
// (tests/golden/obj_reader) and over extremes it writes into argv[2] — an empty file, a file that is one 10 000-byte line, a face
// with 1000 corners, 300 materials.  It checks what the loaders promise of each other (one triangle numbering, one material
// numbering); what the values are is tests/test_obj_reader_cpu.py's business.  `make -C csrc obj-host-check` builds it with
// -fsanitize=address,undefined and runs it: the sanitizer run of the reader.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <string>
#include <vector>

#include "../material_host.hpp"
#include "../obj_host.hpp"
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
  std::fwrite(text.data(), 1, text.size(), f);
  std::fclose(f);
}

static void check_file(const std::string& path) {
  std::string err;
  rtpt_obj::Obj o;
  CHECK(rtpt_obj::parse(path.c_str(), &o, &err) == 0);
  const uint32_t nt = rtpt_obj::n_tris(o), nv = rtpt_obj::n_verts(o);
  CHECK(o.v.size() == 3 * static_cast<size_t>(nv) && o.vt.size() % 2 == 0);
  CHECK(!o.materials.empty() && o.materials[0].name == "<default>" && o.materials[0].map_kd.empty());

  // the projections into arrays of exactly the counted size: the sanitizer sees a write past either end
  std::vector<uint32_t> idx(3 * static_cast<size_t>(nt)), tri(nt);
  std::vector<float> uv(6 * static_cast<size_t>(nt));
  rtpt_obj::copy_indices(o, idx.data());
  rtpt_obj::copy_tri_uv(o, uv.data());
  rtpt_obj::copy_tri_material(o, tri.data());
  for (uint32_t t = 0; t < nt; t++) CHECK(tri[t] < o.materials.size());
  if (!o.bad_vertex_index)
    for (uint32_t i : idx) CHECK(i < nv);
  const std::vector<rtpt_material> kd = rtpt_obj::records(o, rtpt_obj::material_of);
  const std::vector<rtpt_material_ext> ext = rtpt_obj::records(o, rtpt_obj::material_ext_of);
  const std::vector<rtpt_material_ext> ni = rtpt_obj::records(o, rtpt_obj::material_ni_of);
  CHECK(kd.size() == o.materials.size() && ext.size() == kd.size() && ni.size() == kd.size());
  for (size_t i = 0; i < kd.size(); i++) {
    CHECK(!std::memcmp(kd[i].albedo, ext[i].albedo, 12) && !std::memcmp(kd[i].emission, ext[i].emission, 12));
    CHECK(!std::memcmp(kd[i].albedo, ni[i].albedo, 12) && !std::memcmp(kd[i].emission, ni[i].emission, 12));
    CHECK((ext[i].flags & ~RTPT_MAT_SPECULAR) == 0 && ext[i]._pad == 0);
    CHECK(ni[i].flags == RTPT_MAT_DIELECTRIC || !std::memcmp(&ni[i], &ext[i], sizeof ext[i]));
  }

  // the loaders of material_host.hpp and texture_host.hpp, count-only and then filling: the same numbers as the parse
  for (auto load : {rtpt_mat::load_obj_materials, rtpt_mat::load_obj_materials_ni}) {
    uint32_t n0 = ~0u, n1 = ~0u;
    std::vector<rtpt_material_ext> m0, m1;
    bool lib0 = !o.any_library, lib1 = !o.any_library;
    CHECK(load(path.c_str(), nullptr, &n0, &m0, &lib0, &err) == 0 && n0 == nt && lib0 == o.any_library);
    std::vector<uint32_t> tm(n0, ~0u);
    CHECK(load(path.c_str(), tm.data(), &n1, &m1, &lib1, &err) == 0 && n1 == nt && lib1 == o.any_library);
    CHECK(tm == tri && m0.size() == kd.size() && m1.size() == kd.size());
  }
  uint32_t n0 = ~0u, n1 = ~0u;
  CHECK(rtpt_tex::load_obj_texcoords(path.c_str(), nullptr, &n0, &err) == (o.bad_texcoord_index ? -1 : 0) && n0 == nt);
  std::vector<float> uv1(6 * static_cast<size_t>(n0), -1.0f);
  CHECK(rtpt_tex::load_obj_texcoords(path.c_str(), uv1.data(), &n1, &err) == (o.bad_texcoord_index ? -1 : 0) && n1 == nt);
  CHECK(uv1.empty() || !std::memcmp(uv1.data(), uv.data(), uv.size() * sizeof(float)));
  // the vn projection (rtpt_util_load_obj_normals): a smooth triangle's corners are vn records of the file bit for bit, any other is 0
  CHECK(o.vn.size() % 3 == 0);
  std::vector<float> nrm(static_cast<size_t>(nt) * 9, -1.0f);
  std::vector<uint32_t> smooth(nt, 7u);
  if (nt) rtpt_obj::copy_tri_normals(o, nrm.data(), smooth.data());
  if (nt) rtpt_obj::copy_tri_normals(o, nrm.data(), nullptr);
  uint32_t n_smooth = 0;
  for (uint32_t t = 0; t < nt; t++) {
    CHECK(smooth[t] <= 1u);
    n_smooth += smooth[t];
    for (int k = 0; k < 3; k++) {
      const float* c = nrm.data() + 9 * static_cast<size_t>(t) + 3 * k;
      bool found = !smooth[t];
      if (!smooth[t]) {
        const float zero[3] = {0.0f, 0.0f, 0.0f};
        CHECK(!std::memcmp(c, zero, sizeof zero));
      }
      for (size_t r = 0; !found && r < o.vn.size() / 3; r++) found = !std::memcmp(c, o.vn.data() + 3 * r, 12);
      CHECK(found);
    }
  }
  CHECK(!o.vn.empty() || n_smooth == 0);

  std::vector<std::string> maps{"stale"};
  CHECK(rtpt_tex::load_obj_map_kd(path.c_str(), &maps, &err) == 0);
  CHECK(maps.size() == (o.any_library ? o.materials.size() : 0));

  std::printf("obj_host_check: %s %u vertices, %u triangles (%u smooth), %zu materials%s%s%s%s\n", std::filesystem::path(path).filename().c_str(), nv, nt,
              n_smooth, o.materials.size(), o.any_library ? "" : ", no library", o.bad_vertex_index ? ", bad vertex index" : "",
              o.bad_texcoord_index ? ", bad texcoord index" : "", o.bad_normal_index ? ", bad normal index" : "");
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: obj_host_check <corpus directory> <scratch directory> [<second corpus directory>]\n");
    return 2;
  }
  std::vector<std::string> files;
  for (const auto& e : std::filesystem::directory_iterator(argv[1]))
    if (e.path().extension() == ".obj") files.push_back(e.path().string());
  if (argc > 3)  // the hostile vn files (tests/golden/obj_normals)
    for (const auto& e : std::filesystem::directory_iterator(argv[3]))
      if (e.path().extension() == ".obj") files.push_back(e.path().string());
  std::sort(files.begin(), files.end());
  CHECK(!files.empty());

  const std::string dir = argv[2];
  write_file(dir + "/empty.obj", "");
  write_file(dir + "/one_long_line.obj", "f " + std::string(9998, '1'));  // no newline: five buffers, a number no long holds
  std::string fan = "mtllib three_hundred_materials.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nusemtl m299\nf";
  for (int i = 0; i < 1000; i++) fan += " " + std::to_string(1 + i % 3);  // 2002 bytes: the longest face one buffer holds
  write_file(dir + "/thousand_corners.obj", fan + "\n");
  std::string mtl, faces = "mtllib three_hundred_materials.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\n";
  for (int i = 0; i < 300; i++) {
    const std::string n = std::to_string(i);
    mtl += "newmtl m" + n + "\nKd 0." + n + " 0.5 0.5\nKs 1 1 1\nNs " + n + "\nNi 1." + n + "\nillum " + std::to_string(i % 10) + "\nmap_Kd t" + n + ".ppm\n";
    faces += "usemtl m" + n + "\nf 1 2 3\n";
  }
  write_file(dir + "/three_hundred_materials.mtl", mtl);
  write_file(dir + "/three_hundred_materials.obj", faces);
  // vn extremes: a fan whose every corner names a normal by a negative index; slashes with nothing behind them; numbers no long holds
  std::string nfan = "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nvn 0 1 0\nf";
  for (int i = 0; i < 300; i++) nfan += " " + std::to_string(1 + i % 3) + "//-" + std::to_string(1 + i % 2);
  write_file(dir + "/normal_fan.obj", nfan + "\n");
  write_file(dir + "/normal_slashes.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 1 2 3\nvn\nvn 1\nf 1/ 2// 3///\nf 1//1 2//+1 3//-1\nf 1//99999999999999999999 2//1 3//1\n"
                                           "f 1//-99999999999999999999 2//1 3//1\nf 1/1/1 2/1/1 3/1/1\nf 1//1x 2//1 3//1 /1\n");
  for (const char* name : {"empty.obj", "one_long_line.obj", "thousand_corners.obj", "three_hundred_materials.obj", "normal_fan.obj", "normal_slashes.obj"})
    files.push_back(dir + "/" + name);

  for (const std::string& f : files) check_file(f);

  rtpt_obj::Obj o;
  std::string err;
  CHECK(rtpt_obj::parse((dir + "/thousand_corners.obj").c_str(), &o, &err) == 0);
  CHECK(rtpt_obj::n_tris(o) == 998 && o.tris[997].material == 300 && !o.bad_vertex_index && !o.bad_texcoord_index);
  CHECK(rtpt_obj::parse((dir + "/three_hundred_materials.obj").c_str(), &o, &err) == 0);
  CHECK(o.materials.size() == 301 && rtpt_obj::n_tris(o) == 300 && o.tris[299].material == 300 && o.materials[300].map_kd == "t299.ppm");
  CHECK(rtpt_obj::parse((dir + "/empty.obj").c_str(), &o, &err) == 0 && o.v.empty() && o.tris.empty() && !o.any_library);
  CHECK(rtpt_obj::parse((dir + "/no_such_file.obj").c_str(), &o, &err) == -1 && err == "cannot open " + dir + "/no_such_file.obj");
  CHECK(rtpt_obj::parse((dir + "/normal_fan.obj").c_str(), &o, &err) == 0);
  CHECK(rtpt_obj::n_tris(o) == 298 && o.tris[0].smooth == 1 && o.tris[297].smooth == 1 && !o.bad_normal_index);
  CHECK(o.tris[0].n[2] == 0.0f && o.tris[0].n[1] == 1.0f && o.tris[0].n[5] == 1.0f);  // corner 0: -1 = the last vn, corner 1: -2 = the first
  CHECK(rtpt_obj::parse((dir + "/normal_slashes.obj").c_str(), &o, &err) == 0);
  CHECK(o.vn.size() == 3 && rtpt_obj::n_tris(o) == 6 && o.bad_normal_index);
  CHECK(!o.tris[0].smooth && o.tris[1].smooth && !o.tris[2].smooth && !o.tris[3].smooth && o.tris[4].smooth && o.tris[5].smooth);
  CHECK(o.tris[1].n[0] == 1.0f && o.tris[1].n[4] == 2.0f && o.tris[1].n[8] == 3.0f);
  std::puts("obj_host_check: ok");
  return 0;
}
