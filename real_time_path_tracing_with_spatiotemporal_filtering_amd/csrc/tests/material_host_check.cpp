// material_host_check.cpp — a plain C++ program (no HIP, no device) over material_host.hpp: the Kd / Ke / Ks / Ns / illum reader
// on files it writes itself, every refusal of check_materials, and the record packing.  `make -C csrc material-host-check`
// builds it with -fsanitize=address,undefined and runs it: the sanitizer run of the host code of rtpt_scene_set_materials_ext.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../material_host.hpp"

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
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string obj = dir + "/material_host_check.obj", mtl = dir + "/material_host_check.mtl";
  // the rule's table: illum 2 / 3 / 5, Ks 0 0 0, Ns absent / 0 / 1000, an emitter with Ks, a negative Ns, broken lines
  write_file(mtl,
             "Ks 1 1 1\nNs 5\n"  // before any newmtl: ignored
             "newmtl diffuse2\nKd 0.1 0.2 0.3\nKs 0.5 0.5 0.5\nNs 1000\nillum 2\n"
             "newmtl mirror3\nKd 0.4 0.4 0.4\nKs 0.9 0.8 0.7\nillum 3\n"
             "newmtl rough5\nKs 0.5 0.25 0.125\nNs 0\nillum 5\n"
             "newmtl gloss3\nKs 1 1 1\nNs 1000\nillum 3\n"
             "newmtl black3\nKs 0 0 0\nNs 10\nillum 3\n"
             "newmtl lamp3\nKe 5 5 5\nKs 1 1 1\nillum 3\n"
             "newmtl odd\nKs 1 1\nNs\nillum\nNs -7\nKs 0.5 0.5 0.5\nillum 9\n");
  std::string text = "mtllib material_host_check.mtl\nmtllib no_such.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\n"
                     "f 1 2 3\nusemtl mirror3\nf 1 2 3 4\nusemtl nobody\nf 1 2 3\nusemtl odd\nf 1/1 2/2 3/3\n";
  text += "usemtl rough5\nf";
  for (int i = 0; i < 900; i++) text += " 1/1";  // longer than the reader's 2048-byte line buffer: read in pieces, as the old reader does
  text += "\n";
  write_file(obj, text);

  std::string err;
  uint32_t nt = 0;
  std::vector<rtpt_material_ext> m;
  bool lib = false;
  CHECK(rtpt_mat::load_obj_materials(obj.c_str(), nullptr, &nt, &m, &lib, &err) == 0);
  CHECK(lib && m.size() == 8 && nt >= 5);
  std::vector<uint32_t> tm(nt, 99u);
  uint32_t nt2 = 0;
  CHECK(rtpt_mat::load_obj_materials(obj.c_str(), tm.data(), &nt2, &m, &lib, &err) == 0 && nt2 == nt);
  CHECK(tm[0] == 0 && tm[1] == 2 && tm[2] == 2 && tm[3] == 0 && tm[4] == 7 && tm[5] == 3);
  CHECK(m[0].albedo[0] == 0.7f && m[0].flags == 0 && m[0].roughness == 0.0f && m[0].specular[0] == 0.0f);
  CHECK(m[1].albedo[1] == 0.2f && m[1].specular[0] == 0.5f && m[1].flags == 0);  // illum 2 stays diffuse
  CHECK(m[1].roughness == std::sqrt(2.0f / 1002.0f));
  CHECK(m[2].flags == RTPT_MAT_SPECULAR && m[2].roughness == 0.0f && m[2].specular[2] == 0.7f && m[2].albedo[0] == 0.4f);  // no Ns: mirror
  CHECK(m[3].flags == RTPT_MAT_SPECULAR && m[3].roughness == 1.0f && m[3].specular[1] == 0.25f);  // Ns 0
  CHECK(m[4].flags == RTPT_MAT_SPECULAR && m[4].roughness == std::sqrt(2.0f / 1002.0f));
  CHECK(m[5].flags == 0);  // Ks 0 0 0
  CHECK(m[6].flags == 0 && m[6].emission[0] == 5.0f);  // an emitter stays diffuse
  CHECK(m[7].flags == RTPT_MAT_SPECULAR && m[7].roughness == 1.0f && m[7].specular[0] == 0.5f);  // Ns -7: no number in [0, 1]
  CHECK(m[7]._pad == 0);
  CHECK(rtpt_mat::roughness_of_ns(-2.0f) == 1.0f && rtpt_mat::roughness_of_ns(std::numeric_limits<float>::quiet_NaN()) == 1.0f);
  CHECK(rtpt_mat::roughness_of_ns(std::numeric_limits<float>::infinity()) == 0.0f);
  CHECK(rtpt_mat::load_obj_materials((dir + "/no_such_file.obj").c_str(), nullptr, &nt2, &m, &lib, &err) == -1);
  write_file(obj, "v 0 0 0\nf 1 1 1\n");
  CHECK(rtpt_mat::load_obj_materials(obj.c_str(), nullptr, &nt2, &m, &lib, &err) == 0 && !lib && nt2 == 1);

  // check_materials: one accepted set, then every refusal
  const uint32_t n = 3;
  std::vector<uint32_t> tri{0, 1, 1};
  std::vector<rtpt_material_ext> mats(3);
  for (auto& x : mats) std::memset(&x, 0, sizeof x);
  mats[1].flags = RTPT_MAT_SPECULAR;
  mats[1].specular[0] = 0.5f;
  mats[1].roughness = 0.25f;
  mats[2].roughness = 7.0f;  // diffuse: the range is not asked for
  auto check = [&]() { return rtpt_mat::check_materials(tri.data(), n, 3, mats.data(), 3); };
  CHECK(check() == nullptr);
  CHECK(rtpt_mat::check_materials(tri.data(), n, 4, mats.data(), 3) != nullptr);
  tri[2] = 3;
  CHECK(check() != nullptr);
  tri[2] = 1;
  mats[2].flags = 2;  // unknown flag, on a material no triangle uses
  CHECK(check() != nullptr);
  mats[2].flags = 0;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (float bad : {nan, inf, -inf}) {
    float* slots[4] = {&mats[0].albedo[1], &mats[0].emission[2], &mats[2].specular[0], &mats[2].roughness};
    for (float* s : slots) {
      const float keep = *s;
      *s = bad;
      CHECK(check() != nullptr);
      *s = keep;
    }
  }
  for (float bad : {-0.125f, 1.0000001f, 2.0f}) {
    mats[1].roughness = bad;
    CHECK(check() != nullptr);
  }
  mats[1].roughness = 1.0f;
  CHECK(check() == nullptr);
  mats[1].emission[1] = 1e-30f;
  CHECK(check() != nullptr);
  mats[1].emission[1] = 0.0f;
  mats[1].roughness = 0.0f;
  CHECK(check() == nullptr);

  // the packing: diffuse records are rtpt_scene_set_materials', a specular one is (Ks, -g) (0, 0, 0, 0)
  mats[0].albedo[0] = 0.1f, mats[0].albedo[1] = 0.2f, mats[0].albedo[2] = 0.3f;
  mats[0].specular[0] = 9.0f;  // ignored
  mats[2].emission[1] = 4.0f;
  std::vector<float> rec(8 * n, -1.0f);
  CHECK(rtpt_mat::pack_records(tri.data(), n, mats.data(), rec.data()));
  CHECK(rec[0] == 0.1f && rec[1] == 0.2f && rec[2] == 0.3f && bits(rec[3]) == 0u && rec[7] == 0.0f);
  CHECK(rec[8] == 0.5f && bits(rec[11]) == 0x80000000u && rec[12] == 0.0f && rec[15] == 0.0f);  // the mirror: -0.0f, not 0
  mats[1].roughness = 0.25f;
  rtpt_mat::pack_records(tri.data(), n, mats.data(), rec.data());
  CHECK(rec[19] == -0.25f);
  tri[1] = tri[2] = 2;  // the specular material assigned to no triangle
  CHECK(!rtpt_mat::pack_records(tri.data(), n, mats.data(), rec.data()));
  CHECK(rec[8 + 5] == 4.0f && rec[8 + 7] == 1.0f && bits(rec[8 + 3]) == 0u);
  std::remove(obj.c_str());
  std::remove(mtl.c_str());
  std::puts("material_host_check ok");
  return 0;
}
