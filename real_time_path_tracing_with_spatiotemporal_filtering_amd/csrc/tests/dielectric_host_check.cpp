// dielectric_host_check.cpp — a plain C++ program (no HIP, no device) over material_host.hpp's dielectric side: the Ni / Tf reader
// on files it writes itself next to the old reader on the same files, every refusal check_materials adds for
// RTPT_MAT_DIELECTRIC, and the record's ior, 1 / ior and R0.  `make -C csrc dielectric-host-check` builds it with
// -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstddef>
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
  static_assert(sizeof(rtpt_material_ext) == 48, "the union keeps the struct's size");
  static_assert(offsetof(rtpt_material_ext, ior) == 44 && offsetof(rtpt_material_ext, _pad) == 44, "ior is the word _pad names");
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string obj = dir + "/dielectric_host_check.obj", mtl = dir + "/dielectric_host_check.mtl";
  write_file(mtl,
             "Ni 1.5\nTf 1 1 1\n"  // before any newmtl: ignored
             "newmtl glass7\nKd 0.4 0.4 0.4\nKs 0.9 0.8 0.7\nNs 100\nNi 1.5\nillum 7\n"
             "newmtl tf4\nKs 0.9 0.8 0.7\nTf 0.25 0.5 0.75\nNi 2.417\nillum 4\n"
             "newmtl mirror7\nKs 0.9 0.8 0.7\nTf 0.25 0.5 0.75\nillum 7\n"  // no Ni
             "newmtl mirror3\nKs 0.9 0.8 0.7\nNi 1.5\nillum 3\n"            // illum 3
             "newmtl thin\nKs 0.9 0.8 0.7\nNi 0.5\nillum 6\n"               // Ni < 1
             "newmtl lamp\nKs 1 1 1\nKe 5 5 5\nNi 1.5\nillum 9\n"           // an emitter
             "newmtl black\nKs 1 1 1\nTf 0 0 0\nNi 1.5\nillum 9\n"          // a complete Tf of 0 is the colour
             "newmtl odd\nKs 0.5 0.5 0.5\nTf 0.1 0.2\nNi\nNi x\nTf\nillum 9\nNi inf\n"   // broken lines, a Ni that is not finite
             "newmtl one\nKs 0.5 0.5 0.5\nNi 1\nillum 6\n");
  write_file(obj, "mtllib dielectric_host_check.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3\nusemtl glass7\nf 1 2 3 4\nusemtl one\nf 1 2 3\n");

  std::string err;
  uint32_t nt = 0;
  std::vector<rtpt_material_ext> m, e;
  bool lib = false;
  CHECK(rtpt_mat::load_obj_materials_ni(obj.c_str(), nullptr, &nt, &m, &lib, &err) == 0);
  CHECK(lib && m.size() == 10 && nt == 4);
  std::vector<uint32_t> tm(nt, 99u), te(nt, 98u);
  CHECK(rtpt_mat::load_obj_materials_ni(obj.c_str(), tm.data(), &nt, &m, &lib, &err) == 0);
  CHECK(rtpt_mat::load_obj_materials(obj.c_str(), te.data(), &nt, &e, &lib, &err) == 0 && e.size() == m.size());
  CHECK(tm == te && tm[0] == 0 && tm[1] == 1 && tm[2] == 1 && tm[3] == 9);
  CHECK(m[1].flags == RTPT_MAT_DIELECTRIC && m[1].ior == 1.5f && m[1].roughness == 0.0f && m[1].specular[0] == 0.9f && m[1].albedo[0] == 0.4f);
  CHECK(m[2].flags == RTPT_MAT_DIELECTRIC && m[2].ior == 2.417f && m[2].specular[0] == 0.25f && m[2].specular[2] == 0.75f);  // Tf, not Ks
  CHECK(m[9].flags == RTPT_MAT_DIELECTRIC && m[9].ior == 1.0f && m[9].specular[1] == 0.5f);
  for (size_t i : {size_t(0), size_t(3), size_t(4), size_t(5), size_t(6), size_t(7), size_t(8)})  // every other one is the old reader's, bit for bit
    CHECK(std::memcmp(&m[i], &e[i], sizeof(rtpt_material_ext)) == 0 && m[i]._pad == 0);
  CHECK(m[3].flags == RTPT_MAT_SPECULAR && m[4].flags == RTPT_MAT_SPECULAR && m[5].flags == RTPT_MAT_SPECULAR);
  CHECK(m[6].flags == 0 && m[6].emission[0] == 5.0f);
  CHECK(m[7].flags == RTPT_MAT_SPECULAR && m[7].specular[0] == 1.0f);  // Tf 0 0 0: not glass, and Ks stays the mirror's colour
  CHECK(m[8].flags == RTPT_MAT_SPECULAR && m[8].specular[0] == 0.5f);
  for (size_t i = 0; i < e.size(); i++) CHECK(e[i]._pad == 0 && !(e[i].flags & RTPT_MAT_DIELECTRIC));  // the old reader knows no Ni
  CHECK(e[1].flags == RTPT_MAT_SPECULAR && e[1].roughness == std::sqrt(2.0f / 102.0f));

  // check_materials: an accepted dielectric, then every refusal it adds
  std::vector<uint32_t> tri{0, 1, 1};
  std::vector<rtpt_material_ext> mats(2);
  for (auto& x : mats) std::memset(&x, 0, sizeof x);
  mats[1].flags = RTPT_MAT_DIELECTRIC;
  mats[1].specular[0] = 0.5f;
  mats[1].ior = 1.5f;
  auto check = [&]() { return rtpt_mat::check_materials(tri.data(), 3, 3, mats.data(), 2); };
  CHECK(check() == nullptr);
  mats[1].ior = 1.0f;
  CHECK(check() == nullptr);
  mats[1].flags = RTPT_MAT_DIELECTRIC | RTPT_MAT_SPECULAR;
  CHECK(check() != nullptr);
  mats[1].flags = RTPT_MAT_DIELECTRIC;
  mats[1].roughness = 0.25f;
  CHECK(check() != nullptr);
  mats[1].roughness = 0.0f;
  mats[1].emission[2] = 1e-30f;
  CHECK(check() != nullptr);
  mats[1].emission[2] = 0.0f;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  for (float bad : {nan, inf, -inf, 0.0f, 0.99999994f, -1.5f}) {
    mats[1].ior = bad;
    CHECK(check() != nullptr);
  }
  mats[1].ior = 1.5f;
  CHECK(check() == nullptr);
  mats[0]._pad = 0x7fc00000u;  // without the flag the word is ignored
  CHECK(check() == nullptr);
  mats[0]._pad = 0;

  // the packing: (colour, ior) (1 / ior, R0, 0, 0); the mode says which kernels a set needs
  std::vector<float> rec(8 * 3, -1.0f);
  CHECK(rtpt_mat::pack_records_mode(tri.data(), 3, mats.data(), rec.data()) == rtpt_mat::kModeDielectric);
  CHECK(rec[8] == 0.5f && rec[11] == 1.5f && rec[12] == 1.0f / 1.5f && rec[13] == (0.5f / 2.5f) * (0.5f / 2.5f) && rec[14] == 0.0f && rec[15] == 0.0f);
  CHECK(bits(rec[3]) == 0u && rec[7] == 0.0f);
  CHECK(rtpt_mat::pack_records(tri.data(), 3, mats.data(), rec.data()));
  tri[1] = tri[2] = 0;  // the dielectric assigned to no triangle
  CHECK(rtpt_mat::pack_records_mode(tri.data(), 3, mats.data(), rec.data()) == rtpt_mat::kModeDiffuse);
  mats[0].flags = RTPT_MAT_SPECULAR;
  CHECK(rtpt_mat::pack_records_mode(tri.data(), 3, mats.data(), rec.data()) == rtpt_mat::kModeSpecular);
  tri[2] = 1;
  CHECK(rtpt_mat::pack_records_mode(tri.data(), 3, mats.data(), rec.data()) == rtpt_mat::kModeDielectric);
  std::remove(obj.c_str());
  std::remove(mtl.c_str());
  std::puts("dielectric_host_check ok");
  return 0;
}
