// light_list_host_check.cpp — a plain C++ program (no HIP, no device) over light_list_host.hpp: the light list of next-event
// estimation on hand-made tables, for both material struct types, 1 to 3 instances, and the bound of 2^24 entries from either
// side.  `make -C csrc light-list-host-check` builds it with -fsanitize=address,undefined and runs it: the sanitizer run of the
// host code rtpt_scene_set_materials and rtpt_scene_set_materials_ext build the list with.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../light_list_host.hpp"

#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

using rtpt_light::build_light_list;
using rtpt_light::kListOk;
using rtpt_light::kListTooLong;
using rtpt_light::kMaxLights;

template <class M>
static M material(float ke_r, float ke_g, float ke_b) {
  M m;
  std::memset(&m, 0, sizeof m);
  m.albedo[0] = m.albedo[1] = m.albedo[2] = 0.5f;
  m.emission[0] = ke_r, m.emission[1] = ke_g, m.emission[2] = ke_b;
  return m;
}

// the list by its definition, one posed triangle at a time
template <class M>
static std::vector<uint32_t> expected(const std::vector<uint32_t>& tm, const std::vector<M>& mats, uint32_t ni) {
  std::vector<uint32_t> out;
  const uint32_t nt = static_cast<uint32_t>(tm.size());
  for (uint64_t id = 0; id < static_cast<uint64_t>(ni) * nt; id++)
    if (rtpt_light::emissive(mats[tm[id % nt]])) out.push_back(static_cast<uint32_t>(id + 1));
  return out;
}

template <class M>
static void cases() {
  // materials: 0 dark, 1 a lamp, 2 a lamp in one channel only, 3 (the table's last) a lamp with a negative channel
  const std::vector<M> mats = {material<M>(0, 0, 0), material<M>(4, 3, 2), material<M>(0, 0, 1e-30f), material<M>(-1, 0, 0)};
  const uint32_t sentinel = 0xABCDu;
  for (uint32_t ni = 1; ni <= 3; ni++) {
    std::vector<uint32_t> out{sentinel};
    // no emitter
    std::vector<uint32_t> tm = {0, 0, 0, 0, 0};
    CHECK(build_light_list(tm.data(), mats.data(), 5u, ni, &out) == kListOk && out.empty());
    // every triangle an emitter
    tm = {1, 2, 3, 1, 2};
    CHECK(build_light_list(tm.data(), mats.data(), 5u, ni, &out) == kListOk);
    CHECK(out.size() == 5u * ni);
    for (uint32_t i = 0; i < out.size(); i++) CHECK(out[i] == i + 1);
    // an emitter as the last base triangle only: the list's last entry is the scene's last triangle, of the last instance
    tm = {0, 0, 0, 0, 3};  // ... with the material index n_materials - 1
    CHECK(build_light_list(tm.data(), mats.data(), 5u, ni, &out) == kListOk);
    CHECK(out.size() == ni && out.back() == 5u * ni);
    for (uint32_t i = 0; i < ni; i++) CHECK(out[i] == 5u * i + 5u);
    // mixed, against the definition; ascending
    tm = {0, 1, 0, 2, 0, 0, 3};
    CHECK(build_light_list(tm.data(), mats.data(), 7u, ni, &out) == kListOk);
    CHECK(out == expected(tm, mats, ni));
    for (size_t i = 1; i < out.size(); i++) CHECK(out[i - 1] < out[i]);
    // a single triangle
    tm = {1};
    CHECK(build_light_list(tm.data(), mats.data(), 1u, ni, &out) == kListOk && out.size() == ni && out[0] == 1u);
  }
  // -0.0f is zero: no emitter
  {
    const std::vector<M> z = {material<M>(-0.0f, 0.0f, -0.0f)};
    const std::vector<uint32_t> tm = {0, 0};
    std::vector<uint32_t> out{sentinel};
    CHECK(build_light_list(tm.data(), z.data(), 2u, 2u, &out) == kListOk && out.empty());
  }
  // the bound: one below, at, and one above 2^24 entries, from a table where one material emits (the input is a large index
  // array); a refused call leaves *out as it was
  {
    const std::vector<M> two = {material<M>(0, 0, 0), material<M>(1, 1, 1)};
    std::vector<uint32_t> tm(static_cast<size_t>(kMaxLights) + 2u, 1u);
    tm[0] = 0u;  // dark: entries start at id + 1 = 2
    std::vector<uint32_t> out{sentinel};
    CHECK(build_light_list(tm.data(), two.data(), kMaxLights, 1u, &out) == kListOk);  // 2^24 - 1 emitters
    CHECK(out.size() == kMaxLights - 1u && out.front() == 2u && out.back() == kMaxLights);
    CHECK(build_light_list(tm.data(), two.data(), kMaxLights + 1u, 1u, &out) == kListOk);  // 2^24
    CHECK(out.size() == kMaxLights && out.back() == kMaxLights + 1u);
    out.assign(1, sentinel);
    CHECK(build_light_list(tm.data(), two.data(), kMaxLights + 2u, 1u, &out) == kListTooLong);  // 2^24 + 1
    CHECK(out.size() == 1 && out[0] == sentinel);
    // ... and through the instance count: 2^23 emitters twice is the bound, three times is beyond it
    CHECK(build_light_list(tm.data() + 1, two.data(), kMaxLights / 2u, 2u, &out) == kListOk && out.size() == kMaxLights);
    CHECK(out.back() == kMaxLights);
    out.assign(1, sentinel);
    CHECK(build_light_list(tm.data() + 1, two.data(), kMaxLights / 2u, 3u, &out) == kListTooLong);
    CHECK(out.size() == 1 && out[0] == sentinel);
  }
}

int main() {
  cases<rtpt_material>();
  cases<rtpt_material_ext>();
  // the extended records: a specular or dielectric material's record carries no Ke, so it is no light whatever its emission says
  // (rtpt_scene_set_materials_ext refuses such a table; the list's rule is the record's)
  {
    std::vector<rtpt_material_ext> mats = {material<rtpt_material_ext>(1, 1, 1), material<rtpt_material_ext>(1, 1, 1),
                                           material<rtpt_material_ext>(1, 1, 1)};
    mats[1].flags = RTPT_MAT_SPECULAR;
    mats[2].flags = RTPT_MAT_DIELECTRIC;
    const std::vector<uint32_t> tm = {2, 1, 0, 1};
    std::vector<uint32_t> out;
    CHECK(build_light_list(tm.data(), mats.data(), 4u, 2u, &out) == kListOk);
    CHECK((out == std::vector<uint32_t>{3u, 7u}));
  }
  std::puts("light_list_host_check: ok");
  return 0;
}
