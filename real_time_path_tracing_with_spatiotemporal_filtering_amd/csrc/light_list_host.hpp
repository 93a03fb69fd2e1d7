// light_list_host.hpp — the light list of next-event estimation (RTPT_FLAG_EXT_NEE; light_sample.hpp states the estimator), built
// on the host beside the material records by rtpt_scene_set_materials and rtpt_scene_set_materials_ext.  Free of HIP, like
// material_host.hpp, so that a plain C++ program can exercise it under a sanitizer (csrc/tests/light_list_host_check.cpp).
//
// The list holds, ascending, id + 1 (the convention of HitRec::id1) of every POSED triangle id = inst * n_base_tris + t whose base
// triangle t has an emissive material: Ke != 0 in a record that is neither specular nor dielectric — the rule that sets the
// record's m1.w (material_host.hpp: pack_records_mode; rtpt_scene_set_materials).  An entry is a posed id: the kernels read its
// vertices from shade record id and its Ke from material record id % n_base_tris.
#pragma once

#include <cstdint>
#include <new>
#include <vector>

#include "../../include/rtpt.h"

namespace rtpt_light {

constexpr uint32_t kMaxLights = 1u << 24;  // light::kMaxLights (light_sample.hpp): the pick's draw has 24 bits

inline bool emissive(const rtpt_material& m) { return m.emission[0] != 0.0f || m.emission[1] != 0.0f || m.emission[2] != 0.0f; }
inline bool emissive(const rtpt_material_ext& m) {
  if (m.flags & (RTPT_MAT_SPECULAR | RTPT_MAT_DIELECTRIC)) return false;  // their records carry no Ke
  return m.emission[0] != 0.0f || m.emission[1] != 0.0f || m.emission[2] != 0.0f;
}

enum { kListOk = 0, kListTooLong = 1, kListNoMem = 2 };

// tri_material: n_base_tris indices into `materials`, every one in range (the callers checked them); n_instances >= 1, and
// n_instances * n_base_tris + 1 fits 32 bits (rtpt_scene_upload's bound).  *out is written only when the result is kListOk; a list
// of more than kMaxLights entries is kListTooLong.
template <class M>
inline int build_light_list(const uint32_t* tri_material, const M* materials, uint32_t n_base_tris, uint32_t n_instances,
                            std::vector<uint32_t>* out) {
  uint64_t per_instance = 0;
  for (uint32_t t = 0; t < n_base_tris; t++)
    if (emissive(materials[tri_material[t]])) per_instance++;
  const uint64_t count = per_instance * n_instances;
  if (count > kMaxLights) return kListTooLong;
  std::vector<uint32_t> list;
  try {
    list.reserve(static_cast<size_t>(count));
  } catch (const std::bad_alloc&) {
    return kListNoMem;
  }
  for (uint32_t inst = 0; inst < n_instances; inst++)
    for (uint32_t t = 0; t < n_base_tris; t++)
      if (emissive(materials[tri_material[t]]))
        list.push_back(static_cast<uint32_t>(static_cast<uint64_t>(inst) * n_base_tris + t + 1u));
  out->swap(list);
  return kListOk;
}

// THE SEARCH (RTPT_FLAG_EXT_NEE_MIS; light_sample.hpp: the bounce's weight at an emitter it hit): the index of id1 in the ascending
// list ids[0, n), or n where the list does not hold it.  Stated once, here, for the device (the tracing kernels, through
// light_sample.hpp, and rtpt_selftest_light_find) and for a plain C++ program under a sanitizer (csrc/tests/
// light_find_host_check.cpp).  Every index read lies in [0, n) whatever ids and id1 hold: lo <= mid < hi <= n inside the loop, and
// the read behind it is guarded by lo < n.  On a list that is not ascending the answer is some index whose entry is id1, or n.
#if defined(__HIPCC__)
#define RTPT_LIGHT_HD __host__ __device__
#else
#define RTPT_LIGHT_HD
#endif
RTPT_LIGHT_HD inline uint32_t find(const uint32_t* ids, uint32_t n, uint32_t id1) {
  uint32_t lo = 0u, hi = n;  // the first entry >= id1 lies in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (ids[mid] < id1)
      lo = mid + 1u;
    else
      hi = mid;
  }
  return (lo < n && ids[lo] == id1) ? lo : n;
}

}  // namespace rtpt_light
