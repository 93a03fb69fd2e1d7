// normal_host.hpp — the host side of smooth shading (rtpt_scene_set_normals), free of HIP so that a plain C++ program can exercise it
// under a sanitizer (csrc/tests/normal_host_check.cpp): the checks the call applies before anything reaches the device, and the
// record packing.  The rules and the cofactor function are shading_normal.hpp's; the `vn` reader is obj_host.hpp's.
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/rtpt.h"

namespace rtpt_nrm {

constexpr uint32_t kRecordFloats = 12;  // NormalView::records: three float4 per base triangle

// Everything rtpt_scene_set_normals refuses, decided on arguments alone (the values of the normals are never a reason: NaN, zero and
// any length are the rules' business).  NULL: the arguments are fine.  Not for the removing call (tri_normals NULL, n_tris 0).
inline const char* check_normals(const float* tri_normals, uint32_t n_tris, uint32_t n_base_tris, uint32_t ctx_flags) {
  if (ctx_flags & RTPT_FLAG_NO_PATH_COMPACTION) return "a context with RTPT_FLAG_NO_PATH_COMPACTION has no kernels that shade with vertex normals";
  if (!tri_normals) return "tri_normals is NULL (with n_tris 0 the call removes the normals)";
  if (n_tris != n_base_tris) return "nine floats per triangle of the uploaded mesh";
  return nullptr;
}

// n_tris records of 12 floats: (n0.xyz, smooth as bits) (n1.xyz, 0) (n2.xyz, 0); smooth is 1 where tri_smooth is NULL or non-zero.
// The normals are copied bit for bit.
inline void pack_records(const float* tri_normals, const uint32_t* tri_smooth, uint32_t n_tris, float* rec) {
  for (uint32_t t = 0; t < n_tris; t++) {
    const float* n = tri_normals + 9 * static_cast<size_t>(t);
    float* r = rec + kRecordFloats * static_cast<size_t>(t);
    const uint32_t smooth = (!tri_smooth || tri_smooth[t]) ? 1u : 0u;
    for (int k = 0; k < 3; k++) {
      std::memcpy(r + 4 * k, n + 3 * k, 3 * sizeof(float));
      const uint32_t w = k == 0 ? smooth : 0u;
      std::memcpy(r + 4 * k + 3, &w, sizeof w);
    }
  }
}

}  // namespace rtpt_nrm
