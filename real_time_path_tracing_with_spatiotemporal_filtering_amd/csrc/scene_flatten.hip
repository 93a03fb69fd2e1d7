// scene_flatten.hip — mesh x instance transforms -> the un-posed triangle soup, on the device (buildAccelerationStructure's
// instance records, main.cpp:728-741), and the fan-pair test over that soup.  What rtpt_scene_upload does on one CPU
// thread for RTPT_FLAG_DEVICE_FLATTEN scenes, and the first step of rtpt_scene_set_instances (then k_pose, the refit and
// the leaf records follow on the same stream: refit.hip, kernels.hip).
//   k_flatten     one thread per output vertex: xf[instance] * xyz[idx[3 t + k]] in the host's arithmetic (api_scene.hip:
//                 host_flatten), so the bits are the host's; without transforms a copy
//   k_fan_pairs   one thread per pair (2q, 2q + 1): v0 of both and v2 of the first against v1 of the second, compared as
//                 integers like the host's memcmp (-0 != +0, equal NaN bits are equal).  The result word is preset to 1;
//                 every lane that finds a mismatch stores 0 — all writers write the same value, no atomics
#include "device_common.hpp"

namespace rt {
namespace {

__global__ void k_flatten(FlattenArgs a) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= a.n_out_verts) return;
  const uint32_t per_inst = 3 * a.n_tris;
  const uint32_t inst = v / per_inst, k = v - inst * per_inst;
  const float* p = a.xyz + 3 * static_cast<size_t>(a.idx[k]);
  const float x = p[0], y = p[1], z = p[2];
  float w[3] = {x, y, z};
  if (a.xf) {
    const float* m = a.xf + 12 * static_cast<size_t>(inst);
    for (int r = 0; r < 3; r++) w[r] = fmaf_(m[4 * r + 2], z, fmaf_(m[4 * r + 1], y, m[4 * r] * x)) + m[4 * r + 3];
  }
  float* o = a.out + 3 * static_cast<size_t>(v);  // stored last: nothing is loaded behind a store that might alias it
  o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
}

__global__ void k_fan_pairs(uint32_t n_pairs, const uint32_t* __restrict__ tris, uint32_t* __restrict__ all_paired) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_pairs) return;
  const uint32_t* ta = tris + 18 * static_cast<size_t>(q);
  const uint32_t* tb = ta + 9;
  uint32_t diff = 0;  // all twelve words loaded, no branch between them
  for (int j = 0; j < 3; j++) diff |= (ta[j] ^ tb[j]) | (ta[6 + j] ^ tb[3 + j]);
  if (diff) *all_paired = 0u;
}

}  // namespace

void launch_flatten(const FlattenArgs& a, hipStream_t s) {
  if (!a.n_out_verts) return;
  hipLaunchKernelGGL(k_flatten, dim3((a.n_out_verts + 255) / 256), dim3(256), 0, s, a);
}

void launch_fan_pairs(uint32_t n_pairs, const float* tris, uint32_t* all_paired, hipStream_t s) {
  if (!n_pairs) return;
  hipLaunchKernelGGL(k_fan_pairs, dim3((n_pairs + 255) / 256), dim3(256), 0, s, n_pairs, reinterpret_cast<const uint32_t*>(tris), all_paired);
}

}  // namespace rt
