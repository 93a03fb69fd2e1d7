// bvh_build_common.hpp — what the two device tree builders (bvh_build.hip: Karras LBVH, bvh_build_sah.hip: the host's
// binned SAH restated level by level) share: the box of a primitive, the renumbering of nodes from their sorted ranges
// (ranges nest, so the position in the order (first ascending, last descending) IS the pre-order rank), the heights by
// leaves walking up, the height histogram.  Kernels live in an anonymous namespace like every kernel of this library.
#pragma once

#include "bvh.hpp"
#include "device_common.hpp"

namespace rt {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr int kBlock = 256;

__device__ __forceinline__ void prim_box(const float* __restrict__ tris, uint32_t p, uint32_t w, float mn[3], float mx[3]) {
  for (int a = 0; a < 3; a++) {
    mn[a] = 3.402823466e+38f;
    mx[a] = -3.402823466e+38f;
  }
  const float* t = tris + 9 * static_cast<size_t>(p) * w;
  for (uint32_t v = 0; v < 3 * w; v++)
    for (int a = 0; a < 3; a++) {
      mn[a] = __builtin_fminf(mn[a], t[3 * v + a]);
      mx[a] = __builtin_fmaxf(mx[a], t[3 * v + a]);
    }
}

__global__ __launch_bounds__(kBlock) void k_rank(uint32_t m, const uint32_t* __restrict__ order, uint32_t* __restrict__ rank) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r < m) rank[order[r]] = r;
}

__device__ __forceinline__ uint32_t leaf_ref(uint32_t sorted_pos, uint32_t w) { return kLeafBit | ((sorted_pos * w) << 2) | (w - 1u); }

// a leaf child in kl / kr: kLeafBit | sorted position (one primitive: the LBVH), or with final_leaf_refs the finished
// reference (the SAH builder's leaves hold one or two primitives)
__global__ __launch_bounds__(kBlock) void k_emit_nodes(uint32_t m, uint32_t w, uint32_t final_leaf_refs, const uint32_t* __restrict__ order, const uint32_t* __restrict__ rank,
                                                       const uint32_t* __restrict__ kl, const uint32_t* __restrict__ kr,
                                                       BvhNodeQ* __restrict__ nodes, uint32_t* __restrict__ header) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= m) return;
  const uint32_t i = order[r];
  BvhNodeQ nd;
  for (int k = 0; k < 12; k++) nd.box[k] = 0;
  const uint32_t a = kl[i], b = kr[i];
  nd.lref = (a & kLeafBit) ? (final_leaf_refs ? a : leaf_ref(a & ~kLeafBit, w)) : rank[a];
  nd.rref = (b & kLeafBit) ? (final_leaf_refs ? b : leaf_ref(b & ~kLeafBit, w)) : rank[b];
  nodes[r] = nd;
  if (r == 0) header[1] = m;
}

__global__ __launch_bounds__(kBlock) void k_emit_leaves(uint32_t n, uint32_t w, const uint32_t* __restrict__ sorted_prim, uint32_t* __restrict__ leaf_order) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t p = sorted_prim[j];
  for (uint32_t k = 0; k < w; k++) leaf_order[static_cast<size_t>(j) * w + k] = p * w + k;
}

// height of a node = 0 when both children are leaves, else 1 + the higher interior child.  `slot` holds kNone before the
// first arrival; what arrives is (height of the child's subtree + 1), a leaf arriving with 0.
__global__ __launch_bounds__(kBlock) void k_heights(uint32_t n, const uint32_t* __restrict__ leaf_parent, const uint32_t* __restrict__ parent,
                                                    uint32_t* __restrict__ slot, uint32_t* __restrict__ height, uint32_t* __restrict__ header) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  uint32_t cur = leaf_parent[j], mine = 0;
  if (cur == kNone) return;  // the SAH builder indexes leaves by their first slot: not every slot starts one
  for (uint32_t step = 0; step < n; step++) {  // a path has fewer than n nodes
    const uint32_t other = atomicExch(&slot[cur], mine);
    if (other == kNone) return;  // first of the two: the sibling carries the height on
    const uint32_t h = other > mine ? other : mine;
    height[cur] = h;
    const uint32_t up = parent[cur];
    if (up == kNone) {
      header[0] = h + 1u;  // depth as the host builder counts it: the deepest leaf's level, the root pair's children at 1
      return;
    }
    mine = h + 1u;
    cur = up;
  }
}

__global__ __launch_bounds__(kBlock) void k_height_keys(uint32_t m, const uint32_t* __restrict__ order, const uint32_t* __restrict__ height,
                                                        uint32_t* __restrict__ hkey, uint32_t* __restrict__ hval, uint32_t* __restrict__ header) {
  __shared__ uint32_t hist[kLbvhMaxLevels];
  for (uint32_t b = threadIdx.x; b < kLbvhMaxLevels; b += kBlock) hist[b] = 0;
  __syncthreads();
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r < m) {
    uint32_t h = height[order[r]];
    if (h > kLbvhMaxLevels - 1u) h = kLbvhMaxLevels - 1u;  // 63 + 32 key bits: cannot happen; such a tree is refused for its depth anyway
    hkey[r] = h;
    hval[r] = r;
    atomicAdd(&hist[h], 1u);
  }
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kLbvhMaxLevels; b += kBlock)
    if (hist[b]) atomicAdd(&header[2 + b], hist[b]);
}

inline size_t up256(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }

inline dim3 grid_for(uint32_t n) { return dim3((n + kBlock - 1) / kBlock); }

}  // namespace
}  // namespace rt
