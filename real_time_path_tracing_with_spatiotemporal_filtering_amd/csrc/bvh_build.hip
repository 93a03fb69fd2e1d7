// bvh_build.hip — the tree of buildAccelerationStructure (main.cpp:687-742, a device build there, :723-741) built ON THE
// DEVICE: a linear BVH after Karras 2012 ("Maximizing parallelism in the construction of BVHs, octrees and k-d trees").
// Opt-in (RTPT_FLAG_DEVICE_BVH_BUILD); the default stays the host's 32-bin SAH builder (bvh.cpp).
//
// This file makes the TOPOLOGY only — child references, leaf order, the nodes sorted by height — in exactly the formats
// the host path uploads (bvh.hpp: BvhNodeQ, leaf reference = bit 31 | first << 2 | count - 1).  The boxes, the padding,
// the 16-bit grid and the leaf records are then filled by the same launch_refit + launch_scene_prepare a changed model
// matrix runs (refit.hip, kernels.hip): no second copy of the box arithmetic the traversal was proven against.  Boxes only
// cull and order (closest hit = min over (t, id) of one ray-triangle routine, D4), so ANY valid tree traces the same bits.
//
//   k_prim_centre   per primitive (one triangle, or one fan pair 2q, 2q + 1) the centre of its box; block min / max
//   k_centre_bounds one block over the partials: the bounds of the centres (two stages, no float atomics)
//   k_morton        63-bit Morton key (21 bits per axis, computed in binary64: total for any finite input)
//   rocprim sort    (key, primitive) — stable, so equal keys stay in primitive order; a tie is split by sorted position
//                   (Karras' augmented key): d duplicates cost log2(d) levels, not a chain
//   k_hierarchy     one thread per internal node: range, split, children, parent pointers
//   rocprim sort    the internal nodes by (first ascending, last descending): ranges nest, so the position in that order
//                   IS the pre-order rank — node 0 the root, every child behind its parent, every subtree contiguous
//   k_emit_nodes / k_emit_leaves   the renumbered child-pair nodes and the leaf order
//   k_heights       every leaf walks up; at each node the first arrival leaves its height IN the atomic exchange and
//                   stops, the second takes it from the return value and goes on.  Nothing waits, and no plain store of
//                   this launch is read by another workgroup of it (parents come from k_hierarchy's launch)
//   k_height_keys   height per (renumbered) node + the histogram of heights (LDS per block, then one atomic per bin)
//   rocprim sort    nodes by height (stable: ascending index within a height) = refit_order
// Every step is a function of its input alone (integer atomics only count or exchange), so the same triangles give the
// same node array whatever the dispatch order.
#include <algorithm>
#include <cstring>  // before rocprim: its texture_cache_iterator.hpp calls memset

#include <rocprim/rocprim.hpp>

#include "bvh_build_common.hpp"

namespace rt {
namespace {

constexpr uint32_t kMaxPartials = 1024;  // blocks of k_prim_centre (grid-stride beyond)

// block-wide min / max of 6 values per thread; result in s[0..5] of thread 0's view after the call
__device__ __forceinline__ void block_minmax(float v[6], float (*s)[6]) {
  const int t = threadIdx.x;
  for (int k = 0; k < 6; k++) s[t][k] = v[k];
  __syncthreads();
  for (int stride = kBlock / 2; stride > 0; stride >>= 1) {
    if (t < stride)
      for (int k = 0; k < 3; k++) {
        s[t][k] = __builtin_fminf(s[t][k], s[t + stride][k]);
        s[t][3 + k] = __builtin_fmaxf(s[t][3 + k], s[t + stride][3 + k]);
      }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBlock) void k_prim_centre(uint32_t n, uint32_t w, const float* __restrict__ tris, float* __restrict__ centre,
                                                        float* __restrict__ partial) {
  __shared__ float s[kBlock][6];
  float acc[6] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < n; p += gridDim.x * kBlock) {
    float mn[3], mx[3];
    prim_box(tris, p, w, mn, mx);
    for (int a = 0; a < 3; a++) {
      const float c = 0.5f * mn[a] + 0.5f * mx[a];  // halves first: finite for any finite box
      centre[3 * static_cast<size_t>(p) + a] = c;
      acc[a] = __builtin_fminf(acc[a], c);
      acc[3 + a] = __builtin_fmaxf(acc[3 + a], c);
    }
  }
  block_minmax(acc, s);
  if (threadIdx.x < 6) partial[6 * blockIdx.x + threadIdx.x] = s[0][threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void k_centre_bounds(uint32_t n_partials, const float* __restrict__ partial, float* __restrict__ bounds) {
  __shared__ float s[kBlock][6];
  float acc[6] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
  for (uint32_t b = threadIdx.x; b < n_partials; b += kBlock)
    for (int k = 0; k < 3; k++) {
      acc[k] = __builtin_fminf(acc[k], partial[6 * b + k]);
      acc[3 + k] = __builtin_fmaxf(acc[3 + k], partial[6 * b + 3 + k]);
    }
  block_minmax(acc, s);
  if (threadIdx.x < 6) bounds[threadIdx.x] = s[0][threadIdx.x];
}

__device__ __forceinline__ uint64_t spread3(uint32_t x) {  // 21 bits -> every third bit of 61
  uint64_t v = x & 0x1FFFFFu;
  v = (v | (v << 32)) & 0x001F00000000FFFFull;
  v = (v | (v << 16)) & 0x001F0000FF0000FFull;
  v = (v | (v << 8)) & 0x100F00F00F00F00Full;
  v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}

__global__ __launch_bounds__(kBlock) void k_morton(uint32_t n, const float* __restrict__ centre, const float* __restrict__ bounds,
                                                   uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  uint32_t q[3];
  for (int a = 0; a < 3; a++) {
    // binary64: the extent of two binary32 values and the quotient neither overflow nor lose the cell (extents of 1e-13
    // and of 1e13, coordinates near 1e5); a zero or inverted extent (one point, a flat axis, no finite centre) is cell 0
    const double lo = static_cast<double>(bounds[a]), ext = static_cast<double>(bounds[3 + a]) - lo;
    double x = ext > 0.0 ? (static_cast<double>(centre[3 * static_cast<size_t>(p) + a]) - lo) / ext * 2097152.0 : 0.0;
    if (!(x >= 0.0)) x = 0.0;  // also a NaN centre
    if (x > 2097151.0) x = 2097151.0;
    q[a] = static_cast<uint32_t>(x);
  }
  keys[p] = (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[2]);
  vals[p] = p;
}

// length of the common prefix of the augmented keys (key, sorted position) of leaves i and j; -1 outside the array
__device__ __forceinline__ int delta(const uint64_t* __restrict__ keys, int64_t n, int64_t i, int64_t j) {
  if (j < 0 || j >= n) return -1;
  if (i == j) return 96;
  const uint64_t x = keys[i] ^ keys[j];
  if (x) return __builtin_clzll(x);
  return 64 + __builtin_clz(static_cast<uint32_t>(i) ^ static_cast<uint32_t>(j));  // i != j
}

// n >= 2 leaves, n - 1 internal nodes; Karras' numbering (node i sits at one end of its range, node 0 is the root).
// A child reference here: kLeafBit | sorted position, or the internal node's Karras index.
__global__ __launch_bounds__(kBlock) void k_hierarchy(uint32_t n, const uint64_t* __restrict__ keys, uint32_t* __restrict__ kl,
                                                      uint32_t* __restrict__ kr, uint32_t* __restrict__ parent,
                                                      uint32_t* __restrict__ leaf_parent, uint32_t* __restrict__ slot,
                                                      uint64_t* __restrict__ range_key, uint32_t* __restrict__ range_val) {
  const uint32_t iu = blockIdx.x * kBlock + threadIdx.x;
  if (iu >= n - 1) return;
  const int64_t N = n, i = iu;
  const int64_t d = delta(keys, N, i, i + 1) > delta(keys, N, i, i - 1) ? 1 : -1;
  const int dmin = delta(keys, N, i, i - d);
  int64_t lmax = 2;
  while (delta(keys, N, i, i + lmax * d) > dmin) lmax *= 2;  // ends: delta is -1 outside the array
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (delta(keys, N, i, i + (l + t) * d) > dmin) l += t;
  const int64_t j = i + l * d;
  const int dnode = delta(keys, N, i, j);
  int64_t s = 0, t = l;
  do {
    t = (t + 1) / 2;
    if (delta(keys, N, i, i + (s + t) * d) > dnode) s += t;
  } while (t > 1);
  const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
  const int64_t first = i < j ? i : j, last = i < j ? j : i;
  const uint32_t g = static_cast<uint32_t>(gamma);
  if (first == gamma) {
    kl[iu] = kLeafBit | g;
    leaf_parent[g] = iu;
  } else {
    kl[iu] = g;
    parent[g] = iu;
  }
  if (last == gamma + 1) {
    kr[iu] = kLeafBit | (g + 1u);
    leaf_parent[g + 1u] = iu;
  } else {
    kr[iu] = g + 1u;
    parent[g + 1u] = iu;
  }
  if (iu == 0) parent[0] = kNone;
  slot[iu] = kNone;
  range_key[iu] = (static_cast<uint64_t>(first) << 32) | static_cast<uint64_t>(0xFFFFFFFFu - static_cast<uint32_t>(last));
  range_val[iu] = iu;
}

// A/B numbering (LbvhArgs::by_height): nodes numbered by DESCENDING height instead of pre-order — the cheapest order with
// every child behind its parent (a parent is strictly higher than its children; the root alone has the largest height, so
// it stays node 0), and what a builder without the pre-order sort would ship.  by_height[p] = pre-order index of the p-th
// node in ascending height.
__global__ __launch_bounds__(kBlock) void k_height_rank(uint32_t m, const uint32_t* __restrict__ by_height, uint32_t* __restrict__ renum) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p < m) renum[by_height[p]] = m - 1u - p;
}

__global__ __launch_bounds__(kBlock) void k_renumber(uint32_t m, const uint32_t* __restrict__ renum, const BvhNodeQ* __restrict__ src,
                                                     BvhNodeQ* __restrict__ dst, uint32_t* __restrict__ refit_order) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= m) return;
  BvhNodeQ nd = src[r];
  if (!(nd.lref & kLeafBit)) nd.lref = renum[nd.lref];
  if (!(nd.rref & kLeafBit)) nd.rref = renum[nd.rref];
  dst[renum[r]] = nd;
  refit_order[r] = m - 1u - r;  // ascending height = descending index
}

// one primitive: the root pair with one leaf and an absent child, as the host builder makes it
__global__ void k_single(uint32_t w, BvhNodeQ* __restrict__ nodes, uint32_t* __restrict__ leaf_order, uint32_t* __restrict__ refit_order,
                         uint32_t* __restrict__ header) {
  if (blockIdx.x || threadIdx.x) return;
  BvhNodeQ nd;
  for (int k = 0; k < 12; k++) nd.box[k] = 0;
  nd.lref = leaf_ref(0, w);
  nd.rref = kBvhEmpty;
  nodes[0] = nd;
  for (uint32_t k = 0; k < w; k++) leaf_order[k] = k;
  refit_order[0] = 0;
  header[0] = 0;
  header[1] = 1;
  header[2] = 1;
}

// the carve-up of the context's scratch area; offsets in bytes
struct Layout {
  size_t centre, partial, bounds, key_a, key_b, val_a, val_b, kl, kr, parent, leaf_parent, slot, height, rank, hkey, hval, nodes_tmp, sort_tmp, sort_tmp_bytes,
      total;
};

hipError_t make_layout(uint32_t n, bool by_height, Layout& L) {
  const size_t N = n;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += up256(bytes);
    return at;
  };
  L.centre = take(N * 12);
  L.partial = take(kMaxPartials * 6 * sizeof(float));
  L.bounds = take(6 * sizeof(float));
  L.key_a = take(N * 8);
  L.key_b = take(N * 8);
  L.val_a = take(N * 4);
  L.val_b = take(N * 4);
  L.kl = take(N * 4);
  L.kr = take(N * 4);
  L.parent = take(N * 4);
  L.leaf_parent = take(N * 4);
  L.slot = take(N * 4);
  L.height = take(N * 4);
  L.rank = take(N * 4);
  L.hkey = take(N * 4);
  L.hval = take(N * 4);
  L.nodes_tmp = take(by_height ? N * sizeof(BvhNodeQ) : 0);
  size_t t64 = 0, t32 = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, t64, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                           static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), N, 0, 64, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::radix_sort_pairs(nullptr, t32, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                static_cast<uint32_t*>(nullptr), N, 0, 7, nullptr);
  if (e != hipSuccess) return e;
  L.sort_tmp_bytes = t64 > t32 ? t64 : t32;
  L.sort_tmp = take(L.sort_tmp_bytes ? L.sort_tmp_bytes : 1);
  L.total = off;
  return hipSuccess;
}

}  // namespace

size_t lbvh_scratch_bytes(uint32_t n_prims, bool by_height) {
  Layout L;
  if (n_prims < 2) return 256;
  return make_layout(n_prims, by_height, L) == hipSuccess ? L.total : 0;
}

hipError_t launch_lbvh_build(const LbvhArgs& a, void* scratch, size_t scratch_bytes, hipStream_t s) {
  if (!a.n_prims || (a.prim_w != 1 && a.prim_w != 2) || !scratch) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.header, 0, kLbvhHeaderWords * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  if (a.n_prims == 1) {
    hipLaunchKernelGGL(k_single, dim3(1), dim3(64), 0, s, a.prim_w, a.nodes, a.leaf_order, a.refit_order, a.header);
    return hipGetLastError();
  }
  const uint32_t n = a.n_prims, m = n - 1;
  Layout L;
  if ((e = make_layout(n, a.by_height != 0, L)) != hipSuccess) return e;
  if (L.total > scratch_bytes) return hipErrorInvalidValue;
  char* base = static_cast<char*>(scratch);
  float* centre = reinterpret_cast<float*>(base + L.centre);
  float* partial = reinterpret_cast<float*>(base + L.partial);
  float* bounds = reinterpret_cast<float*>(base + L.bounds);
  uint64_t* key_a = reinterpret_cast<uint64_t*>(base + L.key_a);
  uint64_t* key_b = reinterpret_cast<uint64_t*>(base + L.key_b);
  uint32_t* val_a = reinterpret_cast<uint32_t*>(base + L.val_a);
  uint32_t* val_b = reinterpret_cast<uint32_t*>(base + L.val_b);
  uint32_t* kl = reinterpret_cast<uint32_t*>(base + L.kl);
  uint32_t* kr = reinterpret_cast<uint32_t*>(base + L.kr);
  uint32_t* parent = reinterpret_cast<uint32_t*>(base + L.parent);
  uint32_t* leaf_parent = reinterpret_cast<uint32_t*>(base + L.leaf_parent);
  uint32_t* slot = reinterpret_cast<uint32_t*>(base + L.slot);
  uint32_t* height = reinterpret_cast<uint32_t*>(base + L.height);
  uint32_t* rank = reinterpret_cast<uint32_t*>(base + L.rank);
  uint32_t* hkey = reinterpret_cast<uint32_t*>(base + L.hkey);
  uint32_t* hval = reinterpret_cast<uint32_t*>(base + L.hval);
  void* tmp = base + L.sort_tmp;
  size_t tmp_bytes = L.sort_tmp_bytes;

  const uint32_t n_partials = std::min<uint32_t>(kMaxPartials, (n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(k_prim_centre, dim3(n_partials), dim3(kBlock), 0, s, n, a.prim_w, a.tris, centre, partial);
  hipLaunchKernelGGL(k_centre_bounds, dim3(1), dim3(kBlock), 0, s, n_partials, partial, bounds);
  hipLaunchKernelGGL(k_morton, grid_for(n), dim3(kBlock), 0, s, n, centre, bounds, key_a, val_a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // sorted keys in key_b, the primitive at each sorted position in val_b
  if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, key_a, key_b, val_a, val_b, static_cast<size_t>(n), 0, 64, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_emit_leaves, grid_for(n), dim3(kBlock), 0, s, n, a.prim_w, val_b, a.leaf_order);
  // key_a / val_a are free again: the internal nodes' (first, ~last) keys
  hipLaunchKernelGGL(k_hierarchy, grid_for(m), dim3(kBlock), 0, s, n, key_b, kl, kr, parent, leaf_parent, slot, key_a, val_a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // pre-order: order[rank] = Karras index, in val_b (the sorted primitives are consumed); the sorted range keys overwrite key_b
  // only after k_hierarchy has read the Morton keys (stream order)
  uint32_t* order = val_b;
  tmp_bytes = L.sort_tmp_bytes;
  if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, key_a, key_b, val_a, order, static_cast<size_t>(m), 0, 64, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_rank, grid_for(m), dim3(kBlock), 0, s, m, order, rank);
  hipLaunchKernelGGL(k_emit_nodes, grid_for(m), dim3(kBlock), 0, s, m, a.prim_w, 0u, order, rank, kl, kr, a.nodes, a.header);
  hipLaunchKernelGGL(k_heights, grid_for(n), dim3(kBlock), 0, s, n, leaf_parent, parent, slot, height, a.header);
  hipLaunchKernelGGL(k_height_keys, grid_for(m), dim3(kBlock), 0, s, m, order, height, hkey, hval, a.header);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tmp_bytes = L.sort_tmp_bytes;
  // sorted heights land in val_a (scratch); the nodes by height in refit_order
  if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, hkey, val_a, hval, a.refit_order, static_cast<size_t>(m), 0, 7, s)) != hipSuccess) return e;
  if (a.by_height) {
    BvhNodeQ* nodes_tmp = reinterpret_cast<BvhNodeQ*>(base + L.nodes_tmp);
    uint32_t* renum = rank;  // the pre-order ranks are consumed
    if ((e = hipMemcpyAsync(nodes_tmp, a.nodes, static_cast<size_t>(m) * sizeof(BvhNodeQ), hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_height_rank, grid_for(m), dim3(kBlock), 0, s, m, a.refit_order, renum);
    hipLaunchKernelGGL(k_renumber, grid_for(m), dim3(kBlock), 0, s, m, renum, nodes_tmp, a.nodes, a.refit_order);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace rt
