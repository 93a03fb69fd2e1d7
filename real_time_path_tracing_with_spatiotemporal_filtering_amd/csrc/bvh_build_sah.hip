// bvh_build_sah.hip — the HOST builder's tree (bvh.cpp: Builder::build, 32-bin SAH, object median past the depth budget)
// built ON THE DEVICE, node for node.  Opt-in: RTPT_FLAG_DEVICE_BVH_SAH together with RTPT_FLAG_DEVICE_BVH_BUILD.
//
// Builder::build decides everything from quantities that do not depend on the order of the primitives: min / max of boxes
// and integer counts per bin, a cost scan in a fixed (axis, bin) order, a median by the total order (centre, id).  So the
// hierarchy is a function of the triangle SET, and a level-synchronous restatement that evaluates the same binary32
// expressions in the same operation order (this library is compiled with -ffp-contract=off) reproduces it exactly:
// the same child references in the same pre-order numbering, the same leaf order up to the order of the two triangles
// inside a two-triangle leaf (std::partition is not stable; only the sets on either side of a split matter).
//
// Like bvh_build.hip this file makes the TOPOLOGY only; launch_refit + launch_scene_prepare fill boxes, grid and records.
//
// State: a permutation `perm` of the primitives and, per level, two tables of segments [lo, hi) of it (with the temporary
// index of the parent node and the side): SMALL segments (up to kSmall primitives) and LARGE ones.
//   k_sah_prims     per primitive its box and the centre 0.5f * (mn + mx), the host's expression
//   k_sah_small     one workgroup per small segment, everything in LDS: centroid and box bounds, 3 x 32 bins of (box, count)
//                   through integer min / max / add on an order-preserving encoding of binary32, the cost scan (one thread
//                   per axis, the host's loop as written), the leaf decision, a stable partition by bin <= split (block
//                   scan), or the median by rank counting; then the node and its two children are emitted
//   large segments  the host cuts them into chunks of kSmall positions (it reads their table back, a few hundred entries at
//                   most) and the same steps run as separate launches over the chunks: k_large_bounds and k_large_bin
//                   privatise in LDS and flush ONCE per workgroup with global integer atomics (no per-primitive global
//                   atomic anywhere), k_large_split scans the cost per segment, k_large_count / k_large_scan /
//                   k_large_scatter are the stable partition across chunks.  A large segment on the median path (depth >= 22
//                   or no SAH split, e.g. thousands of duplicates) goes through two radix sorts: by (ordered centre, id),
//                   then stably by segment
//   emit            a node's temporary index is mid - 1 (every boundary between two slots is the split of at most one node);
//                   its range key (first ascending, last descending) is sorted at the end: the position in that order is the
//                   pre-order rank, which is the order in which the host allocates nodes.  Heights and the height sort are
//                   the LBVH's (bvh_build_common.hpp)
// Host synchronisation: one readback of a few words per level (the sizes of the next level's tables, plus the large
// table while there are large segments) — the calls that build block anyway.  Integer atomics only take min / max, add
// counts or hand out table slots; the ORDER of a table changes nothing that is written to the tree, so the same triangles
// give the same arrays whatever the dispatch order.  Finite input only, like the LBVH.
#include <algorithm>
#include <cstring>  // before rocprim: its texture_cache_iterator.hpp calls memset
#include <vector>

#include <rocprim/rocprim.hpp>

#include "bvh_build_common.hpp"

namespace rt {
namespace {

constexpr int kBins = kBvhBins;
constexpr int kPer = 4;                        // primitives per thread
constexpr uint32_t kSmall = kBlock * kPer;     // a segment up to this size is handled whole by one workgroup
constexpr int kBinWords = 7;                   // box min xyz, box max xyz (encoded), triangle count
constexpr int kAxisWords = kBins * kBinWords;  // 224
constexpr int kSegBinWords = 3 * kAxisWords;   // 672 words = 2,688 bytes
constexpr float kFltMax = 3.402823466e+38f;

struct Seg {
  uint32_t lo, hi;  // positions of perm
  uint32_t parent;  // temporary index of the parent node (kNone: the root)
  uint32_t side;    // 0 left, 1 right
};

struct Chunk {
  uint32_t seg;     // index into this level's large table
  uint32_t lo, hi;  // positions, inside that segment
  uint32_t first;   // index of that segment's first chunk in the list (its chunks follow each other)
};

struct LargeState {
  uint32_t bounds[12];  // encoded: centre min xyz, centre max xyz, box min xyz, box max xyz
  int32_t axis, split;
  uint32_t median, nleft;
  uint32_t bins[kSegBinWords];
};
constexpr uint32_t kLargeWords = sizeof(LargeState) / 4;

// counters: [2 p] small segments of table p, [2 p + 1] large ones, [4] a large segment of this level takes the median path,
// [5] nodes so far
constexpr uint32_t kCtrWords = 8;

struct SahArgs {
  uint32_t n, w;
  const float* tris;
  float* pbox;  // n x 6
  float* pcen;  // n x 3
  uint32_t *perm, *perm_alt;
  uint32_t *kl, *kr, *parent, *leaf_parent;
  uint64_t* range_key;
  uint32_t* range_val;
  Seg* small[2];
  Seg* large[2];
  LargeState* lstate;
  Chunk* chunks;
  uint32_t *chunk_left, *chunk_off;
  uint32_t* ctr;
};

// order-preserving map of binary32 onto unsigned integers (finite values; -0 sorts below +0, which no decision sees)
__device__ __forceinline__ uint32_t enc(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec(uint32_t e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7FFFFFFFu) : ~e); }

struct Box3 {
  float mn[3], mx[3];
};
__device__ __forceinline__ void box_reset(Box3& b) {
  for (int a = 0; a < 3; a++) {
    b.mn[a] = kFltMax;
    b.mx[a] = -kFltMax;
  }
}
// Box::half_area of bvh.cpp, operation for operation
__device__ __forceinline__ float half_area(const Box3& b) {
  const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
  if (dx < 0.f) return 0.f;
  return dx * dy + dy * dz + dz * dx;
}

// the host's bin: min(kBins - 1, int((c - mn) * scale)), clamped at 0 as well (the product is never negative for a
// centre inside its bounds; where the host's conversion is undefined — an infinite or NaN product — this is bin 31 or 0).
// The float is tested before it is converted, so no conversion here is out of int's range.
__device__ __forceinline__ int bin_of(float c, float mn, float scale) {
  const float x = (c - mn) * scale;
  return !(x >= 0.f) ? 0 : (x >= static_cast<float>(kBins) ? kBins - 1 : static_cast<int>(x));
}

// one axis of the host's cost scan over finished bins: the first minimum in bin order (strict <); split -1: no candidate
__device__ void axis_best(const uint32_t* bins, float& best_cost, int& best_split) {
  float right_area[kBins];
  uint32_t right_cnt[kBins];
  Box3 acc;
  box_reset(acc);
  uint32_t c = 0;
  for (int b = kBins - 1; b > 0; b--) {
    for (int a = 0; a < 3; a++) {
      acc.mn[a] = __builtin_fminf(acc.mn[a], dec(bins[b * kBinWords + a]));
      acc.mx[a] = __builtin_fmaxf(acc.mx[a], dec(bins[b * kBinWords + 3 + a]));
    }
    c += bins[b * kBinWords + 6];
    right_area[b] = half_area(acc);
    right_cnt[b] = c;
  }
  box_reset(acc);
  c = 0;
  best_cost = kFltMax;
  best_split = -1;
  for (int b = 0; b < kBins - 1; b++) {
    for (int a = 0; a < 3; a++) {
      acc.mn[a] = __builtin_fminf(acc.mn[a], dec(bins[b * kBinWords + a]));
      acc.mx[a] = __builtin_fmaxf(acc.mx[a], dec(bins[b * kBinWords + 3 + a]));
    }
    c += bins[b * kBinWords + 6];
    if (c == 0 || right_cnt[b + 1] == 0) continue;
    const float cost = half_area(acc) * static_cast<float>(c) + right_area[b + 1] * static_cast<float>(right_cnt[b + 1]);
    if (cost < best_cost) {
      best_cost = cost;
      best_split = b;
    }
  }
}

__device__ __forceinline__ uint32_t bin_init_word(uint32_t j) {
  const uint32_t k = j % kBinWords;
  return k < 3 ? enc(kFltMax) : (k < 6 ? enc(-kFltMax) : 0u);
}
__device__ __forceinline__ uint32_t bound_init_word(uint32_t j) { return (j % 6) < 3 ? enc(kFltMax) : enc(-kFltMax); }

// exclusive scan of one value per thread over the workgroup; every thread calls it
__device__ uint32_t block_excl_scan(uint32_t v, uint32_t* s, uint32_t& total) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int d = 1; d < kBlock; d <<= 1) {
    const uint32_t x = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  total = s[kBlock - 1];
  const uint32_t r = s[t] - v;
  __syncthreads();
  return r;
}

// up to kPer primitives of thread t: positions base + kPer t + k < end
struct Mine {
  uint32_t p[kPer];
  float c[kPer][3];
  Box3 box[kPer];
  bool valid[kPer];
};
__device__ __forceinline__ void load_mine(const SahArgs& A, uint32_t base, uint32_t end, Mine& m) {
  for (int k = 0; k < kPer; k++) {
    const uint32_t i = base + kPer * threadIdx.x + k;
    m.valid[k] = i < end;
    m.p[k] = 0;
    if (!m.valid[k]) continue;
    const uint32_t p = A.perm[i];
    m.p[k] = p;
    for (int a = 0; a < 3; a++) {
      m.c[k][a] = A.pcen[3 * static_cast<size_t>(p) + a];
      m.box[k].mn[a] = A.pbox[6 * static_cast<size_t>(p) + a];
      m.box[k].mx[a] = A.pbox[6 * static_cast<size_t>(p) + 3 + a];
    }
  }
}
__device__ __forceinline__ void bounds_to_lds(const Mine& m, uint32_t* s_bounds) {
  for (int k = 0; k < kPer; k++) {
    if (!m.valid[k]) continue;
    for (int a = 0; a < 3; a++) {
      atomicMin(&s_bounds[a], enc(m.c[k][a]));
      atomicMax(&s_bounds[3 + a], enc(m.c[k][a]));
      atomicMin(&s_bounds[6 + a], enc(m.box[k].mn[a]));
      atomicMax(&s_bounds[9 + a], enc(m.box[k].mx[a]));
    }
  }
}
// bins of every axis with a positive centroid extent, as the host fills them (counts in triangles)
__device__ __forceinline__ void bins_to_lds(const Mine& m, const float cmn[3], const float cmx[3], uint32_t w, uint32_t* s_bins) {
  for (int a = 0; a < 3; a++) {
    const float ext = cmx[a] - cmn[a];
    if (!(ext > 0.f)) continue;
    const float scale = kBins / ext;
    for (int k = 0; k < kPer; k++) {
      if (!m.valid[k]) continue;
      uint32_t* bin = s_bins + a * kAxisWords + bin_of(m.c[k][a], cmn[a], scale) * kBinWords;
      for (int x = 0; x < 3; x++) {
        atomicMin(&bin[x], enc(m.box[k].mn[x]));
        atomicMax(&bin[3 + x], enc(m.box[k].mx[x]));
      }
      atomicAdd(&bin[6], w);
    }
  }
}

__device__ __forceinline__ void emit_leaf(const SahArgs& A, uint32_t lo, uint32_t cnt, uint32_t parent, uint32_t side) {
  (side ? A.kr : A.kl)[parent] = kLeafBit | ((lo * A.w) << 2) | (cnt * A.w - 1u);
  A.leaf_parent[lo] = parent;
}

// the node over seg split at mid, and its children: leaves by size at once, segments of the next level (table np) otherwise
__device__ void emit_split(const SahArgs& A, const Seg& seg, uint32_t mid, uint32_t np) {
  const uint32_t id = mid - 1u;
  if (seg.parent != kNone) (seg.side ? A.kr : A.kl)[seg.parent] = id;
  A.parent[id] = seg.parent;
  A.range_key[id] = (static_cast<uint64_t>(seg.lo) << 32) | static_cast<uint64_t>(0xFFFFFFFFu - (seg.hi - 1u));
  atomicAdd(&A.ctr[5], 1u);
  for (uint32_t side = 0; side < 2; side++) {
    Seg c;
    c.lo = side ? mid : seg.lo;
    c.hi = side ? seg.hi : mid;
    c.parent = id;
    c.side = side;
    const uint32_t cnt = c.hi - c.lo;
    if (cnt == 1 || cnt * A.w <= static_cast<uint32_t>(kBvhMinLeaf)) {
      emit_leaf(A, c.lo, cnt, id, side);
    } else if (cnt > kSmall) {
      A.large[np][atomicAdd(&A.ctr[2 * np + 1], 1u)] = c;
    } else {
      A.small[np][atomicAdd(&A.ctr[2 * np], 1u)] = c;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_sah_prims(SahArgs A) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= A.n) return;
  float mn[3], mx[3];
  prim_box(A.tris, p, A.w, mn, mx);
  for (int a = 0; a < 3; a++) {
    A.pbox[6 * static_cast<size_t>(p) + a] = mn[a];
    A.pbox[6 * static_cast<size_t>(p) + 3 + a] = mx[a];
    A.pcen[3 * static_cast<size_t>(p) + a] = 0.5f * (mn[a] + mx[a]);
  }
  A.perm[p] = p;
  A.range_val[p] = p;
}

// the key of the median's total order (centre, id): -0 and +0 compare equal on the host, so they share one encoding
__device__ __forceinline__ uint64_t median_key(float c, uint32_t p) {
  return (static_cast<uint64_t>(enc(c == 0.f ? 0.f : c)) << 32) | p;
}

__device__ __forceinline__ int widest_axis(const float cmn[3], const float cmx[3]) {
  int axis = 0;
  float best = -1.f;
  for (int a = 0; a < 3; a++) {
    const float e = cmx[a] - cmn[a];
    if (e > best) {
      best = e;
      axis = a;
    }
  }
  return axis;
}

__global__ __launch_bounds__(kBlock) void k_sah_small(SahArgs A, uint32_t parity, uint32_t depth) {
  __shared__ uint32_t s_bounds[12];
  __shared__ uint32_t s_bins[kSegBinWords];
  __shared__ uint32_t s_scan[kBlock];
  __shared__ uint64_t s_keys[kSmall];
  __shared__ float s_cost[3];
  __shared__ int s_split[3];
  const int t = threadIdx.x;
  const Seg seg = A.small[parity][blockIdx.x];
  const uint32_t lo = seg.lo, hi = seg.hi, cnt = hi - lo, n = cnt * A.w;
  Mine m;
  load_mine(A, lo, hi, m);
  if (t < 12) s_bounds[t] = bound_init_word(t);
  for (uint32_t j = t; j < static_cast<uint32_t>(kSegBinWords); j += kBlock) s_bins[j] = bin_init_word(j);
  __syncthreads();
  bounds_to_lds(m, s_bounds);
  __syncthreads();
  float cmn[3], cmx[3];
  Box3 bb;
  for (int a = 0; a < 3; a++) {
    cmn[a] = dec(s_bounds[a]);
    cmx[a] = dec(s_bounds[3 + a]);
    bb.mn[a] = dec(s_bounds[6 + a]);
    bb.mx[a] = dec(s_bounds[9 + a]);
  }
  const bool may_leaf = n <= static_cast<uint32_t>(kBvhMaxLeaf);
  const bool median = static_cast<int>(depth) >= kBvhMaxDepth - 26;
  // every condition below is computed by every thread from the same LDS words: the branches are uniform
  if (median && may_leaf) {
    if (t == 0) emit_leaf(A, lo, cnt, seg.parent, seg.side);
    return;
  }
  uint32_t mid = lo;
  if (!median) {
    bins_to_lds(m, cmn, cmx, A.w, s_bins);
    __syncthreads();
    if (t < 3) {
      s_cost[t] = kFltMax;
      s_split[t] = -1;
      if (cmx[t] - cmn[t] > 0.f) axis_best(s_bins + t * kAxisWords, s_cost[t], s_split[t]);
    }
    __syncthreads();
    float best_cost = kFltMax;
    int best_axis = -1, best_split = -1;
    for (int a = 0; a < 3; a++)
      if (s_split[a] >= 0 && s_cost[a] < best_cost) {
        best_cost = s_cost[a];
        best_axis = a;
        best_split = s_split[a];
      }
    const float bbh = half_area(bb);
    if (may_leaf && (best_axis < 0 || kNodeCost * bbh + best_cost >= static_cast<float>(n) * bbh)) {
      if (t == 0) emit_leaf(A, lo, cnt, seg.parent, seg.side);
      return;
    }
    if (best_axis >= 0) {
      const float scale = kBins / (cmx[best_axis] - cmn[best_axis]);
      bool left[kPer];
      uint32_t mine = 0;
      for (int k = 0; k < kPer; k++) {
        left[k] = m.valid[k] && bin_of(m.c[k][best_axis], cmn[best_axis], scale) <= best_split;
        mine += left[k] ? 1u : 0u;
      }
      uint32_t nleft;
      uint32_t before = block_excl_scan(mine, s_scan, nleft);
      if (nleft > 0 && nleft < cnt) {
        // all of perm[lo, hi) was read into registers before the first barrier: in place
        for (int k = 0; k < kPer; k++) {
          if (!m.valid[k]) continue;
          const uint32_t i = kPer * t + k;
          A.perm[lo + (left[k] ? before : nleft + (i - before))] = m.p[k];
          before += left[k] ? 1u : 0u;
        }
        mid = lo + nleft;
      }
    }
  }
  if (mid == lo || mid == hi) {
    // object median on the widest centroid axis: position = rank in the total order (centre, id)
    const int axis = widest_axis(cmn, cmx);
    for (int k = 0; k < kPer; k++)
      if (m.valid[k]) s_keys[kPer * t + k] = median_key(m.c[k][axis], m.p[k]);
    __syncthreads();
    for (int k = 0; k < kPer; k++) {
      if (!m.valid[k]) continue;
      const uint64_t key = s_keys[kPer * t + k];
      uint32_t rank = 0;
      for (uint32_t j = 0; j < cnt; j++) rank += s_keys[j] < key ? 1u : 0u;
      A.perm[lo + rank] = m.p[k];
    }
    mid = lo + cnt / 2;
  }
  if (t == 0) emit_split(A, seg, mid, parity ^ 1u);
}

// ------------------------------------------------------------------------------------------ large segments
__global__ __launch_bounds__(kBlock) void k_large_init(SahArgs A, uint32_t n_large) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n_large * kLargeWords) return;
  const uint32_t k = j % kLargeWords;
  uint32_t v = 0;
  if (k < 12) v = bound_init_word(k);
  else if (k >= 16) v = bin_init_word(k - 16);
  reinterpret_cast<uint32_t*>(A.lstate)[j] = v;
}

__global__ __launch_bounds__(kBlock) void k_large_bounds(SahArgs A) {
  __shared__ uint32_t s_bounds[12];
  const Chunk ch = A.chunks[blockIdx.x];
  Mine m;
  load_mine(A, ch.lo, ch.hi, m);
  if (threadIdx.x < 12) s_bounds[threadIdx.x] = bound_init_word(threadIdx.x);
  __syncthreads();
  bounds_to_lds(m, s_bounds);
  __syncthreads();
  if (threadIdx.x < 12) {
    uint32_t* g = &A.lstate[ch.seg].bounds[threadIdx.x];
    if (threadIdx.x % 6 < 3) atomicMin(g, s_bounds[threadIdx.x]);
    else atomicMax(g, s_bounds[threadIdx.x]);
  }
}

__device__ __forceinline__ void large_centre_bounds(const LargeState& st, float cmn[3], float cmx[3]) {
  for (int a = 0; a < 3; a++) {
    cmn[a] = dec(st.bounds[a]);
    cmx[a] = dec(st.bounds[3 + a]);
  }
}

__global__ __launch_bounds__(kBlock) void k_large_bin(SahArgs A) {
  __shared__ uint32_t s_bins[kSegBinWords];
  const Chunk ch = A.chunks[blockIdx.x];
  LargeState& st = A.lstate[ch.seg];
  Mine m;
  load_mine(A, ch.lo, ch.hi, m);
  for (uint32_t j = threadIdx.x; j < static_cast<uint32_t>(kSegBinWords); j += kBlock) s_bins[j] = bin_init_word(j);
  float cmn[3], cmx[3];
  large_centre_bounds(st, cmn, cmx);
  __syncthreads();
  bins_to_lds(m, cmn, cmx, A.w, s_bins);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < 3u * kBins; b += kBlock) {
    const uint32_t* src = s_bins + b * kBinWords;
    if (!src[6]) continue;  // nothing of this chunk fell into the bin
    uint32_t* dst = st.bins + b * kBinWords;
    for (int x = 0; x < 3; x++) {
      atomicMin(&dst[x], src[x]);
      atomicMax(&dst[3 + x], src[3 + x]);
    }
    atomicAdd(&dst[6], src[6]);
  }
}

// one 64-thread workgroup per large segment: the split, or the median path (a large segment is never a leaf)
__global__ __launch_bounds__(64) void k_large_split(SahArgs A, uint32_t depth) {
  __shared__ float s_cost[3];
  __shared__ int s_split[3];
  LargeState& st = A.lstate[blockIdx.x];
  const int t = threadIdx.x;
  const bool median = static_cast<int>(depth) >= kBvhMaxDepth - 26;
  float cmn[3], cmx[3];
  large_centre_bounds(st, cmn, cmx);
  if (t < 3) {
    s_cost[t] = kFltMax;
    s_split[t] = -1;
    if (!median && cmx[t] - cmn[t] > 0.f) axis_best(st.bins + t * kAxisWords, s_cost[t], s_split[t]);
  }
  __syncthreads();
  if (t) return;
  float best_cost = kFltMax;
  int best_axis = -1, best_split = -1;
  for (int a = 0; a < 3; a++)
    if (s_split[a] >= 0 && s_cost[a] < best_cost) {
      best_cost = s_cost[a];
      best_axis = a;
      best_split = s_split[a];
    }
  uint32_t nleft = 0;
  if (best_axis >= 0) {
    for (int b = 0; b <= best_split; b++) nleft += st.bins[best_axis * kAxisWords + b * kBinWords + 6];
    nleft /= A.w;
  }
  const Seg seg = A.large[depth & 1u][blockIdx.x];
  const bool med = best_axis < 0 || nleft == 0 || nleft >= seg.hi - seg.lo;
  st.axis = best_axis;
  st.split = best_split;
  st.nleft = nleft;
  st.median = med ? 1u : 0u;
  if (med) atomicOr(&A.ctr[4], 1u);
}

__device__ __forceinline__ uint32_t large_left_flags(const SahArgs& A, const Chunk& ch, const Mine& m, bool left[kPer]) {
  const LargeState& st = A.lstate[ch.seg];
  float cmn[3], cmx[3];
  large_centre_bounds(st, cmn, cmx);
  const int axis = st.axis, split = st.split;
  const float scale = kBins / (cmx[axis] - cmn[axis]);
  uint32_t mine = 0;
  for (int k = 0; k < kPer; k++) {
    left[k] = m.valid[k] && bin_of(m.c[k][axis], cmn[axis], scale) <= split;
    mine += left[k] ? 1u : 0u;
  }
  return mine;
}

__global__ __launch_bounds__(kBlock) void k_large_count(SahArgs A) {
  __shared__ uint32_t s_scan[kBlock];
  const Chunk ch = A.chunks[blockIdx.x];
  if (A.lstate[ch.seg].median) return;  // uniform
  Mine m;
  load_mine(A, ch.lo, ch.hi, m);
  bool left[kPer];
  uint32_t total;
  block_excl_scan(large_left_flags(A, ch, m, left), s_scan, total);
  if (threadIdx.x == 0) A.chunk_left[blockIdx.x] = total;
}

// left elements of the segment before each chunk: the chunks of one segment follow each other in the list, a thread per
// chunk adds up its predecessors' counts (at most n / kSmall independent loads, for the root)
__global__ __launch_bounds__(kBlock) void k_large_scan(SahArgs A, uint32_t n_chunks) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_chunks) return;
  const Chunk ch = A.chunks[c];
  if (A.lstate[ch.seg].median) return;
  uint32_t off = 0;
  for (uint32_t j = ch.first; j < c; j++) off += A.chunk_left[j];
  A.chunk_off[c] = off;
}

__global__ __launch_bounds__(kBlock) void k_large_scatter(SahArgs A, uint32_t parity) {
  __shared__ uint32_t s_scan[kBlock];
  const Chunk ch = A.chunks[blockIdx.x];
  const LargeState& st = A.lstate[ch.seg];
  if (st.median) return;  // uniform
  const Seg seg = A.large[parity][ch.seg];
  Mine m;
  load_mine(A, ch.lo, ch.hi, m);
  bool left[kPer];
  uint32_t total;
  uint32_t before = block_excl_scan(large_left_flags(A, ch, m, left), s_scan, total);
  const uint32_t left_before_chunk = A.chunk_off[blockIdx.x];
  const uint32_t right_before_chunk = (ch.lo - seg.lo) - left_before_chunk;
  for (int k = 0; k < kPer; k++) {
    if (!m.valid[k]) continue;
    const uint32_t i = kPer * threadIdx.x + k;
    const uint32_t dst = left[k] ? seg.lo + left_before_chunk + before : seg.lo + st.nleft + right_before_chunk + (i - before);
    A.perm_alt[dst] = m.p[k];
    before += left[k] ? 1u : 0u;
  }
}

__global__ __launch_bounds__(kBlock) void k_large_copyback(SahArgs A) {
  const Chunk ch = A.chunks[blockIdx.x];
  if (A.lstate[ch.seg].median) return;
  for (uint32_t i = ch.lo + threadIdx.x; i < ch.hi; i += kBlock) A.perm[i] = A.perm_alt[i];
}

// the median path of large segments: every position gets (key, value) such that sorting by key and then stably by the
// high half of the value leaves everything outside those segments where it is and orders the segments by (centre, id)
__global__ __launch_bounds__(kBlock) void k_msort_fill(SahArgs A, uint64_t* __restrict__ key, uint64_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= A.n) return;
  key[i] = i;
  val[i] = (static_cast<uint64_t>(i) << 32) | A.perm[i];
}
__global__ __launch_bounds__(kBlock) void k_msort_chunk(SahArgs A, uint32_t parity, uint64_t* __restrict__ key, uint64_t* __restrict__ val) {
  const Chunk ch = A.chunks[blockIdx.x];
  const LargeState& st = A.lstate[ch.seg];
  if (!st.median) return;
  const Seg seg = A.large[parity][ch.seg];
  float cmn[3], cmx[3];
  large_centre_bounds(st, cmn, cmx);
  const int axis = widest_axis(cmn, cmx);
  for (uint32_t i = ch.lo + threadIdx.x; i < ch.hi; i += kBlock) {
    const uint32_t p = A.perm[i];
    key[i] = median_key(A.pcen[3 * static_cast<size_t>(p) + axis], p);
    val[i] = (static_cast<uint64_t>(seg.lo) << 32) | p;
  }
}
__global__ __launch_bounds__(kBlock) void k_msort_split(uint32_t n, const uint64_t* __restrict__ val, uint32_t* __restrict__ key32, uint32_t* __restrict__ val32) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  key32[i] = static_cast<uint32_t>(val[i] >> 32);
  val32[i] = static_cast<uint32_t>(val[i]);
}

__global__ __launch_bounds__(kBlock) void k_large_emit(SahArgs A, uint32_t n_large, uint32_t parity) {
  const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_large) return;
  const Seg seg = A.large[parity][s];
  const LargeState& st = A.lstate[s];
  emit_split(A, seg, st.median ? seg.lo + (seg.hi - seg.lo) / 2 : seg.lo + st.nleft, parity ^ 1u);
}

// a scene of at most kBvhMaxLeaf triangles: the root pair with one leaf and an absent child, as the host builder makes it
__global__ void k_sah_single(uint32_t total, BvhNodeQ* __restrict__ nodes, uint32_t* __restrict__ leaf_order, uint32_t* __restrict__ refit_order,
                             uint32_t* __restrict__ header) {
  if (blockIdx.x || threadIdx.x) return;
  BvhNodeQ nd;
  for (int k = 0; k < 12; k++) nd.box[k] = 0;
  nd.lref = kLeafBit | (total - 1u);
  nd.rref = kBvhEmpty;
  nodes[0] = nd;
  for (uint32_t k = 0; k < total; k++) leaf_order[k] = k;
  refit_order[0] = 0;
  header[0] = 0;
  header[1] = 1;
  header[2] = 1;
}

struct Layout {
  size_t pbox, pcen, perm, perm_alt, kl, kr, parent, leaf_parent, slot, height, rank, hkey, hval, order, range_key, range_key_b, range_val, small[2], large[2],
      lstate, chunks, chunk_left, chunk_off, ctr, mkey_a, mkey_b, mval_a, mval_b, sort_tmp, sort_tmp_bytes, total;
  uint32_t cap_large, cap_chunks;
};

hipError_t make_layout(uint32_t n, Layout& L) {
  const size_t N = n;
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += up256(bytes);
    return at;
  };
  L.cap_large = n / kSmall + 2;
  L.cap_chunks = n / kSmall + L.cap_large + 1;
  L.pbox = take(N * 24);
  L.pcen = take(N * 12);
  L.perm = take(N * 4);
  L.perm_alt = take(N * 4);
  L.kl = take(N * 4);
  L.kr = take(N * 4);
  L.parent = take(N * 4);
  L.leaf_parent = take(N * 4);
  L.slot = take(N * 4);
  L.height = take(N * 4);
  L.rank = take(N * 4);
  L.hkey = take(N * 4);
  L.hval = take(N * 4);
  L.order = take(N * 4);
  L.range_key = take(N * 8);
  L.range_key_b = take(N * 8);
  L.range_val = take(N * 4);
  for (int p = 0; p < 2; p++) L.small[p] = take((N / 2 + 1) * sizeof(Seg));
  for (int p = 0; p < 2; p++) L.large[p] = take(L.cap_large * sizeof(Seg));
  L.lstate = take(L.cap_large * sizeof(LargeState));
  L.chunks = take(L.cap_chunks * sizeof(Chunk));
  L.chunk_left = take(L.cap_chunks * 4);
  L.chunk_off = take(L.cap_chunks * 4);
  L.ctr = take(kCtrWords * 4);
  // the median path of large segments (rare: allocated all the same, a rebuild must not allocate)
  L.mkey_a = take(N * 8);
  L.mkey_b = take(N * 8);
  L.mval_a = take(N * 8);
  L.mval_b = take(N * 8);
  size_t t64 = 0, t6464 = 0, t32 = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, t64, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                           static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), N, 0, 64, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::radix_sort_pairs(nullptr, t6464, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr),
                                static_cast<uint64_t*>(nullptr), N, 0, 64, nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::radix_sort_pairs(nullptr, t32, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr),
                                static_cast<uint32_t*>(nullptr), N, 0, 32, nullptr);
  if (e != hipSuccess) return e;
  L.sort_tmp_bytes = std::max(t64, std::max(t6464, t32));
  L.sort_tmp = take(L.sort_tmp_bytes ? L.sort_tmp_bytes : 1);
  L.total = off;
  return hipSuccess;
}

}  // namespace

size_t sah_scratch_bytes(uint32_t n_prims) {
  Layout L;
  if (n_prims < 2) return 256;
  return make_layout(n_prims, L) == hipSuccess ? L.total : 0;
}

hipError_t launch_sah_build(const LbvhArgs& a, void* scratch, size_t scratch_bytes, hipStream_t s) {
  if (!a.n_prims || (a.prim_w != 1 && a.prim_w != 2) || !scratch) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(a.header, 0, kLbvhHeaderWords * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const uint32_t n = a.n_prims, w = a.prim_w;
  if (n * w <= static_cast<uint32_t>(kBvhMaxLeaf)) {
    hipLaunchKernelGGL(k_sah_single, dim3(1), dim3(64), 0, s, n * w, a.nodes, a.leaf_order, a.refit_order, a.header);
    return hipGetLastError();
  }
  Layout L;
  if ((e = make_layout(n, L)) != hipSuccess) return e;
  if (L.total > scratch_bytes) return hipErrorInvalidValue;
  char* base = static_cast<char*>(scratch);
  auto u32 = [base](size_t off) { return reinterpret_cast<uint32_t*>(base + off); };
  auto u64 = [base](size_t off) { return reinterpret_cast<uint64_t*>(base + off); };
  SahArgs A;
  A.n = n;
  A.w = w;
  A.tris = a.tris;
  A.pbox = reinterpret_cast<float*>(base + L.pbox);
  A.pcen = reinterpret_cast<float*>(base + L.pcen);
  A.perm = u32(L.perm);
  A.perm_alt = u32(L.perm_alt);
  A.kl = u32(L.kl);
  A.kr = u32(L.kr);
  A.parent = u32(L.parent);
  A.leaf_parent = u32(L.leaf_parent);
  A.range_key = u64(L.range_key);
  A.range_val = u32(L.range_val);
  for (int p = 0; p < 2; p++) {
    A.small[p] = reinterpret_cast<Seg*>(base + L.small[p]);
    A.large[p] = reinterpret_cast<Seg*>(base + L.large[p]);
  }
  A.lstate = reinterpret_cast<LargeState*>(base + L.lstate);
  A.chunks = reinterpret_cast<Chunk*>(base + L.chunks);
  A.chunk_left = u32(L.chunk_left);
  A.chunk_off = u32(L.chunk_off);
  A.ctr = u32(L.ctr);
  uint32_t* slot = u32(L.slot);
  uint32_t* height = u32(L.height);
  uint32_t* rank = u32(L.rank);
  uint32_t* hkey = u32(L.hkey);
  uint32_t* hval = u32(L.hval);
  uint32_t* order = u32(L.order);
  void* tmp = base + L.sort_tmp;
  size_t tmp_bytes = L.sort_tmp_bytes;

#define SAH_TRY(expr) \
  if ((e = (expr)) != hipSuccess) return e

  hipLaunchKernelGGL(k_sah_prims, grid_for(n), dim3(kBlock), 0, s, A);
  SAH_TRY(hipMemsetAsync(A.range_key, 0xFF, static_cast<size_t>(n) * 8, s));  // unused temporary indices sort behind the nodes
  SAH_TRY(hipMemsetAsync(A.leaf_parent, 0xFF, static_cast<size_t>(n) * 4, s));
  SAH_TRY(hipMemsetAsync(slot, 0xFF, static_cast<size_t>(n) * 4, s));
  SAH_TRY(hipMemsetAsync(A.ctr, 0, kCtrWords * 4, s));
  const Seg root{0u, n, kNone, 0u};
  std::vector<Seg> hl(1, root);  // this level's large table on the host
  uint32_t n_small = 0, n_large = 0;
  if (n > kSmall) {
    n_large = 1;
    SAH_TRY(hipMemcpyAsync(A.large[0], &root, sizeof root, hipMemcpyHostToDevice, s));
  } else {
    n_small = 1;
    SAH_TRY(hipMemcpyAsync(A.small[0], &root, sizeof root, hipMemcpyHostToDevice, s));
  }
  SAH_TRY(hipStreamSynchronize(s));  // `root` is on the stack
  std::vector<Chunk> hc;
  uint32_t ctr[kCtrWords];
  uint32_t depth = 0;
  for (; n_small || n_large; depth++) {
    if (depth >= 2u * static_cast<uint32_t>(kBvhMaxDepth)) return hipErrorInvalidValue;  // the median bounds the depth long before
    const uint32_t p = depth & 1u, np = p ^ 1u;
    const bool median = static_cast<int>(depth) >= kBvhMaxDepth - 26;
    SAH_TRY(hipMemsetAsync(A.ctr + 2 * np, 0, 8, s));
    SAH_TRY(hipMemsetAsync(A.ctr + 4, 0, 4, s));
    if (n_large) {
      if (n_large > L.cap_large) return hipErrorInvalidValue;
      hc.clear();
      for (uint32_t i = 0; i < n_large; i++) {
        const uint32_t first = static_cast<uint32_t>(hc.size());
        for (uint32_t lo = hl[i].lo; lo < hl[i].hi; lo += kSmall) hc.push_back(Chunk{i, lo, std::min(lo + kSmall, hl[i].hi), first});
      }
      const uint32_t nc = static_cast<uint32_t>(hc.size());
      if (nc > L.cap_chunks) return hipErrorInvalidValue;
      SAH_TRY(hipMemcpyAsync(A.chunks, hc.data(), hc.size() * sizeof(Chunk), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_large_init, grid_for(n_large * kLargeWords), dim3(kBlock), 0, s, A, n_large);
      hipLaunchKernelGGL(k_large_bounds, dim3(nc), dim3(kBlock), 0, s, A);
      if (!median) hipLaunchKernelGGL(k_large_bin, dim3(nc), dim3(kBlock), 0, s, A);
      hipLaunchKernelGGL(k_large_split, dim3(n_large), dim3(64), 0, s, A, depth);
      hipLaunchKernelGGL(k_large_count, dim3(nc), dim3(kBlock), 0, s, A);
      hipLaunchKernelGGL(k_large_scan, grid_for(nc), dim3(kBlock), 0, s, A, nc);
      hipLaunchKernelGGL(k_large_scatter, dim3(nc), dim3(kBlock), 0, s, A, p);
      hipLaunchKernelGGL(k_large_copyback, dim3(nc), dim3(kBlock), 0, s, A);
      SAH_TRY(hipGetLastError());
      SAH_TRY(hipMemcpyAsync(ctr, A.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
      SAH_TRY(hipStreamSynchronize(s));  // also: `hc` may be rewritten
      if (ctr[4]) {
        uint64_t *ka = u64(L.mkey_a), *kb = u64(L.mkey_b), *va = u64(L.mval_a), *vb = u64(L.mval_b);
        uint32_t *k32a = reinterpret_cast<uint32_t*>(ka), *k32b = reinterpret_cast<uint32_t*>(kb), *v32a = reinterpret_cast<uint32_t*>(va);
        hipLaunchKernelGGL(k_msort_fill, grid_for(n), dim3(kBlock), 0, s, A, ka, va);
        hipLaunchKernelGGL(k_msort_chunk, dim3(nc), dim3(kBlock), 0, s, A, p, ka, va);
        SAH_TRY(hipGetLastError());
        tmp_bytes = L.sort_tmp_bytes;
        SAH_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, ka, kb, va, vb, static_cast<size_t>(n), 0, 64, s));
        hipLaunchKernelGGL(k_msort_split, grid_for(n), dim3(kBlock), 0, s, n, vb, k32a, v32a);  // ka / va are consumed
        tmp_bytes = L.sort_tmp_bytes;
        SAH_TRY(rocprim::radix_sort_pairs(tmp, tmp_bytes, k32a, k32b, v32a, A.perm_alt, static_cast<size_t>(n), 0, 32, s));
        SAH_TRY(hipMemcpyAsync(A.perm, A.perm_alt, static_cast<size_t>(n) * 4, hipMemcpyDeviceToDevice, s));
      }
      hipLaunchKernelGGL(k_large_emit, grid_for(n_large), dim3(kBlock), 0, s, A, n_large, p);
    }
    if (n_small) hipLaunchKernelGGL(k_sah_small, dim3(n_small), dim3(kBlock), 0, s, A, p, depth);
    SAH_TRY(hipGetLastError());
    SAH_TRY(hipMemcpyAsync(ctr, A.ctr, sizeof ctr, hipMemcpyDeviceToHost, s));
    SAH_TRY(hipStreamSynchronize(s));
    n_small = ctr[2 * np];
    n_large = ctr[2 * np + 1];
    if (n_large) {
      if (n_large > L.cap_large) return hipErrorInvalidValue;
      hl.resize(n_large);
      SAH_TRY(hipMemcpyAsync(hl.data(), A.large[np], n_large * sizeof(Seg), hipMemcpyDeviceToHost, s));
      SAH_TRY(hipStreamSynchronize(s));
    }
  }
#undef SAH_TRY
  const uint32_t m = ctr[5];
  if (!m || m > n - 1) return hipErrorInvalidValue;
  // pre-order: the used temporary indices sorted by (first ascending, last descending); the unused ones follow
  tmp_bytes = L.sort_tmp_bytes;
  if ((e = rocprim::radix_sort_pairs(tmp, tmp_bytes, A.range_key, u64(L.range_key_b), A.range_val, order, static_cast<size_t>(n), 0, 64, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_rank, grid_for(m), dim3(kBlock), 0, s, m, order, rank);
  hipLaunchKernelGGL(k_emit_nodes, grid_for(m), dim3(kBlock), 0, s, m, w, 1u, order, rank, A.kl, A.kr, a.nodes, a.header);
  hipLaunchKernelGGL(k_emit_leaves, grid_for(n), dim3(kBlock), 0, s, n, w, A.perm, a.leaf_order);
  hipLaunchKernelGGL(k_heights, grid_for(n), dim3(kBlock), 0, s, n, A.leaf_parent, A.parent, slot, height, a.header);
  hipLaunchKernelGGL(k_height_keys, grid_for(m), dim3(kBlock), 0, s, m, order, height, hkey, hval, a.header);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  tmp_bytes = L.sort_tmp_bytes;
  // sorted heights land in scratch (rank's neighbour hkey is consumed: perm_alt); the nodes by height in refit_order
  return rocprim::radix_sort_pairs(tmp, tmp_bytes, hkey, A.perm_alt, hval, a.refit_order, static_cast<size_t>(m), 0, 7, s);
}

}  // namespace rt
