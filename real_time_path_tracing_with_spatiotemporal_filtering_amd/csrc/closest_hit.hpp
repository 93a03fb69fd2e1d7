// closest_hit.hpp — the ray-triangle tests and both closest-hit structures (brute force over wave-uniform records, the child-pair
// BVH with its node stack in LDS), stated once: the frame kernels (kernels.hip, through gbuffer_tile.hpp and pathtrace_tile.hpp)
// and the self-test kernels (selftest_kernels.hip) trace with the same code.  Everything here is force-inlined; the caller owns
// the dynamic LDS of the node stack.
#pragma once

#include "device_common.hpp"

namespace rt {
namespace {

// ------------------------------------------------------------------------------------------
// closest hit.  D4: the winner is min over (t, id) of ONE ray-triangle routine, so the result
// does not depend on which structure enumerates the candidates.
// ------------------------------------------------------------------------------------------
struct HitRec {
  float t;       // best t so far (initialised to tmax)
  uint32_t id1;  // primitive id + 1, 0 = none
  float u, v, ad;  // scaled barycentrics of the best hit, u NEGATED: b1 = -u/ad, b2 = v/ad (tri_test)
};

// The divisions of the tracing kernels are hipcc's correctly rounded ones, not exact::div_ (rtpt_math.hpp): the tracing kernels
// sit at their 64-VGPR budget (8 waves per SIMD), the short sequence keeps the refined reciprocal live next to the operands
// of the long path, and what the fewer instructions bring (K2 at 4K 368.7 -> 364.9 us with both) the spills take back on the
// BVH kernel (3.34 -> 3.41 ms; profiles/r03_div_ab.csv).  Two names so that the two groups stay easy to find.  (One exception
// since: the barycentrics of a hit in the brute-force kernels, hit_barycentrics<SHORT_DIV>, shade_segment.hpp.)
#define RTPT_DIV_TH(a, b) ((a) / (b))  // hit distances
#define RTPT_DIV_SH(a, b) ((a) / (b))  // shading (barycentrics, the light test, the pixel's ndc)

// What K2's shading leaves out or shortens, one bit per item so that scripts/build_variant.sh can build each alone
// (-DRTPT_TRACE_ITEMS=<mask>; profiles/r15_trace_shading_ab.txt):
//   1  the last segment of a path returns before the bounce nothing follows (shade_segment)
//   2  the light test takes the sign of its quotient without dividing (exact::quotient_positive)
//   8  the two barycentric divisions of a hit share one reciprocal (exact::div2_) in the brute-force instantiations that keep
//      their registers with it (pathtrace_tile, k_pathtrace_queue: SHORT_DIV)
// (4, the primary ray's two divisions by the frame height through exact::div2_, and 16, exact::div_ for the hit distance of the
// brute-force triangle tests, were measured with these and brought nothing: they are not kept.)
#ifndef RTPT_TRACE_ITEMS
#define RTPT_TRACE_ITEMS 11
#endif

// Scalar-triple-product form of Moller-Trumbore, plane normal n = e1 x e2 precomputed per triangle,
// division deferred until a candidate passes the inside tests:
//   det = -d.n,  tt = (o-v0).n,  c = (o-v0) x d,  u = e2.c,  v = -e1.c        (21 flops instead of 27)
// record: r0 = (v0.xyz, e1.x)  r1 = (e1.yz, e2.xy)  r2 = (e2.z, n.xyz)
template <bool TIE_BREAK>
__device__ __forceinline__ void tri_test(f3 o, f3 d, float4 r0, float4 r1, float4 r2, uint32_t id1, HitRec& h) {
  f3 v0{r0.x, r0.y, r0.z}, e1{r0.w, r1.x, r1.y}, e2{r1.z, r1.w, r2.x}, n{r2.y, r2.z, r2.w};
  f3 tv = o - v0;
  // The signs of u, v, tt follow the sign of det = -d.n.  Instead of comparing det with 0 and selecting three negations
  // (a v_cmp whose result three VOP3 selects must wait two cycles for), the sign bit of d.n is XORed into e2.c, e1.c and
  // tt: that yields -u, +v and -tt of the oriented triangle (v = -e1.c takes the other sign), so two of the tests read
  // the other way round and HitRec keeps -u (HitRec::u: negated).  Same decisions bit for bit: x <= 0 iff -x >= 0,
  // x < 0 iff -x > 0, v - (-u) is u + v.
  const float dn = exact::dot(d, n);
  const uint32_t sm = f2u(dn) & 0x80000000u;
  const float tt = u2f(f2u(exact::dot(tv, n)) ^ sm);
  const f3 c = exact::cross(tv, d);
  const float u = u2f(f2u(exact::dot(e2, c)) ^ sm);
  const float v = u2f(f2u(exact::dot(e1, c)) ^ sm);
  const float ad = __builtin_fabsf(dn);
  // no "ad > 0" term: with ad == 0 only u == v == 0 passes, th is then +inf (tt > 0), and +inf never beats h.t
  const bool ok = (u <= 0.0f) && (v >= 0.0f) && (v - u <= ad) && (tt < 0.0f);
  if (ok) {
    const float th = RTPT_DIV_TH(-tt, ad);
    bool better = th < h.t;
    if (TIE_BREAK) better = better || (th == h.t && h.id1 != 0 && id1 < h.id1);
    if (better) {
      h.t = th;
      h.id1 = id1;
      h.u = u;
      h.v = v;
      h.ad = ad;
    }
  }
}

// Two triangles (a, b, c), (a, c, d) of one fan-triangulated face (main.cpp:416-428 via D5: every `f` line of the
// Cornell OBJ is a quad) share v0 and the edge c - a: tv = o - v0, c = tv x d and e2_A . c == e1_B . c are the SAME
// binary32 values in both tests, so the second test reuses them — 17 instead of 30 VALU, each triangle's own arithmetic
// and the ascending-id update order unchanged (bit-identical hits).  SceneView::paired says every pair (2q, 2q+1) of the
// scene is such a pair (checked bitwise on the uploaded vertices, rtpt_scene_upload).
__device__ __forceinline__ void tri_pair_test(f3 o, f3 d, float4 r0, float4 r1, float4 r2, float4 q1, float4 q2, uint32_t id1, HitRec& h) {
  const f3 v0{r0.x, r0.y, r0.z}, e1{r0.w, r1.x, r1.y}, e2{r1.z, r1.w, r2.x}, n{r2.y, r2.z, r2.w};
  const f3 e2b{q1.z, q1.w, q2.x}, nb{q2.y, q2.z, q2.w};  // B: e1_B == e2 (bitwise), v0_B == v0
  const f3 tv = o - v0;
  const f3 c = exact::cross(tv, d);
  const float e2c = exact::dot(e2, c);
  {
    const float dn = exact::dot(d, n);
    const uint32_t sm = f2u(dn) & 0x80000000u;
    const float tt = u2f(f2u(exact::dot(tv, n)) ^ sm);
    const float u = u2f(f2u(e2c) ^ sm);
    const float v = u2f(f2u(exact::dot(e1, c)) ^ sm);
    const float ad = __builtin_fabsf(dn);
    if ((u <= 0.0f) && (v >= 0.0f) && (v - u <= ad) && (tt < 0.0f)) {
      const float th = RTPT_DIV_TH(-tt, ad);
      if (th < h.t) {
        h.t = th;
        h.id1 = id1;
        h.u = u;
        h.v = v;
        h.ad = ad;
      }
    }
  }
  {
    const float dn = exact::dot(d, nb);
    const uint32_t sm = f2u(dn) & 0x80000000u;
    const float tt = u2f(f2u(exact::dot(tv, nb)) ^ sm);
    const float u = u2f(f2u(exact::dot(e2b, c)) ^ sm);
    const float v = u2f(f2u(e2c) ^ sm);  // e1_B . c
    const float ad = __builtin_fabsf(dn);
    if ((u <= 0.0f) && (v >= 0.0f) && (v - u <= ad) && (tt < 0.0f)) {
      const float th = RTPT_DIV_TH(-tt, ad);
      if (th < h.t) {
        h.t = th;
        h.id1 = id1 + 1;
        h.u = u;
        h.v = v;
        h.ad = ad;
      }
    }
  }
}

// the same for a BVH leaf: leaves are met in traversal order, so equal distances keep the lower id (tri_test<true>'s rule),
// and the two ids come from the leaf's id list
__device__ __forceinline__ void tri_pair_test_leaf(f3 o, f3 d, float4 r0, float4 r1, float4 r2, f3 e2b, f3 nb, uint32_t id1, uint32_t id1b,
                                                   HitRec& h) {
  const f3 v0{r0.x, r0.y, r0.z}, e1{r0.w, r1.x, r1.y}, e2{r1.z, r1.w, r2.x}, n{r2.y, r2.z, r2.w};  // B: e1_B == e2 (bitwise), v0_B == v0
  const f3 tv = o - v0;
  const f3 c = exact::cross(tv, d);
  const float e2c = exact::dot(e2, c);
  {
    const float dn = exact::dot(d, n);
    const uint32_t sm = f2u(dn) & 0x80000000u;
    const float tt = u2f(f2u(exact::dot(tv, n)) ^ sm);
    const float u = u2f(f2u(e2c) ^ sm);
    const float v = u2f(f2u(exact::dot(e1, c)) ^ sm);
    const float ad = __builtin_fabsf(dn);
    if ((u <= 0.0f) && (v >= 0.0f) && (v - u <= ad) && (tt < 0.0f)) {
      const float th = RTPT_DIV_TH(-tt, ad);
      bool better = th < h.t;
      better = better || (th == h.t && h.id1 != 0 && id1 < h.id1);
      if (better) {
        h.t = th;
        h.id1 = id1;
        h.u = u;
        h.v = v;
        h.ad = ad;
      }
    }
  }
  {
    const float dn = exact::dot(d, nb);
    const uint32_t sm = f2u(dn) & 0x80000000u;
    const float tt = u2f(f2u(exact::dot(tv, nb)) ^ sm);
    const float u = u2f(f2u(exact::dot(e2b, c)) ^ sm);
    const float v = u2f(f2u(e2c) ^ sm);  // e1_B . c
    const float ad = __builtin_fabsf(dn);
    if ((u <= 0.0f) && (v >= 0.0f) && (v - u <= ad) && (tt < 0.0f)) {
      const float th = RTPT_DIV_TH(-tt, ad);
      bool better = th < h.t;
      better = better || (th == h.t && h.id1 != 0 && id1b < h.id1);
      if (better) {
        h.t = th;
        h.id1 = id1b;
        h.u = u;
        h.v = v;
        h.ad = ad;
      }
    }
  }
}

// Small scenes (<= 64 triangles, the Cornell box has 32): every lane of the wave tests the same
// triangle at the same time, so the record address is wave-uniform and the loads are scalar
// (s_load_dwordx4 -> SGPR operands of the VALU ops).  No stack, no divergence, no memory latency.
__device__ __forceinline__ void closest_hit_brute(const SceneView& sc, f3 o, f3 d, HitRec& h) {
  // The records are read through the CONSTANT address space: they are never written while a kernel
  // that traces runs, and saying so keeps the loads scalar (s_load_dwordx4) even when the surrounding
  // loop also stores pixels — otherwise hipcc must assume the stores may clobber them and falls back
  // to one vector load + vmcnt(0) per triangle (measured: 2x slower).
  typedef float v4f __attribute__((ext_vector_type(4)));
  using cv4f = const __attribute__((address_space(4))) v4f;
  cv4f* rec = (cv4f*)sc.isect_id;
  const uint32_t n = sc.n_tris;
  constexpr int kBruteUnroll = 8;  // triangles whose records are fetched per batch of scalar loads; K2 at 4K: 2: 517, 4: 505, 8: 499, 16: 498 us
  constexpr int kPairUnroll = 8;   // faces whose records are fetched per batch of scalar loads; K2 at 4K: 2: 384.7, 4: 378.1, 8: 376.3, 16: 376.0 us
  if (sc.paired) {  // wave-uniform
#pragma unroll kPairUnroll
    for (uint32_t i = 0; i < n; i += 2) {
      const v4f a0 = rec[3 * i], a1 = rec[3 * i + 1], a2 = rec[3 * i + 2], b1 = rec[3 * i + 4], b2 = rec[3 * i + 5];
      tri_pair_test(o, d, make_float4(a0.x, a0.y, a0.z, a0.w), make_float4(a1.x, a1.y, a1.z, a1.w), make_float4(a2.x, a2.y, a2.z, a2.w),
                    make_float4(b1.x, b1.y, b1.z, b1.w), make_float4(b2.x, b2.y, b2.z, b2.w), i + 1, h);
    }
    return;
  }
#pragma unroll kBruteUnroll
  for (uint32_t i = 0; i < n; i++) {
    const v4f a0 = rec[3 * i], a1 = rec[3 * i + 1], a2 = rec[3 * i + 2];
    tri_test<false>(o, d, make_float4(a0.x, a0.y, a0.z, a0.w), make_float4(a1.x, a1.y, a1.z, a1.w),
                    make_float4(a2.x, a2.y, a2.z, a2.w), i + 1, h);
  }
}

// Pixels of a 64 x 4 tile a wave starts on: not row w of the tile but the 16 x 4 block of columns [16 w, 16 w + 16).  Rays that
// start through neighbouring pixels walk the same BVH nodes, and a block's rays diverge later than a row's (node-loop lane
// utilisation of the primary rays 0.66 -> 0.77, profiles/r04_wave_block_ab.txt); on small scenes the block's padded
// screen rectangle meets fewer triangle bounds than a 64-pixel span's.
constexpr int kWaveW = 16, kWaveH = 4;  // a wave's footprint in its tile
__device__ __forceinline__ uint32_t tile_pixel(int wave, uint32_t lane) {  // index (row << 6 | column) within the tile
  return ((lane >> 4) << 6) | (static_cast<uint32_t>(wave) << 4) | (lane & 15u);
}
// first column of wave `wave`'s footprint, relative to its tile (its first row is the tile's)
__device__ __forceinline__ int wave_x0(int wave) { return kWaveW * wave; }
// Primary rays of one wave (the kWaveW x kWaveH pixels from (x0, y0)) can only hit triangles whose padded
// screen bounds meet that rectangle.  Lane i classifies triangle i (n <= 64) and the ballot is the
// candidate set; must be called with the whole wave converged (before any early return).
__device__ __forceinline__ unsigned long long span_candidates(const TriBounds* bounds, uint32_t n, int x0, int y0) {
  const uint32_t lane = threadIdx.x & 63u;
  const TriBounds b = bounds[lane < n ? lane : 0u];
  const bool overlap = lane < n && !(b.x0 > x0 + kWaveW - 1 || b.x1 < x0 || b.y0 > y0 + kWaveH - 1 || b.y1 < y0);
  return __ballot(overlap);
}

// brute force over a wave-uniform candidate set; ascending ids, so equal-t ties keep the lower id
__device__ __forceinline__ void closest_hit_brute_set(const SceneView& sc, unsigned long long cand, f3 o, f3 d, HitRec& h) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  using cv4f = const __attribute__((address_space(4))) v4f;
  cv4f* rec = (cv4f*)sc.isect_id;
  const bool paired = sc.paired != 0;
  while (cand) {
    const uint32_t i = static_cast<uint32_t>(__builtin_ctzll(cand));
    cand &= cand - 1;
    const v4f a0 = rec[3 * i], a1 = rec[3 * i + 1], a2 = rec[3 * i + 2];
    if (paired && !(i & 1u) && (cand & (1ull << (i + 1)))) {  // both triangles of a fan pair are candidates (wave-uniform)
      cand &= cand - 1;
      const v4f b1 = rec[3 * i + 4], b2 = rec[3 * i + 5];
      tri_pair_test(o, d, make_float4(a0.x, a0.y, a0.z, a0.w), make_float4(a1.x, a1.y, a1.z, a1.w), make_float4(a2.x, a2.y, a2.z, a2.w),
                    make_float4(b1.x, b1.y, b1.z, b1.w), make_float4(b2.x, b2.y, b2.z, b2.w), i + 1, h);
      continue;
    }
    tri_test<false>(o, d, make_float4(a0.x, a0.y, a0.z, a0.w), make_float4(a1.x, a1.y, a1.z, a1.w),
                    make_float4(a2.x, a2.y, a2.z, a2.w), i + 1, h);
  }
}

// General scenes: per-lane depth-first traversal of the child-pair BVH with the node stack in LDS
// (stack[level][thread]: consecutive lanes hit consecutive banks; the stack is sized to the depth of
// the tree that was built, PathtraceArgs/SceneView::stack_depth).
//
// "while-while" form: the inner loop only walks interior nodes; a leaf child that must be visited is
// pushed (or becomes `cur`) as a leaf reference and is tested in the outer loop.  In the first version
// every iteration fetched a node AND ran the triangle loops of whichever children were leaves under
// a divergent branch; PMC showed ~37 % lane utilisation on the 1.15M-triangle scene.  Here lanes that
// reach a leaf wait at the loop exit and the wave tests leaves together.
//   child reference: bit 31 clear = interior node index; bit 31 set = leaf, (first << 2) | (count - 1);
//   kBvhEmpty = absent child; kSentinel = empty stack.
// Nodes are 32 bytes (two dwordx4 per visit): boxes on the scene's 16-bit grid, rounded outward — they only
// order and cull; the triangle test is binary32 on the exact records.  A box corner q stands for origin + q * cell, so with
// inv = cell / d and oi = (origin - o) / d a slab distance is one convert + one fma: t = q * inv + oi.
constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kSentinel = 0xFFFFFFFEu;
constexpr int kBvhLeafRatio = 2;  // waiting lanes per walking lane at which the node loop hands over.  Plain while-while: 2981 us, 1: 2734, 2: 2714, 3: 2728 for K2 on the 1.15M-triangle frame (profiles/r04_bvh_ab.txt)
constexpr int kLeafBatch = 2;     // 1: 3.72 ms, 2: 3.65 ms, 4: 4.79 ms (registers) on the 1.15M-triangle trace

// Profiling builds (never the shipped library): -DRTPT_BVH_COUNT=1 counts the trips and active lanes of the traversal's loops
// (scripts/bvh_count.py), -DRTPT_TILE_TIMELINE=1 records when every K0 / K2 workgroup starts and ends (scripts/tile_timeline.py).
// Their definitions live in experiments/trace_instrumentation.inc; what remains here are the hooks.
#ifndef RTPT_BVH_COUNT
#define RTPT_BVH_COUNT 0
#endif
#ifndef RTPT_TILE_TIMELINE
#define RTPT_TILE_TIMELINE 0
#endif
#if RTPT_BVH_COUNT || RTPT_TILE_TIMELINE
#define RTPT_INSTR_DEVICE
#include "experiments/trace_instrumentation.inc"
#undef RTPT_INSTR_DEVICE
#endif
#if !RTPT_BVH_COUNT
#define RTPT_COUNT_TRIP(slot) do {} while (0)
#endif

template <bool PAIRS>  // the tree was built over fan pairs (bvh.hpp): a leaf is one or two of them (A, B, A, B)
__device__ __forceinline__ void closest_hit_bvh(const SceneView& sc, f3 o, f3 d, HitRec& h, uint32_t* stack,
                                               int tid, int nt = kThreads, int bucket = 0) {
  if (__builtin_isunordered(o.x, d.x) || __builtin_isunordered(o.y, d.y) || __builtin_isunordered(o.z, d.z)) return;  // see below
#if RTPT_BVH_COUNT
  RTPT_COUNT_BEGIN(bucket, d);
#endif
  // A ray with a NaN component cannot hit anything (every comparison of tri_test fails, D7) — but min/max drop
  // NaNs, so every box would "pass" and that one lane would walk all of the scene: on the 1.15M-triangle lattice
  // single frames took 38-47 ms instead of 6.3 because of a handful of such paths (the test at the top of the function).
  // A direction component that is exactly 0 (axis-parallel rays do occur: d = (0,0,1) was measured) would make
  // that axis' slab distances inf - inf = NaN, which min/max drop: the axis stops culling and the ray visits
  // every node ahead of it (34 755 node visits for one ray, 45 ms for the frame).  With |d| clamped to 1e-20 the
  // distances are +-huge with the right signs — the padded boxes keep every face of a box the ray can hit
  // further than the rounding error from the ray's coordinate — so the parallel axis culls correctly.
  auto nz = [](float v) { return __builtin_fabsf(v) < 1e-20f ? __builtin_copysignf(1e-20f, v) : v; };
  const f3 rd{fast::rcp_(nz(d.x)), fast::rcp_(nz(d.y)), fast::rcp_(nz(d.z))};
  // x = origin + q * cell  =>  t = (x - o) / d = q * (cell / d) + (origin - o) / d
  // the grid lives in device memory (a device-side refit rewrites it without the host knowing the numbers): six scalar
  // loads through the constant address space
  using cflt = const __attribute__((address_space(4))) float;
  cflt* gr = (cflt*)sc.bvh_grid;
  const f3 inv{gr[3] * rd.x, gr[4] * rd.y, gr[5] * rd.z};
  // The slab distances round (origin - o) / d, and the triangle test rounds o - v0: both errors grow with the origin's
  // distance from the scene, while the boxes' padding (1e-5 x the scene's size, bvh.cpp) does not.  Past ~100 scene
  // diagonals a ray the triangle test accepts at a vertex on a box's edge could find that box's interval empty and the
  // box culled.  So every box is widened per ray by a margin of 2^-19 (32 ulp) of the origin's L1 distance from the grid
  // origin, in position units: on axis a that is pm |1 / d_a| in t, folded into the near and far offsets (oin, oif), so
  // the node step is unchanged.  For an origin inside the scene the margin is below the padding.
  const float pm = 0x1p-19f * (__builtin_fabsf(gr[0] - o.x) + __builtin_fabsf(gr[1] - o.y) + __builtin_fabsf(gr[2] - o.z));
  const f3 oi{(gr[0] - o.x) * rd.x, (gr[1] - o.y) * rd.y, (gr[2] - o.z) * rd.z};
  const f3 mg{pm * __builtin_fabsf(rd.x), pm * __builtin_fabsf(rd.y), pm * __builtin_fabsf(rd.z)};
  const f3 oin{oi.x - mg.x, oi.y - mg.y, oi.z - mg.z}, oif{oi.x + mg.x, oi.y + mg.y, oi.z + mg.z};
  struct { uint32_t x, y, z; } const rot{rd.x < 0.0f ? 16u : 0u, rd.y < 0.0f ? 16u : 0u, rd.z < 0.0f ? 16u : 0u};
  int sp = 0;
  uint32_t cur = 0;  // root pair
  // entries [0, stack_lds) in LDS, the rest in global memory (SceneView::stack_spill)
  const int lds_levels = static_cast<int>(sc.stack_lds);
  const size_t spill_stride = static_cast<size_t>(gridDim.x) * gridDim.y * nt;
  uint32_t* const spill = sc.stack_spill + (static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * nt + tid;
  // the LDS half through an LDS-typed pointer: a generic one lets the compiler fold the two halves of a pop into one
  // flat_load_dword of a selected address
  using lds_u32 = __attribute__((address_space(3))) uint32_t;
  lds_u32* const stack_lds = (lds_u32*)stack;
  auto push = [&](uint32_t v) {
    if (sp < lds_levels)
      stack_lds[sp * nt + tid] = v;
    else
      spill[static_cast<size_t>(sp - lds_levels) * spill_stride] = v;
    sp++;
  };
  auto pop = [&]() -> uint32_t {
    if (sp > 0) {
      sp--;
      // always an LDS read (slot 0 when the entry is in the global half), then the rare global read under its own branch;
      // as one conditional expression over generic pointers the two became ONE flat_load_dword of a selected address,
      // and every pop went through the vector-memory pipe
      uint32_t v = stack_lds[(sp < lds_levels ? sp : 0) * nt + tid];
      if (__builtin_expect(sp >= lds_levels, 0)) v = spill[static_cast<size_t>(sp - lds_levels) * spill_stride];
      return v;
    }
    return kSentinel;
  };
  auto test_leaf = [&](uint32_t ref) {
    const uint32_t first = (ref & ~kLeafBit) >> 2, cnt = (ref & 3u) + 1u;
    if (PAIRS) {
      // (with kBvhMaxLeaf <= 2 a leaf is one pair: the loop is a single pass the compiler sees)
      for (uint32_t j = 0; j < (kBvhMaxLeaf <= 2 ? 1u : cnt); j += 2) {
#if RTPT_BVH_COUNT
        RTPT_COUNT_TRIP(2);
        my_leaves++;
#endif
        // one 80-byte pair record (SceneView::isect_leaf); base + 32-bit byte offset (rtpt_scene_upload bounds the scene)
        const float4* r = reinterpret_cast<const float4*>(reinterpret_cast<const unsigned char*>(sc.isect_leaf) + ((first + j) >> 1) * 80u);
        const float4 p0 = r[0], p1 = r[1], p2 = r[2], p3 = r[3], p4 = r[4];
        tri_pair_test_leaf(o, d, p0, p1, p2, f3{p3.x, p3.y, p3.z}, f3{p3.w, p4.x, p4.y}, f2u(p4.z) + 1, f2u(p4.w) + 1, h);
      }
      return;
    }
    // fetch the records of kLeafBatch triangles before testing any of them: one memory round trip per
    // batch instead of one per triangle (indices past the leaf are clamped to its last triangle and skipped)
    for (uint32_t j0 = 0; j0 < cnt; j0 += kLeafBatch) {
      float4 rec[kLeafBatch][3];
      uint32_t id[kLeafBatch];
#pragma unroll
      for (uint32_t u = 0; u < kLeafBatch; u++) {
        const uint32_t j = j0 + u < cnt ? j0 + u : cnt - 1u;
        const float4* r = sc.isect_leaf + 3 * static_cast<size_t>(first + j);
        rec[u][0] = r[0];
        rec[u][1] = r[1];
        rec[u][2] = r[2];
        id[u] = sc.leaf_ids[first + j];
      }
#pragma unroll
      for (uint32_t u = 0; u < kLeafBatch; u++)
        if (j0 + u < cnt) tri_test<true>(o, d, rec[u][0], rec[u][1], rec[u][2], id[u] + 1, h);
    }
  };
  auto node_step = [&]() {
#if RTPT_BVH_COUNT
    RTPT_COUNT_TRIP(0);
    my_nodes++;
#endif
    // base + 32-bit byte offset (a tree has < 2^27 nodes): the loads take the scalar base and a 32-bit vector offset instead
    // of a 64-bit address computed per step
    const uint4* np = reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned char*>(sc.nodes) + (cur << 5));
    const uint4 a = np[0], b = np[1];
    const uint32_t cl = b.z, cr = b.w;
    const float tb = h.t;
    float tl, tr;
    // Every dword of the six holds one axis of one box as (min16 | max16 << 16).  Rotated by 16 where the ray runs against
    // the axis (rot, per ray), its low half is the plane the ray meets first and its high half the one it leaves through:
    // the min / max pair per axis that sorted the two distances (12 per node) becomes one v_alignbit_b32 (6 per node).
    // Same values: fma(q, inv, oi) is monotonic in q, increasing for inv > 0 and decreasing for inv < 0 (|d| is clamped away
    // from 0 above, so inv is never 0 or NaN), so min(t(min), t(max)) IS t of the half selected here, bit for bit.
    // The near plane takes the offset widened towards the ray (oin), the far one the offset widened away from it (oif).
    auto near_far = [&](uint32_t w, uint32_t rot_, float inv_, float oin_, float oif_, float& tn_, float& tf_) {
      const uint32_t q = __builtin_amdgcn_alignbit(w, w, rot_);
      tn_ = fmaf_(static_cast<float>(q & 0xFFFFu), inv_, oin_);
      tf_ = fmaf_(static_cast<float>(q >> 16), inv_, oif_);
    };
    float n0, n1, n2, f0, f1, f2;
    near_far(a.x, rot.x, inv.x, oin.x, oif.x, n0, f0);
    near_far(a.y, rot.y, inv.y, oin.y, oif.y, n1, f1);
    near_far(a.z, rot.z, inv.z, oin.z, oif.z, n2, f2);
    tl = __builtin_fmaxf(__builtin_fmaxf(n0, n1), __builtin_fmaxf(n2, 0.0f));
    const bool sl = tl <= __builtin_fminf(__builtin_fminf(f0, f1), __builtin_fminf(f2, tb));
    near_far(a.w, rot.x, inv.x, oin.x, oif.x, n0, f0);
    near_far(b.x, rot.y, inv.y, oin.y, oif.y, n1, f1);
    near_far(b.y, rot.z, inv.z, oin.z, oif.z, n2, f2);
    tr = __builtin_fmaxf(__builtin_fmaxf(n0, n1), __builtin_fmaxf(n2, 0.0f));
    const bool sr = tr <= __builtin_fminf(__builtin_fminf(f0, f1), __builtin_fminf(f2, tb));
    const bool hl = sl & (cl != kBvhEmpty), hr = sr & (cr != kBvhEmpty);
    if (hl && hr) {
      const bool left_first = tl <= tr;
      push(left_first ? cr : cl);
      cur = left_first ? cl : cr;
    } else if (hl) {
      cur = cl;
    } else if (hr) {
      cur = cr;
    } else {
      cur = pop();
    }
  };
  // while-while with an early hand-over: the node loop stops not only when every lane holds a leaf (or is done) but as
  // soon as the lanes waiting with a leaf outnumber the lanes still walking kBvhLeafRatio to one — the few walkers
  // sit out one leaf test instead of the many waiting out the walkers' remaining steps
  while (cur != kSentinel) {
    while (true) {
      const bool walk = !(cur & kLeafBit);
      const unsigned long long mw = __ballot(walk);
      if (!mw) break;
      // lanes of this loop that are not walking hold a leaf (or have just run out of nodes): they wait
      const int nw = __builtin_popcountll(mw), na = __builtin_popcountll(__ballot(true));
      if (na - nw >= kBvhLeafRatio * nw) break;
      if (walk) node_step();
    }
    if ((cur & kLeafBit) && cur != kSentinel) {  // a leaf
      test_leaf(cur);
      cur = pop();
    }
  }
}

template <int BVH>
__device__ __forceinline__ void closest_hit(const SceneView& sc, f3 o, f3 d, HitRec& h, uint32_t* stack, int tid,
                                            int nt = kThreads, int bucket = 0) {
  // BVH: 0 brute force, 1 BVH over triangles, 2 BVH over fan pairs (SceneView::leaf_pairs) — a kernel holds one leaf routine
  if (BVH)
    closest_hit_bvh<BVH == 2>(sc, o, d, h, stack, tid, nt, bucket);
  else
    closest_hit_brute(sc, o, d, h);
}

// v0*b0 + v1*b1 + v2*b2 (raytrace.comp.glsl:137) := fma(v2,b2, fma(v1,b1, v0*b0))
__device__ __forceinline__ f3 bary_point(f3 v0, f3 v1, f3 v2, float b0, float b1, float b2) {
  return f3{fmaf_(v2.x, b2, fmaf_(v1.x, b1, v0.x * b0)), fmaf_(v2.y, b2, fmaf_(v1.y, b1, v0.y * b0)),
            fmaf_(v2.z, b2, fmaf_(v1.z, b1, v0.z * b0))};
}

// the scene's closest-hit mode, closest_hit's BVH, for with_mode<3> (select.hpp): 2 BVH over fan pairs, 1 BVH over triangles, 0
// brute force (the brute-force tile kernels have names of their own, *_small, for their occupancy pin)
inline int scene_mode(const SceneView& sc) { return sc.use_bvh ? (sc.leaf_pairs ? 2 : 1) : 0; }

}  // namespace
}  // namespace rt
