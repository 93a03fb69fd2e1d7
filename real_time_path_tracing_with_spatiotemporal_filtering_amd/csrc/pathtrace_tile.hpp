// pathtrace_tile.hpp — the body of the K2 tile kernels (k_pathtrace*, k_gbuffer_pathtrace*, k_pathtrace_final) and the steps it
// shares with the queue kernel (k_pathtrace_queue), all in kernels.hip: the exchange buffer of the compaction, the hand-over of
// unfinished paths to the next launch and the ray count; and the body of k_pathtrace_final's run workgroups, which serve the tile
// columns no triangle reaches (pathtrace_empty_run).  Everything here is force-inlined; the caller (a kernel, or
// pathtrace_tile for the tile kernels) owns the LDS.
#pragma once

#include "gbuffer_tile.hpp"
#include "shade_segment.hpp"

namespace rt {
namespace {

// K2 tile: 64 x kPtRows pixels per workgroup.  More paths compacted together shrink the share of the half-empty
// last wave of every later segment, but every compaction is a workgroup barrier on the slowest wave.  Swept at
// 4K (Cornell 4 segments / 1.15M triangles 8 segments, k_pathtrace): 2 rows 862 us / 4.18 ms, 3 rows 569 / 4.04,
// 4 rows 517 / 3.99, 8 rows 540 / 4.23, 16 rows 728 / 5.80.
constexpr int kPtRows = 4;
constexpr int kPtThreads = kBlockX * kPtRows;

// Hand-over of the paths a launch did not finish (PathtraceArgs::seg_end < max_segments) to the next launch: a
// workgroup appends ALL of its survivors with one atomic (the per-wave counts are summed through LDS).  One atomic
// per wave on the same counter serialised badly (tile kernel 516 -> 814 us with a window of 2).  The queue can be
// split into kPathQueues regions with a counter each (a region then holds the survivors of at most
// ceil(blocks / kPathQueues) workgroups: PathtraceArgs::queue_region records); once the atomics are per workgroup
// one region is the fastest, so that is what ships.
__device__ __forceinline__ void enqueue_paths(const PathtraceArgs& a, uint32_t region, uint32_t* wave_cnt, uint32_t* bcast,
                                              bool alive, int wave, uint32_t lane, uint32_t pixg, uint32_t rng, f3 o, f3 d, f3 acc) {
  const unsigned long long m = __ballot(alive);
  if (lane == 0) wave_cnt[wave] = static_cast<uint32_t>(__builtin_popcountll(m));
  __syncthreads();
  uint32_t before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kPtRows; w++) {
    const uint32_t c = wave_cnt[w];
    if (w < wave) before += c;
    total += c;
  }
  if (wave == 0 && lane == 0) *bcast = total ? atomicAdd(a.q_out_count + region, total) : 0u;
  __syncthreads();
  if (alive) {
    const uint32_t slot = region * a.queue_region + *bcast + before +
                          __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
    float4* q = reinterpret_cast<float4*>(a.q_out) + 3 * static_cast<size_t>(slot);
    q[0] = make_float4(__uint_as_float(pixg), __uint_as_float(rng), o.x, o.y);
    q[1] = make_float4(o.z, d.x, d.y, d.z);
    q[2] = make_float4(acc.x, acc.y, acc.z, 0.0f);
  }
  __syncthreads();  // wave_cnt / bcast may be reused right away
}

// K2 tile kernel with optional per-segment compaction (PathtraceArgs::compact).
//
// A 256-thread block owns a 64x4 pixel tile and advances all of its paths one segment at a time
// (the segment index is block-uniform).  The PRIMARY segment runs with the lane <-> pixel mapping
// intact, so a wave's rays are coherent and only the triangles whose screen bounds meet the wave's
// span are tested.  After every segment the surviving paths (light hit, sky and the segment budget
// end paths; at 4 segments the Cornell box averages 2.25 queries per pixel) are compacted to the
// front of the block through LDS, so secondary segments — incoherent anyway — run in full waves and
// emptied waves skip the segment entirely: 16 wave-segments per tile become ~10.  A path's RNG stream
// depends only on (x, y, frame, batch) (raytrace.comp.glsl:297) and every path runs the reference's
// loop body unchanged, so the image is independent of the schedule (bit-exact parity with the oracle).
// Measured in one process at 4K on the Cornell box (us, 4 / 8 / 32 segments): without compaction
// 503 / 985 / 3410, with 495 / 925 / 2810 — at 4 segments most waves retire early anyway (sky and the
// unoccluded light end whole waves), the gain grows with the path length.  (A per-wave path
// regeneration scheme — finished lanes pick up new pixels — was also built and measured: it mixes
// primary and secondary rays in every wave, loses the coherent, culled primary segment and ran
// 1.5x slower at 4 segments; it is not kept.)
struct PathState {  // SoA in LDS, one slot per thread
  uint32_t pix[kPtThreads];   // local pixel index (ty*64 + tx)
  uint32_t rng[kPtThreads];
  float ox[kPtThreads], oy[kPtThreads], oz[kPtThreads];
  float dx[kPtThreads], dy[kPtThreads], dz[kPtThreads];
  float ar[kPtThreads], ag[kPtThreads], ab[kPtThreads];
};

// "ray" = one closest-hit query; a thread's count `rays` goes through the wave and the workgroup's LDS word
// block_rays (zeroed by the caller) into ONE 64-bit atomic per workgroup, on counter `slot` of the kRayCounters: 32 400
// same-address atomics per 4K launch serialise in the memory system and kept the workgroups' slots occupied until acknowledged
// (a 1-segment launch took 397 us, of which the arithmetic is ~110)
__device__ __forceinline__ void add_block_rays(const PathtraceArgs& a, unsigned int rays, unsigned int* block_rays, int tid, uint32_t slot) {
  for (int off = 32; off > 0; off >>= 1) rays += __shfl_down(rays, off, 64);
  if ((tid & 63) == 0 && rays) atomicAdd(block_rays, rays);
  __syncthreads();
  const unsigned int sum = *block_rays;  // (read by every thread, as the compiler arranged it when this was written against the LDS word itself)
  if (tid == 0 && sum) atomicAdd(a.raycount + (slot & (kRayCounters - 1u)), static_cast<unsigned long long>(sum));
}

// The kernel needs its 8 waves per SIMD to hide the scalar-load latency of the brute-force loop; left alone the
// compiler keeps 106 SGPRs of kernel arguments live (7 waves).  Measured at 4K: 6 / 7 (compiler's choice) / 8 waves
// 506 / 505 / 479 us (a few dwords of scalar spills are cheaper than the lost wave).
constexpr int kPtWaves = 8;
// GB: the launch also holds the workgroups of K0 (+ K1) (gbuffer_pathtrace_body below), which put the G-buffer depth into the
// traced image's alpha themselves: a path that ends stores the 12 bytes of its colour only.  The launch's grid is then
// taller than the tile grid (a.tiles_y rows of tiles).
// DEMOD: RTPT_FLAG_EXT_DEMODULATE, the albedo store of segment 0 (PathtraceArgs::albedo).  A compile-time switch: as a run-time
// test the extra pointer cost the BVH variants, pinned at 64 VGPRs, 2 to 15 more spilled registers per lane, also with the flag off.
// TEX: shade_segment samples the scene's albedo textures.  SPEC: the materials it bounces and the lights it samples (kernels.hpp
// names the axis, shade_segment.hpp says what each value does).
// the tile grid's width / a tile's linear index, where pathtrace_tile used to read gridDim.x / compute the index (every use keeps
// its place, so that the ROLE = 0 instantiations compile to what they were)
template <int ROLE>
__device__ __forceinline__ uint32_t tile_gx(uint32_t role_gx) {
  if constexpr (ROLE != 0) return role_gx;
  else return gridDim.x;
}
template <int ROLE>
__device__ __forceinline__ uint32_t tile_lin(uint32_t role_lin) {
  if constexpr (ROLE != 0) return role_lin;
  else return blockIdx.y * gridDim.x + blockIdx.x;
}
// ROLE: 1 in the launch that also holds filter workgroups (k_pathtrace_final).  An instantiation of its own, so that its three
// static LDS words are that kernel's alone: shared between two kernels they would move into the module-wide LDS block and
// shift the dynamic LDS of every kernel of kernels.hip.
// lights: the light list as SPEC takes it (spec_lights_t<SPEC>), the tile kernels' trailing parameter pack: nothing where no light is
// sampled
// what shade_segment takes for the lights and for the normals, out of a tile kernel's pack (the ENV instantiations)
template <int SPEC, class... LV>
__device__ __forceinline__ auto tile_nee_args([[maybe_unused]] NeeState* st, const LV&... lights) {
  if constexpr (spec_lights(SPEC)) return NeeArgs<spec_lights_t<SPEC>>{pack_first(lights...), st};
  else return NoNee{};
}
template <bool NRM, class... LV>
__device__ __forceinline__ auto tile_normals(const LV&... lights) {
  if constexpr (NRM) return pack_get<NormalView>(lights...);
  else return NoNormals{};
}
template <int BVH, bool COMPACT, bool GB, bool DEMOD, int TEX, int SPEC = 0, int ROLE = 0, class... LV>
__device__ __forceinline__ void pathtrace_tile(const PathtraceArgs& a, const TexView& tex, const uint32_t role_lin = 0, const uint32_t role_gx = 0,
                                               const uint32_t role_gy = 0, const LV&... lights) {
  static_assert(pack_takes<SPEC, LV...>(), "an instantiation takes the light argument of its SPEC, spec_lights_t<SPEC>, then a NormalView or nothing, then an EnvView or nothing");
  constexpr bool NRM = pack_nrm<LV...>();  // kernels.hpp: the NRM axis; the pack then holds the scene's NormalView
  constexpr bool ENV = pack_env<LV...>();  // kernels.hpp: the ENV axis; the pack's last argument is then the context's EnvView
  // ROLE: the workgroup is tile role_lin of a role_gx x role_gy tile grid that is not the launch's own grid
  // dynamic LDS, two tenants that are never live together: the BVH node stack (stack_depth x 256 entries, only
  // inside closest_hit) and the compaction exchange buffer (only between the barriers of the compaction step).
  // Sharing it takes the BVH kernel from 41 to 30 KB per block: 5 instead of 3 resident blocks per CU for a
  // kernel that PMC shows waiting on memory for 78 % of its wave-cycles.
  extern __shared__ __attribute__((aligned(16))) uint32_t stack[];
  PathState& st = *reinterpret_cast<PathState*>(stack);
  // per-pixel sample accumulators and RNG state between samples: behind the shared region, allocated (by
  // launch_pathtrace) only when spp > 1 — the reference runs 1 spp (raytrace.comp.glsl:306); spp > 1 is an EXTENSION, see
  // the note at the rng_pix store below
  // spec_lights(SPEC): the pixel's radiance R, what its light samples collected so far (light_sample.hpp), sits where the sums sit
  // otherwise and the sums move behind it; allocated by launch_pathtrace for these instantiations only.  Indexed by the local
  // pixel `pix`, like the sums, because the compaction moves paths between threads; one path per pixel is live at a time, so a
  // plain read-modify-write has no race.  Zeroed at the start of every sample by the thread that starts on the pixel, read where
  // the path ends.
  // spec_mis(SPEC): a fourth array behind R, the cosine the pixel's path left its last diffuse hit with (NeeState::cb), so that it
  // follows the path through the compaction without a field in PathState, which every tracing kernel shares: written in front of
  // the compaction's first barrier by the thread that holds the path, read behind its second by the thread that takes it over,
  // and only while the sampled bit is set.  Without compaction the value stays in its register.  1 KB more per workgroup.
  constexpr uint32_t kRadWords = spec_mis(SPEC) ? 4u * kPtThreads : (spec_lights(SPEC) ? 3u * kPtThreads : 0u);
  [[maybe_unused]] float* const rad_r = reinterpret_cast<float*>(stack + a.multi_off);
  [[maybe_unused]] float* const rad_g = rad_r + kPtThreads;
  [[maybe_unused]] float* const rad_b = rad_g + kPtThreads;
  [[maybe_unused]] float* const cb_pix = rad_b + kPtThreads;  // spec_mis(SPEC)
  float* const sum_r = reinterpret_cast<float*>(stack + a.multi_off + kRadWords);
  float* const sum_g = sum_r + kPtThreads;
  float* const sum_b = sum_g + kPtThreads;
  uint32_t* const rng_pix = reinterpret_cast<uint32_t*>(sum_b + kPtThreads);
  __shared__ uint32_t wave_cnt[kPtRows];
  __shared__ uint32_t q_base;
  __shared__ unsigned int block_rays;
  const int tid = threadIdx.y * kBlockX + threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.y));
  const uint32_t lane = threadIdx.x;
  if (tid == 0) block_rays = 0;
  // workgroups are dispatched in the order of their linear index; tiles are taken column by column from the middle of
  // the frame outwards, so the last ones dispatched — the tail of the launch — are the outermost columns, where (camera
  // facing the scene) the paths are short.  A frame of a few thousand tiles is only ~2 generations of workgroups.
  const uint32_t tiles_y_ = GB ? a.tiles_y : (ROLE ? role_gy : gridDim.y);
  const uint32_t lin_ = tile_lin<ROLE>(role_lin), col_ = lin_ / tiles_y_;
  uint32_t bx_ = (col_ & 1u) ? (tile_gx<ROLE>(role_gx) - 1u) / 2u + (col_ + 1u) / 2u : (tile_gx<ROLE>(role_gx) - 1u) / 2u - col_ / 2u, by_ = lin_ % tiles_y_;
#if RTPT_TILE_TIMELINE
  if (g_tile_order_n == tile_gx<ROLE>(role_gx) * (ROLE ? role_gy : gridDim.y)) {
    const uint32_t t_ = g_tile_order[lin_];
    bx_ = t_ % tile_gx<ROLE>(role_gx);
    by_ = t_ / tile_gx<ROLE>(role_gx);
  }
#endif
#if RTPT_TILE_TIMELINE
  TimelineScope tl_(1, by_ * tile_gx<ROLE>(role_gx) + bx_);  // indexed by tile
#endif
  const int tile_x0 = static_cast<int>(bx_) * kBlockX, tile_y0 = a.g.y0 + static_cast<int>(by_) * kPtRows;
  const float fw = static_cast<float>(a.g.W), fh = static_cast<float>(a.g.H);
  const f3 light_c = ld3(a.light_c);
  unsigned int rays = 0;
  unsigned long long cand = 0;  // candidate triangles of this wave's (jittered) primary rays
  if (!BVH && a.cull) cand = span_candidates(a.bounds, a.scene.n_tris, tile_x0 + wave_x0(wave), tile_y0);

  // per-thread path registers
  const uint32_t pix0 = tile_pixel(wave, lane);  // the pixel this thread starts on
  uint32_t pix = pix0, rng = 0;
  f3 o{0.f, 0.f, 0.f}, d{0.f, 0.f, -1.f}, acc{1.f, 1.f, 1.f};
  [[maybe_unused]] NeeState nee{f3{0.f, 0.f, 0.f}, f3{0.f, 0.f, 0.f}, 0u, false, false, f3{0.f, 0.f, 0.f}, false, false, 0.0f};  // spec_lights(SPEC)
  {
    const int x = tile_x0 + static_cast<int>(pix0 & 63u), y = tile_y0 + static_cast<int>(pix0 >> 6);
    rng = exact::rng_seed(static_cast<uint32_t>(x), static_cast<uint32_t>(y), a.frame, a.batch);  // :297
    if (a.spp > 1) sum_r[tid] = sum_g[tid] = sum_b[tid] = 0.0f;
  }
  for (uint32_t smp = 0; smp < a.spp; smp++) {
    // ---- primary rays: thread <-> its starting pixel pix0 (mapping restored at the start of every sample)
    if (smp > 0) {
      __syncthreads();
      pix = pix0;
      rng = rng_pix[pix0];  // the pixel's RNG state after its previous sample (stored at path end)
    }
    if constexpr (spec_lights(SPEC)) {
      // (smp > 0: behind the barrier above, so the thread that ended this pixel's previous path has read its R)
      rad_r[pix0] = rad_g[pix0] = rad_b[pix0] = 0.0f;
      nee.sampled = false;  // the primary ray
      if constexpr (spec_sphere(SPEC)) nee.sphere = false;
    }
    const int px0 = tile_x0 + static_cast<int>(pix0 & 63u), py0 = tile_y0 + static_cast<int>(pix0 >> 6);
    bool alive = (px0 < a.g.W) && (py0 < a.g.y1);
    if (alive) {
      float u1 = glsl_max(1e-38f, exact::rng_next(rng));  // :87 Box-Muller
      float u2 = exact::rng_next(rng);
      float rad = exact::sqrt_(-2.0f * exact::log_(u1));
      float sn, cs;
      exact::sincos2pi(u2, sn, cs);
      float cx = fmaf_(a.jitter, rad * cs, static_cast<float>(px0) + 0.5f);  // :314
      float cy = fmaf_(a.jitter, rad * sn, static_cast<float>(py0) + 0.5f);
      float ux = RTPT_DIV_SH(fmaf_(2.0f, cx, -fw), fh);     // :315
      float uy = -RTPT_DIV_SH(fmaf_(2.0f, cy, -fh), fh);  // :316
      d = exact::normalize(f3{a.slope * ux, a.slope * uy, -1.0f});  // :319-320
      o = ld3(a.cam);
      acc = f3{1.f, 1.f, 1.f};  // :201
    }
    for (uint32_t seg = 0; seg < a.seg_end; seg++) {  // :204 (block-uniform); seg_end < max_segments: the rest is handed over
      if (alive) {
        HitRec h{a.tmax, 0u, 0.f, 0.f, 1.f};
        if (!BVH && a.cull && seg == 0)
          closest_hit_brute_set(a.scene, cand, o, d, h);
        else
          closest_hit<BVH>(a.scene, o, d, h, stack, tid, kPtThreads, 1 + static_cast<int>(seg));  // :208-222
        const int x = tile_x0 + static_cast<int>(pix & 63u), y = tile_y0 + static_cast<int>(pix >> 6);
        if (y >= a.count_y0 && y < a.count_y1) rays++;
        const size_t gi = static_cast<size_t>(y - a.g.row_base) * a.g.W + x;
        if (seg == 0 && smp == 0 && a.hit_id) a.hit_id[gi] = h.id1;
        // the short barycentric divisions where they cost no register: with DEMOD or without compaction they spill one
        constexpr bool kShortDiv = (RTPT_TRACE_ITEMS & 8) && BVH == 0 && COMPACT && !DEMOD;
        if constexpr (spec_lights(SPEC)) nee.valid = false;
        if constexpr (spec_sphere(SPEC)) nee.sphere_valid = false;
        bool done;
        if constexpr (ENV) {  // the same four forms with the EnvView behind them, their arguments picked from the pack by type
          using NeeT = std::conditional_t<spec_lights(SPEC), NeeArgs<spec_lights_t<SPEC>>, NoNee>;
          using NrmT = std::conditional_t<NRM, NormalView, NoNormals>;
          done = shade_segment<TEX, BVH, kShortDiv, SPEC, NeeT, NrmT, EnvView>(a, h, seg, light_c, o, d, acc, rng, tex, (DEMOD && seg == 0) ? a.albedo + gi : nullptr,
                                                                               tile_nee_args<SPEC>(&nee, lights...), tile_normals<NRM>(lights...),
                                                                               pack_get<EnvView>(lights...));
        } else if constexpr (NRM && spec_lights(SPEC))
          done = shade_segment<TEX, BVH, kShortDiv, SPEC, NeeArgs<spec_lights_t<SPEC>>, NormalView>(
              a, h, seg, light_c, o, d, acc, rng, tex, (DEMOD && seg == 0) ? a.albedo + gi : nullptr,
              NeeArgs<spec_lights_t<SPEC>>{pack_first(lights...), &nee}, pack_get<NormalView>(lights...));
        else if constexpr (NRM)
          done = shade_segment<TEX, BVH, kShortDiv, SPEC, NoNee, NormalView>(a, h, seg, light_c, o, d, acc, rng, tex,
                                                                             (DEMOD && seg == 0) ? a.albedo + gi : nullptr, NoNee{}, pack_get<NormalView>(lights...));
        else if constexpr (spec_lights(SPEC))
          done = shade_segment<TEX, BVH, kShortDiv, SPEC, NeeArgs<spec_lights_t<SPEC>>>(a, h, seg, light_c, o, d, acc, rng, tex,
                                                                                        (DEMOD && seg == 0) ? a.albedo + gi : nullptr,
                                                                                        NeeArgs<spec_lights_t<SPEC>>{lights..., &nee});
        else
          done = shade_segment<TEX, BVH, kShortDiv, SPEC>(a, h, seg, light_c, o, d, acc, rng, tex, (DEMOD && seg == 0) ? a.albedo + gi : nullptr);
        if constexpr (spec_lights(SPEC)) {
          // The sphere sample's gain (RTPT_FLAG_EXT_NEE_SPHERE) goes into R first: it needs no query, the order of the two additions
          // is fixed this way, and the gain is dead before the traversal below starts.
          if constexpr (spec_sphere(SPEC)) {
            if (nee.sphere_valid) {
              rad_r[pix] += nee.sphere_c.x;
              rad_g[pix] += nee.sphere_c.y;
              rad_b[pix] += nee.sphere_c.z;
            }
          }
          // The shadow query of the light sample, from the new origin towards the sampled point: the path's own closest hit, so
          // "unoccluded" is "the nearest triangle along the ray is the sampled one", ties resolved as the path resolves them.
          // No new barrier: in the BVH variants the node stack aliases the exchange buffer, which is written and read only
          // between the compaction's first barrier below and the barrier that ends it; this call sits where the segment's first
          // query sits, behind the previous compaction's last barrier and in front of this one's first.  R lies behind both.
          if (nee.valid) {
            HitRec hs{a.tmax, 0u, 0.f, 0.f, 1.f};
            closest_hit<BVH>(a.scene, o, nee.wd, hs, stack, tid, kPtThreads, 1 + static_cast<int>(seg));
            if (y >= a.count_y0 && y < a.count_y1) rays++;
            if (hs.id1 == nee.id1) {
              rad_r[pix] += nee.c.x;
              rad_g[pix] += nee.c.y;
              rad_b[pix] += nee.c.z;
            }
          }
          if (done) acc = f3{rad_r[pix] + acc.x, rad_g[pix] + acc.y, rad_b[pix] + acc.z};  // R + terminal
        }
        if (done) {
          alive = false;
          if (a.spp == 1) {
            // :328,:343 — alpha carries the G-buffer depth for the filter (rgbd)
            if (GB)
              store_rgb(a.image + gi, acc);  // alpha = the G-buffer depth, stored by the G-buffer workgroups of this launch
            else
              a.image[gi] = make_float4(acc.x, acc.y, acc.z, a.depth[gi]);
          } else {
            sum_r[pix] += acc.x;  // :325 (one path per pixel at a time: no race)
            sum_g[pix] += acc.y;
            sum_b[pix] += acc.z;
            // EXTENSION (not the reference's behaviour): the next sample of this pixel continues the stream after this
            // sample's bounce draws.  The reference text takes rngState by value into the bounce loop
            // (raytrace.comp.glsl:200), so with NUM_SAMPLES > 1 it would replay sample 0's bounce draws and only the jitter
            // stream of :314 would continue (tests/test_reference_shaders.py::test_samples_per_pixel_is_an_extension)
            rng_pix[pix] = rng;
          }
        }
      }
      if (seg + 1 >= a.seg_end) break;
      if (!COMPACT) {  // short paths: keep the lane <-> pixel mapping, a wave leaves when all its paths ended
        if (__ballot(alive) == 0ull) break;
        continue;
      }
      // ---- compact the survivors to the front of the block.  (k_pathtrace_queue states the same sequence a second time, on
      // purpose: as a function of either kernel's path registers — by reference, by value with a returned struct, whole or in
      // halves around the `break` — it compiled to other code, 29 to 136 of the file's kernels, with other scratch offsets.)
      const unsigned long long live = __ballot(alive);
      if (lane == 0) wave_cnt[wave] = static_cast<uint32_t>(__builtin_popcountll(live));
      __syncthreads();
      uint32_t base = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kPtRows; w++) {
        const uint32_t c = wave_cnt[w];
        if (w < wave) base += c;
        total += c;
      }
      if (total == 0) break;  // block-uniform
      if (alive) {
        const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(live >> 32),
                                                              __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(live), 0u));
        uint32_t word = pix;  // pix has 8 bits: the path's sampled bit travels with it, and the sphere bit beside that
        if constexpr (spec_lights(SPEC)) word |= nee.sampled ? 0x100u : 0u;
        if constexpr (spec_sphere(SPEC)) word |= nee.sphere ? 0x200u : 0u;
        if constexpr (spec_mis(SPEC)) {
          if (nee.sampled) cb_pix[pix] = nee.cb;  // by pixel: one path per pixel is live
        }
        st.pix[slot] = word;
        st.rng[slot] = rng;
        st.ox[slot] = o.x; st.oy[slot] = o.y; st.oz[slot] = o.z;
        st.dx[slot] = d.x; st.dy[slot] = d.y; st.dz[slot] = d.z;
        st.ar[slot] = acc.x; st.ag[slot] = acc.y; st.ab[slot] = acc.z;
      }
      __syncthreads();
      alive = static_cast<uint32_t>(tid) < total;
      if (alive) {
        pix = st.pix[tid];
        if constexpr (spec_lights(SPEC)) {
          nee.sampled = (pix & 0x100u) != 0u;
          if constexpr (spec_sphere(SPEC)) nee.sphere = (pix & 0x200u) != 0u;
          pix &= 0xFFu;
          if constexpr (spec_mis(SPEC)) {
            if (nee.sampled) nee.cb = cb_pix[pix];
          }
        }
        rng = st.rng[tid];
        o = f3{st.ox[tid], st.oy[tid], st.oz[tid]};
        d = f3{st.dx[tid], st.dy[tid], st.dz[tid]};
        acc = f3{st.ar[tid], st.ag[tid], st.ab[tid]};
      }
      // BVH: the traversal's node stack aliases the exchange buffer, so everybody must have read its slot before any
      // wave walks on.  Brute force: nothing writes the buffer before the NEXT compaction's first barrier, which every
      // thread reaches only after these reads — a third barrier per segment would only hold the fast waves back.
      if (BVH) __syncthreads();
    }
    if (a.seg_end < a.max_segments) {  // only with spp == 1: the unfinished paths continue in a queue kernel
      const uint32_t pixg = (static_cast<uint32_t>(tile_y0 + static_cast<int>(pix >> 6)) << 16) |
                            static_cast<uint32_t>(tile_x0 + static_cast<int>(pix & 63u));
      const uint32_t blk = tile_lin<ROLE>(role_lin);
      enqueue_paths(a, blk % kPathQueues, wave_cnt, &q_base, alive, wave, lane, pixg, rng, o, d, acc);
    }
  }
  __syncthreads();
  if (a.spp > 1) {
    const int x = tile_x0 + static_cast<int>(lane), y = tile_y0 + wave;
    if (x < a.g.W && y < a.g.y1) {
      const float ns = static_cast<float>(a.spp);
      const size_t gi = static_cast<size_t>(y - a.g.row_base) * a.g.W + x;
      if (GB)
        store_rgb(a.image + gi, f3{sum_r[tid] / ns, sum_g[tid] / ns, sum_b[tid] / ns});
      else
        a.image[gi] = make_float4(sum_r[tid] / ns, sum_g[tid] / ns, sum_b[tid] / ns, a.depth[gi]);  // :328,:343
    }
  }
  add_block_rays(a, rays, &block_rays, tid, tile_lin<ROLE>(role_lin));
}

// A run of `rows` vertically consecutive tiles, from tile row `row0` on, of tile column `bx` that no triangle's screen bounds
// reach (final_split.hpp: final_full_columns; a.cull holds, one sample per pixel): the workgroup of k_pathtrace_final that serves
// them all.  Every path of such a tile ends at its first query, on the light or in the sky, so of pathtrace_tile only the
// primary segment is left: no candidate set, no closest hit (it would find id 0), no compaction, no path state in LDS, no
// hand-over to a queue (nothing survives), and the loop has no barrier.  The ray count goes out once per workgroup.  A wave
// takes a row of a tile, lane = column: the image does not depend on which lane traces a pixel.
// The primary ray restates pathtrace_tile's, statement for statement, as compact_paths is restated in k_pathtrace_queue: as a
// function of both it compiled the other tracing kernels to other code.  tests/test_empty_runs_gpu.py asks for the bits of a
// context without runs.
// block_rays: an LDS word of the caller's, nothing else of the workgroup's LDS is touched.
__device__ __forceinline__ void pathtrace_empty_run(const PathtraceArgs& a, uint32_t bx, uint32_t row0, uint32_t rows, uint32_t slot,
                                                    unsigned int* block_rays) {
  const int tid = threadIdx.y * kBlockX + threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.y));
  if (tid == 0) *block_rays = 0;
  const float fw = static_cast<float>(a.g.W), fh = static_cast<float>(a.g.H);
  const f3 light_c = ld3(a.light_c);
  const int px0 = static_cast<int>(bx) * kBlockX + static_cast<int>(threadIdx.x);
  unsigned int rays = 0;
  if (px0 < a.g.W && a.seg_end > 0) {
    for (uint32_t r = 0; r < rows; r++) {
      const int py0 = a.g.y0 + static_cast<int>(row0 + r) * kPtRows + wave;
      if (py0 >= a.g.y1) break;  // (wave-uniform: the frame's last tile row)
      const size_t gi = static_cast<size_t>(py0 - a.g.row_base) * a.g.W + px0;
      const float depth = a.depth[gi];
      uint32_t rng = exact::rng_seed(static_cast<uint32_t>(px0), static_cast<uint32_t>(py0), a.frame, a.batch);  // :297
      float u1 = glsl_max(1e-38f, exact::rng_next(rng));  // :87 Box-Muller
      float u2 = exact::rng_next(rng);
      float rad = exact::sqrt_(-2.0f * exact::log_(u1));
      float sn, cs;
      exact::sincos2pi(u2, sn, cs);
      float cx = fmaf_(a.jitter, rad * cs, static_cast<float>(px0) + 0.5f);  // :314
      float cy = fmaf_(a.jitter, rad * sn, static_cast<float>(py0) + 0.5f);
      float ux = RTPT_DIV_SH(fmaf_(2.0f, cx, -fw), fh);     // :315
      float uy = -RTPT_DIV_SH(fmaf_(2.0f, cy, -fh), fh);  // :316
      const f3 d = exact::normalize(f3{a.slope * ux, a.slope * uy, -1.0f});  // :319-320
      const f3 o = ld3(a.cam);
      f3 acc{1.f, 1.f, 1.f};  // :201
      if (py0 >= a.count_y0 && py0 < a.count_y1) rays++;
      if (a.hit_id) a.hit_id[gi] = 0u;
      if (ray_hits_light(o, d, light_c, a.light_r2))  // :226
        acc = acc * ld3(a.light_col_first);            // :229
      else
        acc = acc * sky_color(d);                      // :266
      a.image[gi] = make_float4(acc.x, acc.y, acc.z, depth);  // :328,:343
    }
  }
  __syncthreads();  // block_rays is zero before the first wave adds to it
  add_block_rays(a, rays, block_rays, tid, slot);
}

// K0 + K1 + K2 in one launch, the body of k_gbuffer_pathtrace and k_gbuffer_pathtrace_small (kernels.hip has the reasons): rows
// [0, a.tiles_y) of the grid are the tracing tiles, the rows behind them the G-buffer's 64 x 4 tiles, which put their depth into
// the alpha of the traced image's pixels
template <int BVH, bool DEMOD, int TEX, int SPEC, class... LV>
__device__ __forceinline__ void gbuffer_pathtrace_body(const PathtraceArgs& a, const GbufferArgs& g, const TexView& tex, const LV&... lights) {
  if (blockIdx.y < a.tiles_y) {
    pathtrace_tile<BVH, true, true, DEMOD, TEX, SPEC>(a, tex, 0, 0, 0, lights...);
  } else {
    extern __shared__ __attribute__((aligned(16))) uint32_t stack[];
#if RTPT_TILE_TIMELINE
    TimelineScope tl_(0, (blockIdx.y - a.tiles_y) * gridDim.x + blockIdx.x);
#endif
    if constexpr (pack_nrm<LV...>())  // the scene's NormalView: K0 writes the guide normal while its switch is set (gbuffer_tile.hpp)
      gbuffer_tile<BVH>(g, blockIdx.x, blockIdx.y - a.tiles_y, stack, a.image, a.g.y0, a.g.y1, pack_get<NormalView>(lights...));
    else
      gbuffer_tile<BVH>(g, blockIdx.x, blockIdx.y - a.tiles_y, stack, a.image, a.g.y0, a.g.y1);
  }
}

// the two kernels of the tile body (kernels.hip): the wave-uniform brute-force one is pinned at 8 waves per SIMD (kPtWaves), the BVH one
// is LDS-limited anyway and loses 4 % to the scalar spills the pin costs (1.15M-triangle trace 3.69 -> 3.85 ms)
// The BVH variant waits on memory for most of its wave-cycles and is that sensitive to occupancy (kernels.hpp
// SceneView::stack_lds); with the stack's LDS share cut to 16 entries the registers set the limit.  1.15M-triangle trace,
// 5 waves per SIMD (the compiler's 79 VGPRs and the old 30 KB stack) 3.69 ms; pinned at 6 / 7 / 8: 3.93 / 3.55 / 3.36 ms
// (at 8: 64 VGPRs and 8 dwords of scratch per lane).
constexpr int kPtBvhWaves = 8;

}  // namespace
}  // namespace rt
