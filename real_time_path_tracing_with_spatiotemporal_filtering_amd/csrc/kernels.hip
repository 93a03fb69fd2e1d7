// kernels.hip — the entry points of the frame's hand-written gfx950 (CDNA4, wave64) kernels K0 to K2, and their launchers.
//
//   k_scene_prepare / k_lut   per-triangle records, LUT (visibility.geom.glsl:44-59), normal table
//   k_gbuffer                 K0  visibility.{vert,geom,frag}.glsl as pixel-centre primary rays     (gbuffer_tile.hpp)
//   k_gradient                K1  temporalGradient.comp.glsl:104-172                                 (gbuffer_tile.hpp)
//   k_pathtrace*, k_gbuffer_pathtrace*, k_pathtrace_final, k_pathtrace_queue
//                             K2  raytrace.comp.glsl:273-344 (software closest-hit, no ray query)    (pathtrace_tile.hpp,
//                                 shade_segment.hpp, closest_hit.hpp)
// (K3, temporalFiltering.comp.glsl:191-265, is atrous.hip / atrous_chain.hip; the self-test kernels are selftest_kernels.hip.)
//
// The device code lives in the headers; what stays here is every __global__ of the frame, in ONE translation unit, because
//   * the fused launches put K0 + K1 and K2 bodies (k_gbuffer_pathtrace*), and a K2 and a K3 body (k_pathtrace_final), into one kernel;
//   * every kernel that uses dynamic LDS declares the same array, `stack`, and a translation unit has one such symbol: its
//     alignment, and with it the byte the array starts at behind a kernel's static LDS, is that of the declaration emitted first.
//     That is k_gbuffer's, which states none, because launch_gbuffer instantiates it before launch_pathtrace instantiates the
//     tracing kernels (whose declarations say aligned(16)): `stack` starts at byte 24 of the tracing kernels' LDS.  Compiled
//     without k_gbuffer and k_gradient, 189 of the other 194 kernels change: .amdhsa_group_segment_fixed_size 24 -> 32 and the
//     matching immediates, 8 more bytes of LDS per workgroup in kernels whose occupancy is tuned to the byte.  A pathtrace.hip
//     of its own costs that (or a realigned array, measured again); scripts/device_asm_diff.py --by-kernel shows it without a GPU;
//   * the profiling builds' device globals (g_tile_order, g_timeline, TimelineScope: experiments/trace_instrumentation.inc)
//     are read and written by K0 and K2 workgroups alike and by the host functions at the end of this file.
//
// No MFMA anywhere: nothing on this path is a dense contraction.  Compile with -ffp-contract=off.
#include <cstdlib>

#include "atrous_comb.hpp"
#include "final_split.hpp"
#include "pathtrace_tile.hpp"
#include "select.hpp"
#include "tile_kernels.hpp"

namespace rt {
namespace {

// ------------------------------------------------------------------------------------------
// scene records
// ------------------------------------------------------------------------------------------
__global__ void k_scene_prepare(ScenePrepArgs a) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n_tris) return;
  {
    const float* t = a.tris + 9 * static_cast<size_t>(i);
    f3 v0 = ld3(t), v1 = ld3(t + 3), v2 = ld3(t + 6);
    f3 e1 = v1 - v0, e2 = v2 - v0;
    f3 nn = exact::cross(e1, e2);
    a.isect_id[3 * i] = make_float4(v0.x, v0.y, v0.z, e1.x);
    a.isect_id[3 * i + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
    a.isect_id[3 * i + 2] = make_float4(e2.z, nn.x, nn.y, nn.z);
    f3 n = exact::normalize(nn);  // raytrace.comp.glsl:150
    a.shade[3 * i] = make_float4(v0.x, v0.y, v0.z, n.x);
    a.shade[3 * i + 1] = make_float4(v1.x, v1.y, v1.z, n.y);
    a.shade[3 * i + 2] = make_float4(v2.x, v2.y, v2.z, n.z);
  }
  if (!a.leaf_pairs) {
    uint32_t id = a.leaf_order[i];  // leaf slot i holds triangle id (ids stay in leaf_order)
    const float* t = a.tris + 9 * static_cast<size_t>(id);
    f3 v0 = ld3(t), v1 = ld3(t + 3), v2 = ld3(t + 6);
    f3 e1 = v1 - v0, e2 = v2 - v0;
    f3 nn = exact::cross(e1, e2);
    a.isect_leaf[3 * i] = make_float4(v0.x, v0.y, v0.z, e1.x);
    a.isect_leaf[3 * i + 1] = make_float4(e1.y, e1.z, e2.x, e2.y);
    a.isect_leaf[3 * i + 2] = make_float4(e2.z, nn.x, nn.y, nn.z);
  } else if (!(i & 1u) && i + 1 < a.n_tris) {
    // leaf slots (i, i + 1) hold the two triangles A = (a, b, c), B = (a, c, d) of one fan pair: one 80-byte record, each
    // triangle's edges and plane normal computed exactly as for its own 48-byte record (SceneView::isect_leaf)
    const uint32_t ia = a.leaf_order[i], ib = a.leaf_order[i + 1];
    const float* ta = a.tris + 9 * static_cast<size_t>(ia);
    const float* tb = a.tris + 9 * static_cast<size_t>(ib);
    const f3 v0 = ld3(ta), e1 = ld3(ta + 3) - v0, e2 = ld3(ta + 6) - v0, nn = exact::cross(e1, e2);
    const f3 v0b = ld3(tb), e1b = ld3(tb + 3) - v0b, e2b = ld3(tb + 6) - v0b, nb = exact::cross(e1b, e2b);
    float4* r = a.isect_leaf + 5 * static_cast<size_t>(i >> 1);
    r[0] = make_float4(v0.x, v0.y, v0.z, e1.x);
    r[1] = make_float4(e1.y, e1.z, e2.x, e2.y);
    r[2] = make_float4(e2.z, nn.x, nn.y, nn.z);
    r[3] = make_float4(e2b.x, e2b.y, e2b.z, nb.x);
    r[4] = make_float4(nb.y, nb.z, u2f(ia), u2f(ib));
  }
}

// visibility.vert.glsl:24 + visibility.geom.glsl:57-59: LUT[t+1] = model * (v0,v1,v2), written for
// every triangle (the geometry stage precedes clipping).  Also the per-id normal table the filter
// gathers instead of re-deriving normalize(cross) from the LUT at each of its 10 reads per pixel
// (temporalFiltering.comp.glsl:80-91) — same values, computed once per triangle.
__global__ void k_lut(LutArgs a) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {
    a.lut[0] = a.lut[1] = a.lut[2] = make_float4(0.f, 0.f, 0.f, 0.f);
    f3 n{0.f, 0.f, 1.f};  // temporalFiltering.comp.glsl:83
    a.normal_tab[0] = make_float4(n.x, n.y, n.z, exact::powi(glsl_max(0.0f, exact::dot(n, n)), a.sigma_n));
    a.area_tab[0] = make_float4(0.f, 0.f, 0.f, 0.f);  // never read: id 0 has no triangle (temporalGradient.comp.glsl:128-131)
  }
  if (t >= a.n_tris) return;
  f3 v[3];
  for (int k = 0; k < 3; k++) {
    f3 p = xyz(a.shade[3 * t + k]);
    v[k] = f3{exact::mat_row_point(a.model, 0, p), exact::mat_row_point(a.model, 1, p), exact::mat_row_point(a.model, 2, p)};
    a.lut[3 * (t + 1) + k] = make_float4(v[k].x, v[k].y, v[k].z, 0.f);
  }
  f3 n = exact::normalize(exact::cross(v[1] - v[0], v[2] - v[0]));  // :90
  a.normal_tab[t + 1] = make_float4(n.x, n.y, n.z, exact::powi(glsl_max(0.0f, exact::dot(n, n)), a.sigma_n));
  a.area_tab[t + 1] = make_float4(tri_area(v[0], v[1], v[2]), 0.f, 0.f, 0.f);  // temporalGradient.comp.glsl:60, once per triangle
}

// pow(max(0, dot(n_p, n_q)), sigma_n) for every id pair (temporalFiltering.comp.glsl:62), small scenes
__global__ void k_pair_weights(LutArgs a) {
  const uint32_t np = a.n_tris + 1;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= np * np) return;
  const uint32_t p = i / np, q = i - p * np;
  const f3 n_p = xyz(a.normal_tab[p]), n_q = xyz(a.normal_tab[q]);
  a.pair_tab[i] = exact::powi(glsl_max(0.0f, exact::dot(n_p, n_q)), a.sigma_n);
}

// ------------------------------------------------------------------------------------------
// K0 G-buffer, K1 temporal gradient
// ------------------------------------------------------------------------------------------
// dvx[x] = ((2 (x + .5) - W) / W) / P00 for every column, dvy[y] likewise for every frame row (see k_gbuffer)
__global__ void k_ray_tables(int W, int H, float p00, float p11, float* dvx, float* dvy) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < W) {
    const float fw = static_cast<float>(W);
    dvx[i] = (fmaf_(2.0f, static_cast<float>(i) + 0.5f, -fw) / fw) / p00;
  }
  if (i < H) {
    const float fh = static_cast<float>(H);
    dvy[i] = (fmaf_(2.0f, static_cast<float>(i) + 0.5f, -fh) / fh) / p11;
  }
}

// NV: nothing, or the scene's NormalView while RTPT_FLAG_EXT_SMOOTH_GUIDE is active (kernels.hpp; the two BVH modes only)
template <int BVH, class... NV>
__global__ __launch_bounds__(kThreads) void k_gbuffer(GbufferArgs a, NV... normals) {
  static_assert(sizeof...(NV) == 0 || (sizeof...(NV) == 1 && pack_nrm<NV...>() && BVH != 0), "a NormalView or nothing");
  extern __shared__ uint32_t stack[];  // BVH: stack_depth x 256 entries (dynamic); unused otherwise
#if RTPT_TILE_TIMELINE
  TimelineScope tl_(0, blockIdx.y * gridDim.x + blockIdx.x);
#endif
  if constexpr (sizeof...(NV) != 0)
    gbuffer_tile<BVH>(a, blockIdx.x, blockIdx.y, stack, nullptr, 0, 0, normals...);
  else
    gbuffer_tile<BVH>(a, blockIdx.x, blockIdx.y, stack);
}

__global__ __launch_bounds__(kThreads) void k_gradient(GradientArgs a) {
  const int x = blockIdx.x * kBlockX + threadIdx.x;
  const int y = a.g.y0 + blockIdx.y * kBlockY + threadIdx.y;
  if (x >= a.g.W || y >= a.g.y1) return;  // D10: bounds check first
  const size_t i = static_cast<size_t>(y - a.g.row_base) * a.g.W + x;
  const uint32_t id = a.vis[i];
  const f3 wp = id ? xyz(a.worldpos[i]) : f3{0.f, 0.f, 0.f};
  store_gradient(a.grad, i, gradient_lambda(id, wp, a.lut, a.lut_prev, a.normal_tab, a.area_tab, ld3(a.cam), ld3(a.light), ld3(a.light_prev), ld3(a.color),
                                            ld3(a.color_prev)));
}

// K2 of frame n + 1 and the final filter pass of frame n in one launch (api_passes.hip: DeferredFinal).  The trace is bound by VALU
// issue and touches next to no memory, the final pass by HBM; neither reads what the other writes (DESIGN §4 has the table), and
// as launches of their own they never share the machine.  One grid, three runs of workgroups in dispatch order (final_split.hpp
// states the layout and the role of a workgroup, once): sp.n_front filter workgroups, which run beside the body of the trace; the
// tracing tiles; sp.n_tail filter workgroups, which start as the last tiles drain (none by default: the front group owns the
// whole list).  The filter workgroups are the comb kernel's (atrous_comb.hpp: comb_items); the front group owns the first
// sp.front_items items of the list and the tail group the rest, so every item has one owner and no workgroup waits for another.
// Between the tiles and the tail group: the run workgroups (sp.n_runs), which serve the tile columns at the end of the dispatch
// order that no triangle's bounds reach, sp.run_len tiles each (pathtrace_tile.hpp: pathtrace_empty_run).
// The launch's dynamic LDS is the larger of the two bodies': a staged row of kFinalRoleCw cells keeps it at 8 workgroups per CU.
// Only the pass that loads its reprojected pixels (RLOAD) is instantiated: at this kernel's 64 VGPRs it needs no scratch, the
// reprojecting pass would spill 48 registers per lane — it runs as the launch of its own (atrous_final_role).
// (CW, the staged row: a template like every other user of the dynamic LDS array `stack`, so that the array is still first
// emitted through k_gbuffer's declaration — a plain kernel here comes first and hands its 16-byte alignment to the one symbol
// all of them share, which moves the dynamic LDS of every kernel of this file from byte 24 to 32)
template <int CW>
__global__ __launch_bounds__(kPtThreads)
__attribute__((amdgpu_waves_per_eu(kPtWaves, kPtWaves)))
void k_pathtrace_final(PathtraceArgs a, TexView tex, AtrousArgs f, FinalSplit sp) {
  static_assert(kPtThreads == kShThreads && kPtRows == kShWaves, "the two bodies share the workgroup shape");
  const FinalRole r = final_role(sp, blockIdx.x);
  if (r.role == kFinalRoleTile) {
    pathtrace_tile<0, true, false, false, 0, 0, 1>(a, tex, r.index, sp.tiles_x, a.tiles_y);
  } else if (r.role == kFinalRoleRun) {
    // the columns behind the last one a triangle's bounds reach, a run of tiles per workgroup (final_split.hpp, pathtrace_tile.hpp)
    extern __shared__ __attribute__((aligned(16))) unsigned char final_lds[];
#if RTPT_TILE_TIMELINE
    FilterTimelineScope tl_(r.role, sp.n_front + sp.n_tail + r.index);
#endif
    const FinalRun run = final_run(sp, r.index);
    pathtrace_empty_run(a, run.column, run.row0, run.rows, sp.n_tiles + r.index, reinterpret_cast<unsigned int*>(final_lds));
  } else {
    extern __shared__ __attribute__((aligned(16))) unsigned char final_lds[];
    const bool front = r.role == kFinalRoleFront;
#if RTPT_TILE_TIMELINE
    FilterTimelineScope tl_(r.role, front ? r.index : sp.n_front + r.index);
#endif
    comb_items<CW, true, false, false, 1, false, false, true, true>(f, final_lds, r.index, front ? sp.n_front : sp.n_tail,
                                                                       front ? 0u : sp.front_items, front ? sp.front_items : sp.items);
  }
}

// NV: nothing, or the scene's NormalView (kernels.hpp: the NRM axis).  The queue record does not change: a shading normal belongs to
// a hit, not to a path.
template <int BVH, int TEX, int SPEC, class... NV>
__global__ __launch_bounds__(kPtThreads) void k_pathtrace_queue(PathtraceArgs a, TexView tex, NV... normals) {
  static_assert(sizeof...(NV) == 0 || (sizeof...(NV) == 1 && pack_nrm<NV...>()), "a NormalView or nothing");
  extern __shared__ __attribute__((aligned(16))) uint32_t stack[];
  PathState& st = *reinterpret_cast<PathState*>(stack);
  __shared__ uint32_t wave_cnt[kPtRows];
  __shared__ uint32_t q_base;
  __shared__ unsigned int block_rays;
  const int tid = threadIdx.y * kBlockX + threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.y));
  const uint32_t lane = threadIdx.x;
  if (tid == 0) block_rays = 0;
  const f3 light_c = ld3(a.light_c);
  // workgroup b serves region b mod kPathQueues, every (gridDim.x / kPathQueues)-th chunk of 256 records
  const uint32_t region = blockIdx.x % kPathQueues;
  const uint32_t n_in = a.q_in_count[region];
  const size_t region_base = static_cast<size_t>(region) * a.queue_region;
  unsigned int rays = 0;
  for (uint32_t base = (blockIdx.x / kPathQueues) * kPtThreads; base < n_in; base += (gridDim.x / kPathQueues) * kPtThreads) {  // block-uniform
    uint32_t pix = 0, rng = 0;
    f3 o{0.f, 0.f, 0.f}, d{0.f, 0.f, -1.f}, acc{1.f, 1.f, 1.f};
    bool alive = base + static_cast<uint32_t>(tid) < n_in;
    if (alive) {
      const float4* q = reinterpret_cast<const float4*>(a.q_in) + 3 * (region_base + base + tid);
      const float4 q0 = q[0], q1 = q[1], q2 = q[2];
      pix = __float_as_uint(q0.x);
      rng = __float_as_uint(q0.y);
      o = f3{q0.z, q0.w, q1.x};
      d = f3{q1.y, q1.z, q1.w};
      acc = f3{q2.x, q2.y, q2.z};
    }
    for (uint32_t seg = a.seg_begin; seg < a.seg_end; seg++) {
      if (alive) {
        HitRec h{a.tmax, 0u, 0.f, 0.f, 1.f};
        closest_hit<BVH>(a.scene, o, d, h, stack, tid, kPtThreads, 1 + static_cast<int>(seg));  // :208-222
        const int x = static_cast<int>(pix & 0xFFFFu), y = static_cast<int>(pix >> 16);
        if (y >= a.count_y0 && y < a.count_y1) rays++;
        bool done;
        if constexpr (sizeof...(NV) != 0)
          done = shade_segment<TEX, BVH, (RTPT_TRACE_ITEMS & 8) && BVH == 0, SPEC, NoNee, NormalView>(a, h, seg, light_c, o, d, acc, rng, tex, nullptr, NoNee{},
                                                                                                      normals...);
        else
          done = shade_segment<TEX, BVH, (RTPT_TRACE_ITEMS & 8) && BVH == 0, SPEC>(a, h, seg, light_c, o, d, acc, rng, tex);
        if (done) {
          alive = false;
          const size_t gi = static_cast<size_t>(y - a.g.row_base) * a.g.W + x;
          a.image[gi] = make_float4(acc.x, acc.y, acc.z, a.depth[gi]);  // :328,:343 (+ depth in alpha)
        }
      }
      if (seg + 1 >= a.seg_end) break;
      // compact the survivors to the front of the block (as in pathtrace_tile)
      const unsigned long long live = __ballot(alive);
      if (lane == 0) wave_cnt[wave] = static_cast<uint32_t>(__builtin_popcountll(live));
      __syncthreads();
      uint32_t cbase = 0, total = 0;
#pragma unroll
      for (int w = 0; w < kPtRows; w++) {
        const uint32_t c = wave_cnt[w];
        if (w < wave) cbase += c;
        total += c;
      }
      if (total == 0) break;  // block-uniform
      if (alive) {
        const uint32_t slot = cbase + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(live >> 32),
                                                              __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(live), 0u));
        st.pix[slot] = pix;
        st.rng[slot] = rng;
        st.ox[slot] = o.x; st.oy[slot] = o.y; st.oz[slot] = o.z;
        st.dx[slot] = d.x; st.dy[slot] = d.y; st.dz[slot] = d.z;
        st.ar[slot] = acc.x; st.ag[slot] = acc.y; st.ab[slot] = acc.z;
      }
      __syncthreads();
      alive = static_cast<uint32_t>(tid) < total;
      if (alive) {
        pix = st.pix[tid];
        rng = st.rng[tid];
        o = f3{st.ox[tid], st.oy[tid], st.oz[tid]};
        d = f3{st.dx[tid], st.dy[tid], st.dz[tid]};
        acc = f3{st.ar[tid], st.ag[tid], st.ab[tid]};
      }
      if (BVH) __syncthreads();  // the node stack aliases the exchange buffer (see pathtrace_tile)
    }
    if (a.seg_end < a.max_segments) enqueue_paths(a, region, wave_cnt, &q_base, alive, wave, lane, pix, rng, o, d, acc);
    __syncthreads();  // wave_cnt / st are reused by the next chunk
  }
  add_block_rays(a, rays, &block_rays, tid, blockIdx.x);
}

#ifndef RTPT_AB_VARIANTS
#define RTPT_AB_VARIANTS 0
#endif
#if RTPT_AB_VARIANTS
#include "experiments/pathtrace_pool.inc"
#endif

}  // namespace

#if RTPT_BVH_COUNT || RTPT_TILE_TIMELINE
#define RTPT_INSTR_HOST
#include "experiments/trace_instrumentation.inc"
#undef RTPT_INSTR_HOST
#endif

void launch_scene_prepare(const ScenePrepArgs& a, hipStream_t s) {
  if (!a.n_tris) return;
  hipLaunchKernelGGL(k_scene_prepare, dim3((a.n_tris + 255) / 256), dim3(256), 0, s, a);
}
void launch_lut(const LutArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_lut, dim3((a.n_tris + 256) / 256), dim3(256), 0, s, a);
  if (a.pair_tab) {
    const uint32_t n = (a.n_tris + 1) * (a.n_tris + 1);
    hipLaunchKernelGGL(k_pair_weights, dim3((n + 255) / 256), dim3(256), 0, s, a);
  }
}
void launch_ray_tables(int W, int H, float p00, float p11, float* dvx, float* dvy, hipStream_t s) {
  const int n = W > H ? W : H;
  hipLaunchKernelGGL(k_ray_tables, dim3((n + 255) / 256), dim3(256), 0, s, W, H, p00, p11, dvx, dvy);
}
void launch_gbuffer(const GbufferArgs& a, hipStream_t s, const NormalView& normals) {
  if (a.g.y1 <= a.g.y0) return;
  const bool guide = normals.guide != 0u;  // RTPT_FLAG_EXT_SMOOTH_GUIDE is active: a scene with normals, traced through its tree
  if (guide && (!normals.records || !normals.cof || !a.scene.use_bvh || !a.normals)) std::abort();
  with_mode<3>(scene_mode(a.scene), [&](auto mode) {
    constexpr int M = decltype(mode)::value;
    if constexpr (M != 0) {
      if (guide) {  // (the launch syntax: launch_pathtrace's `go` says why)
        k_gbuffer<M><<<grid_for(a.g), dim3(kBlockX, kBlockY), a.scene.stack_lds * kThreads * 4, s>>>(a, normals);
        return;
      }
    }
    k_gbuffer<M><<<grid_for(a.g), dim3(kBlockX, kBlockY), M ? a.scene.stack_lds * kThreads * 4 : 0, s>>>(a);
  });
}
void launch_gradient(const GradientArgs& a, hipStream_t s) {
  if (a.g.y1 <= a.g.y0) return;
  hipLaunchKernelGGL(k_gradient, grid_for(a.g), dim3(kBlockX, kBlockY), 0, s, a);
}
bool pathtrace_fuses_gbuffer(const PathtraceArgs& a, const GbufferArgs& g) {
  // the G-buffer's rows must contain the traced ones (the depth in the traced image's alpha comes from them) and the two
  // workgroup shapes must agree (they share the launch)
  return a.compact && a.spp >= 1 && g.g.y0 <= a.g.y0 && g.g.y1 >= a.g.y1 && a.g.y1 > a.g.y0 && kPtRows == kBlockY;
}
// the path-pool form of the tile kernel (experiments/pathtrace_pool.inc, -DRTPT_AB_VARIANTS=1 builds only) serves scenes whose
// BVH is built over fan pairs, one sample per pixel
#if RTPT_AB_VARIANTS
bool pathtrace_uses_pool(const PathtraceArgs& a) {  // (a launch that samples lights gets no slab: ensure_path_pool)
  return a.pool_slab && a.scene.use_bvh && a.scene.leaf_pairs && a.compact && a.spp == 1;
}
size_t pathtrace_pool_bytes(int W, int rows) {  // slabs of the tracing workgroups of a launch over `rows` rows
  return static_cast<size_t>((W + kBlockX - 1) / kBlockX) * ((rows + kPoolRows - 1) / kPoolRows) * (7u * kPoolPaths * sizeof(float4));
}
#else
constexpr int kPoolRows = kPtRows;
bool pathtrace_uses_pool(const PathtraceArgs&) { return false; }
size_t pathtrace_pool_bytes(int, int) { return 0; }
#endif
bool pathtrace_takes_final(const PathtraceArgs& a, const TexView& tex, int specular) {
  return !a.scene.use_bvh && a.compact && a.spp == 1 && !a.albedo && !tex.records && !specular && !pathtrace_uses_pool(a) && a.g.y1 > a.g.y0;
}
uint32_t pathtrace_grid_blocks(const PathtraceArgs& a, const GbufferArgs* gb) {
  const uint32_t gx = (a.g.W + kBlockX - 1) / kBlockX;
  const int tr = pathtrace_uses_pool(a) ? kPoolRows : kPtRows;
  return gx * ((a.g.y1 - a.g.y0 + tr - 1) / tr + (gb ? (gb->g.y1 - gb->g.y0 + kBlockY - 1) / kBlockY : 0));
}
// the filter workgroups of a launch that carries the final pass `f` (atrous_final_role finished it): how many in front of and
// behind the tiles, and where the work list is cut between them (final_split.hpp)
// ... and which columns of the tile order are served in runs: those behind the last one that a triangle's bounds reach, when the
// launch has bounds (a.cull) and traces at least the primary segment
static FinalSplit final_split(const PathtraceArgs& a, const AtrousArgs& f, const FilterPolicy& pol, uint32_t tiles_x, uint32_t tiles_y) {
  const uint32_t n_cu = a.n_cu > 0 ? static_cast<uint32_t>(a.n_cu) : 256u;
  const uint32_t per_cu = static_cast<uint32_t>(kPtWaves * 4 / kShWaves);  // resident workgroups of either kind
  const uint32_t items = static_cast<uint32_t>(f.tiles_x) * static_cast<uint32_t>(f.tiles_y) * static_cast<uint32_t>(f.stride);
  static_assert(kTileColumnPixels == kBlockX, "final_full_columns and the tile kernel agree on a column");
  const bool runs = pol.empty_run > 0 && a.cull && a.max_segments > 0;
  const uint32_t full_cols = runs ? final_full_columns(a.bounds, a.scene.n_tris, a.g.W, a.g.y0, a.g.y1, tiles_x) : tiles_x;
  return final_split_plan(items, tiles_x, tiles_y, n_cu, per_cu, pol.final_front, pol.final_front_share, full_cols,
                          runs ? static_cast<uint32_t>(pol.empty_run) : 0u);
}
void launch_pathtrace(const PathtraceArgs& a, const GbufferArgs* gb, const TexView& tex, int specular, hipStream_t s, const AtrousArgs* fin,
                      const FilterPolicy* pol, uint32_t* run_info, const LightTableView& lights, const NormalView& normals, const EnvView& envmap) {
  if (run_info) {
    run_info[0] = a.g.y1 > a.g.y0 ? static_cast<uint32_t>((a.g.W + kBlockX - 1) / kBlockX) : 0u;
    run_info[1] = run_info[2] = 0u;
  }
  if (a.g.y1 <= a.g.y0) return;
  dim3 block(kBlockX, kPtRows);
  const int spec = spec_mode(specular);
  const bool nee = spec_lights(spec);  // the launch samples lights: every segment runs in the tile kernels
  // (api_passes.hip: trace_material_mode) the triangles of a list are sampled from a list with entries, on a scene with materials:
  // where the sphere light is sampled without the weighted pick the list may be empty, everywhere else it is not
  const bool may_be_empty = spec_may_be_empty(spec);  // (never a launch that weighs its samples: spec_mis)
  if (nee && !may_be_empty && (!lights.ids || !lights.n || !a.scene.materials)) std::abort();
  if (nee && may_be_empty && lights.n && (!lights.ids || !a.scene.materials)) std::abort();
  if (spec_power(spec) && !lights.cdf) std::abort();  // the weighted pick reads the list's table
  // rtpt_scene_set_normals: the scene is traced through its tree by a compacting launch (api_scene.hip, api_passes.hip see to both)
  const bool nrm = normals.records != nullptr;
  if (nrm && (!normals.cof || !a.scene.use_bvh || (!gb && !a.compact) || fin)) std::abort();
  // rtpt_set_environment: the launch is fused or compacts and carries no final pass (api_context.hip, api_passes.hip see to both)
  const bool envl = envmap.texels != nullptr;
  if (envl && (!envmap.n || envmap.n > 4096u || (!gb && !a.compact) || fin)) std::abort();
  const bool pool = !nee && !nrm && !envl && pathtrace_uses_pool(a);  // never with textures: ensure_path_pool (api_passes.hip) hands out no slab then
  const int tile_rows = pool ? kPoolRows : kPtRows;
  const uint32_t tiles_y = (a.g.y1 - a.g.y0 + tile_rows - 1) / tile_rows;
  const dim3 grid((a.g.W + kBlockX - 1) / kBlockX, tiles_y + (gb ? (gb->g.y1 - gb->g.y0 + kBlockY - 1) / kBlockY : 0), 1);
  const size_t stack_bytes = a.scene.use_bvh ? static_cast<size_t>(a.scene.stack_lds) * kPtThreads * 4 : 0;
  size_t dyn = stack_bytes > sizeof(PathState) ? stack_bytes : sizeof(PathState);  // shared by both tenants
  if (fin) {  // (api_passes.hip asked pathtrace_takes_final and atrous_final_role: no G-buffer workgroups, one sample, no BVH)
    if (gb || !pol || !fin->reproj_in || !pathtrace_takes_final(a, tex, specular)) std::abort();
    dyn = dyn > final_role_lds(*fin) ? dyn : final_role_lds(*fin);
  }
  PathtraceArgs b = a;
  b.tiles_y = tiles_y;
  b.multi_off = static_cast<uint32_t>(dyn / 4);
  const size_t dyn_queue = dyn;
  if (nee) dyn += 3 * kPtThreads * 4;        // rad_r, rad_g, rad_b (pathtrace_tile), in front of the sums
  if (spec_mis(spec)) dyn += kPtThreads * 4;  // cb_pix behind them, for the instantiations of RTPT_FLAG_EXT_NEE_MIS only
  if (a.spp > 1) dyn += 4 * kPtThreads * 4;  // sum_r, sum_g, sum_b, rng_pix
  const uint32_t phase0 = a.first_window ? a.first_window : pt_first_window(a.scene.use_bvh != 0);
  const bool split = !nee && !envl && a.spp == 1 && a.compact && a.queue[0] && a.queue_count && a.max_segments > phase0 &&
                     (a.max_segments <= 2 * phase0 || a.queue[1]);  // (the queue kernels sample no light and read no environment)
  b.seg_begin = 0;
  b.seg_end = split ? phase0 : a.max_segments;
  b.q_in = nullptr;
  b.q_in_count = nullptr;
  b.q_out = split ? a.queue[0] : nullptr;
  b.q_out_count = split ? a.queue_count : nullptr;
  if (split) (void)hipMemsetAsync(a.queue_count, 0, 2 * kPathQueues * sizeof(uint32_t), s);
  if (fin) {
    const FinalSplit sp = final_split(a, *fin, *pol, grid.x, tiles_y);
    const dim3 grid1(final_grid(sp));
    if (run_info) {
      run_info[0] = sp.n_runs ? sp.n_tiles / tiles_y : grid.x;
      run_info[1] = sp.n_runs;
      run_info[2] = sp.n_runs ? grid.x * tiles_y - sp.n_tiles : 0u;
    }
    hipLaunchKernelGGL(k_pathtrace_final<kFinalRoleCw>, grid1, block, dyn, s, b, tex, *fin, sp);
  } else
#if RTPT_AB_VARIANTS
  if (pool) {
    if (gb)
      hipLaunchKernelGGL((k_pathtrace_pool<true>), grid, block, dyn, s, b, *gb);
    else
      hipLaunchKernelGGL((k_pathtrace_pool<false>), grid, block, dyn, s, b, GbufferArgs{});
  } else
#endif
  if (envl) {
    // the ENV axis (kernels.hpp): its instantiations are kernels_env.hip's, one part per scene mode with and without a NormalView
    const int m = scene_mode(a.scene);
    const auto part = m == 0 ? launch_pathtrace_env_p0 : (m == 1 ? (nrm ? launch_pathtrace_env_p2 : launch_pathtrace_env_p1) : (nrm ? launch_pathtrace_env_p4 : launch_pathtrace_env_p3));
    part(b, gb, tex, spec, grid, block, dyn, s, lights, normals, envmap);
  } else
  // the instantiation list of the family: scene mode x DEMOD x TEX x SPEC (x COMPACT for the unfused launch) x NRM (kernels.hpp: in
  // the BVH modes and the compacting forms only), here and nowhere else
  with_mode<3>(scene_mode(a.scene), [&](auto mode) {
    constexpr int M = decltype(mode)::value;
    with_bool(a.albedo != nullptr, [&](auto demod) {  // RTPT_FLAG_EXT_DEMODULATE: the instantiations that store the albedo plane
      constexpr bool D = decltype(demod)::value;
      with_mode<3>(tex_mode(tex), [&](auto tmode) {  // rtpt_scene_set_textures: the instantiations that sample the atlas, with mips or without
        constexpr int T = decltype(tmode)::value;
        // rtpt_scene_set_materials_ext: the instantiations that bounce specular / dielectric materials; RTPT_FLAG_EXT_NEE,
        // RTPT_FLAG_EXT_NEE_SPHERE, RTPT_FLAG_EXT_NEE_POWER, RTPT_FLAG_EXT_NEE_MIS: those that sample lights (kernels.hpp: the SPEC axis)
        with_mode<kSpecModes>(spec, [&](auto smode) {
          constexpr int S = decltype(smode)::value;
          // l: the light argument S asks for, spec_lights_t<S>.  (The launch syntax, because a kernel template with a parameter pack
          // left to deduction is no argument for hipLaunchKernelGGL's deduced kernel type: a call deduces it from its arguments.)
          const auto go = [&](auto... l) {
            if constexpr (pack_nrm<decltype(l)...>()) {  // NRM: the fused launch and the unfused compacting one
              if (gb)
                k_gbuffer_pathtrace<M, D, T, S><<<grid, block, dyn, s>>>(b, *gb, tex, l...);
              else
                k_pathtrace<M, true, D, T, S><<<grid, block, dyn, s>>>(b, tex, l...);
            } else {
              if (gb) {
                if constexpr (M != 0)
                  k_gbuffer_pathtrace<M, D, T, S><<<grid, block, dyn, s>>>(b, *gb, tex, l...);
                else
                  k_gbuffer_pathtrace_small<D, T, S><<<grid, block, dyn, s>>>(b, *gb, tex, l...);
                return;
              }
              with_bool(a.compact != 0, [&](auto compact) {
                constexpr bool C = decltype(compact)::value;
                if constexpr (M != 0)
                  k_pathtrace<M, C, D, T, S><<<grid, block, dyn, s>>>(b, tex, l...);
                else
                  k_pathtrace_small<C, D, T, S><<<grid, block, dyn, s>>>(b, tex, l...);
              });
            }
          };
          // n: the scene's NormalView behind it, or nothing
          const auto with_lights = [&](auto... n) {
            if constexpr (spec_power(S))
              go(lights, n...);
            else if constexpr (spec_lights(S))
              go(LightView{lights.ids, lights.n}, n...);
            else
              go(n...);
          };
          if constexpr (M != 0) {
            if (nrm) {
              with_lights(normals);
              return;
            }
          }
          with_lights();
        });
      });
    });
  });
  if (!split) return;
  const int n_cu = a.n_cu > 0 ? a.n_cu : 256;  // of the context's device (rtpt_create)
  const dim3 qgrid(static_cast<uint32_t>(n_cu) * 8u);
  int cur = 0;
  for (uint32_t begin = phase0, len = phase0; begin < a.max_segments; begin += len, len *= 2, cur ^= 1) {
    const uint32_t end = begin + len < a.max_segments ? begin + len : a.max_segments;
    PathtraceArgs c = b;
    c.seg_begin = begin;
    c.seg_end = end;
    c.q_in = a.queue[cur];
    c.q_in_count = a.queue_count + cur * kPathQueues;
    const bool more = end < a.max_segments;
    c.q_out = more ? a.queue[cur ^ 1] : nullptr;
    c.q_out_count = more ? a.queue_count + (cur ^ 1) * kPathQueues : nullptr;
    if (more) (void)hipMemsetAsync(a.queue_count + (cur ^ 1) * kPathQueues, 0, kPathQueues * sizeof(uint32_t), s);
    with_mode<3>(scene_mode(a.scene), [&](auto mode) {
      with_mode<3>(tex_mode(tex), [&](auto tmode) {
        with_mode<3>(spec_mode(specular), [&](auto spec) {
          constexpr int QM = decltype(mode)::value, QT = decltype(tmode)::value, QS = decltype(spec)::value;
          if constexpr (QM != 0) {
            if (nrm) {
              k_pathtrace_queue<QM, QT, QS><<<qgrid, block, dyn_queue, s>>>(c, tex, normals);
              return;
            }
          }
          k_pathtrace_queue<QM, QT, QS><<<qgrid, block, dyn_queue, s>>>(c, tex);  // (the launch syntax: see `go` above)
        });
      });
    });
    if (end >= a.max_segments) break;
  }
}

}  // namespace rt
