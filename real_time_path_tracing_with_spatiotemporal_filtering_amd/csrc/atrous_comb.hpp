// atrous_comb.hpp — the body of the LDS-staged comb filter kernel, stated once: k_atrous_comb_sh (atrous.hip) runs it as a launch
// of its own, k_pathtrace_final (kernels.hip) as the workgroups of a tracing launch that carry the previous frame's final pass.
// Everything here is force-inlined; the caller owns the dynamic LDS and says which workgroup of how many it is.
#pragma once

#include "atrous_math.hpp"
#include "device_common.hpp"
#include "lds_dma.hpp"

namespace rt {
namespace {

// "Comb" kernel.
//
// A wave owns a 64-px-wide column segment and kCombM output rows spaced k apart: y_m = yc + m*k + r
// (a comb of residue r).  Their tap rows y_m - k, y_m, y_m + k are again rows of the comb, so each
// staged row serves up to three outputs.  Rows (64 + 2k px: colour+depth cell, id) are staged into
// LDS with LDS-DMA; the horizontal taps x-k / x / x+k are the same staged row read at three lane
// offsets: 2 vector-memory instructions per staged row instead of 27 per pixel.
//
// Normal weights pow(max(0, dot(n_p, n_q)), sigma_n) (:62) depend only on the id pair, so k_lut
// tabulates them once per frame ((T+1)^2 floats, same arithmetic) and the block copies the table to
// LDS: one ds_read_b32 per tap replaces the compare/branch/gather/pow sequence.
constexpr int kCombM = 2;       // output rows per wave
constexpr int kPairMax = 64;    // ids (T+1) for which the pair table is kept in LDS

// The kernel.  The kShWaves waves of a block filter kShWaves CONSECUTIVE chunks of one comb: 4M outputs
// per column whose tap rows are the 4M+2 rows yg + (j-1)k.  Each distinct row is staged by exactly
// one wave into a block-shared LDS region and a workgroup barrier publishes it.  (A first version
// staged M+2 rows per wave privately — no barrier at all — but then a block fetches 4(M+2) rows of
// which only 4M+2 are distinct, and the duplicates are in flight at the same time so L2 serves few
// of them: PMC showed 1.74x the algorithmic read bytes reaching the fabric, and at 5.6 TB/s the
// kernel was fabric-bound at 72-76 us.  Sharing brought it to 66-69 us.  Sweep at 4K, k = 5:
// (M, waves, 64-px segments per wave row) = (2,4,1) 67 us, (3,4,1) 74, (2,8,1) 68, (1,8,1) 71,
// (2,4,2) 66-77, (2,8,2) 72-88.)
constexpr int kShWaves = 4;   // waves (consecutive chunks) per block
constexpr int kShHalves = 1;  // 64-px segments per wave row: the 2k-column halo is paid once per 64*kShHalves px
constexpr int kShThreads = 64 * kShWaves;

// NRM = true is the variant for scenes whose id-pair table does not fit LDS (more than 63 triangles, i.e. every
// scene but the Cornell box): instead of the 4-byte id, each staged cell carries the pixel's normal — a second
// 16-byte plane written by k_gbuffer (normal_tab[id]: n.xyz and the self weight) — and the normal weight is computed
// per tap from the two staged normals with the same arithmetic as the direct kernel.  32 instead of 20 staged bytes
// per pixel, but 3 vector-memory instructions per staged row instead of the direct kernel's 27 per pixel.
// R / EXTA: the extension modes that only change the TAPS (RTPT_FLAG_EXT_GAUSS5: radius R = 2 with the gaussianKernel2D
// weights the reference declares and never uses, temporalFiltering.comp.glsl:93-99; RTPT_FLAG_EXT_POW2_STRIDE: stride
// 2^(k-1), passed as a.stride) run in this kernel too — the same comb staging with 2R halo rows per workgroup and 2R*s
// halo columns per segment, and the arithmetic of k_atrous_ext (h kept per tap, correctly-rounded final division), so
// the two are bit-identical.  25 taps are 25 LDS reads here instead of 75 global loads per pixel.
constexpr int kFinalWaves = 1;  // id-pair final pass: waves per SIMD to squeeze the registers for (A/B: 4 by itself)

// The reprojected pixel of a final pass as one 4-byte cell (AtrousArgs::reproj_out / reproj_in): the only reader is history_at,
// which returns 0 for every pixel outside [0, W) x [hist_y0, hist_y1), a subset of the frame — so everything outside the frame
// (INT_MIN / INT_MAX / NaN landings included) is one sentinel.  W, H <= 65535 (the host's condition): x = 65535 is never inside.
constexpr uint32_t kReprojOutside = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t reproj_pack(int ppx, int ppy, int W, int H) {
  return (ppx >= 0 && ppx < W && ppy >= 0 && ppy < H) ? (static_cast<uint32_t>(ppy) << 16 | static_cast<uint32_t>(ppx)) : kReprojOutside;
}
__device__ __forceinline__ void reproj_unpack(uint32_t cell, int& ppx, int& ppy) {
  ppx = static_cast<int>(cell & 0xFFFFu);
  ppy = static_cast<int>(cell >> 16);
}
// Where the RLOAD variants issue their two loads (bits 0-1: id-pair, bits 2-3: per-pixel normals).  0: both behind the taps,
// where the id-pair compute variant reprojects; 1: the packed cells right behind the publishing barrier and the history fetch
// ahead of the taps; 2: the packed cells with the staging DMA, ahead of the barrier, and every history fetch of the wave
// right behind it.
// Measured at 4K, k = 5, in-process lines of one job (profiles/r12_reproj_reuse_ab.txt); the compute sibling ran 103-107 us
// (id-pair) and 138 us (per-pixel normals) beside them:
//   id-pair, compiled like its sibling (waves_per_eu 1: 73 VGPRs, 6 waves)   placement 0: 100.2-100.6   1: 104.6-104.8   2: 93.8-94.4
//   id-pair, waves_per_eu 8 (62-64 VGPRs, no scratch; LDS admits 7 workgroups)                          1:  83.8-86.8   2: 83.2-86.8
//   per-pixel normals (69-73 VGPRs; 6 waves either way: LDS admits 6 workgroups) 0: 107.5-107.6         1: 109.7-110.4  2: 108.0-108.2
// The id-pair pass was never short of bytes: the ones it no longer reads bought 3 us until the registers the reprojection no longer needs
// were turned into two more resident waves, which bought 20.  With those, where the 4-byte cell is fetched no longer
// matters, so it stays behind the barrier (placement 1: no load of its own in front of the wait the other workgroups see).
// The per-pixel-normal taps (x^128 per tap) hide the two dependent loads behind them by themselves: placement 0.
#ifndef RTPT_REPROJ_LOAD_PLACE
#define RTPT_REPROJ_LOAD_PLACE 1
#endif
#ifndef RTPT_REPROJ_LOAD_WAVES
#define RTPT_REPROJ_LOAD_WAVES 8  // id-pair RLOAD instances: the waves-per-SIMD pin
#endif

// The plain id-pair final pass as workgroups of a tracing launch (kernels.hip: k_pathtrace_final).  That launch keeps 8
// workgroups per CU, so one workgroup's LDS, static included, stays under 160 KiB / 8 = 20 KiB: a staged row of 74 cells — what
// k = 5, the final pass of the reference's five iterations, needs; the stand-alone instance rounds it to 80 — makes the
// 63-triangle pair table and the ten staged rows 4 368 + 14 800 bytes.  Larger strides run as the launch of their own.
constexpr int kFinalRoleCw = 74;
constexpr int kFinalRoleMaxK = (kFinalRoleCw - kBlockX * kShHalves) / 2;
inline size_t final_role_lds(const AtrousArgs& a) {
  const size_t np = static_cast<size_t>(a.n_tris) + 1;
  return ((np * np * 4 + 15) & ~static_cast<size_t>(15)) + static_cast<size_t>(kShWaves * kCombM + 2) * kFinalRoleCw * 20;
}

// One workgroup's share of a comb launch.  lds_raw: the launch's dynamic LDS (pair table + one staged region).
// ROLE = false: the launch is the comb kernel's own — the workgroup is blockIdx.x of gridDim.x, which share the whole work list
// (the arguments behind lds_raw are not read).  ROLE = true: the launch holds other workgroups too and hands each group of its
// filter workgroups one range of the list — the workgroup is b of the nb (a multiple of 8) that share the items [lb_lo, lb_hi).
// Workgroups b, b + 8, .. take a contiguous eighth of the range (one XCD's, when the launch deals its workgroups round-robin)
// and deal it among themselves item by item.
template <int CWp, bool FINAL, bool EXACT, bool NRM, int R, bool EXTA, bool VAR, bool RLOAD, bool ROLE = false>
__device__ __forceinline__ void comb_items(const AtrousArgs& a, unsigned char* lds_raw, uint32_t b = 0, uint32_t nb = 0, uint32_t lb_lo = 0,
                                           uint32_t lb_hi = 0) {
  static_assert(!RLOAD || (FINAL && R == 1 && !EXTA && !VAR), "the cached reprojection serves the plain final pass only");
  constexpr int kLoadPlace = RLOAD ? ((RTPT_REPROJ_LOAD_PLACE >> (NRM ? 2 : 0)) & 3) : 0;
  constexpr bool kLoadEarly = kLoadPlace != 0;
  const int W = a.g.W, H = a.g.H, k = a.stride;  // a.stride == a.k (main.cpp:1259-1260, :135) unless POW2_STRIDE
  constexpr int rows = kShWaves * kCombM + 2 * R, cells = rows * CWp;  // block-shared rows
  const int NP = NRM ? 0 : static_cast<int>(a.n_tris) + 1;
  const int lane = static_cast<int>(threadIdx.x);
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.y));
  float* pairw = reinterpret_cast<float*>(lds_raw);  // [NP][NP]
  const int pair_bytes = (NP * NP * 4 + 15) & ~15;
  unsigned char* mine = lds_raw + pair_bytes;  // one region per block
  const float4* col = reinterpret_cast<const float4*>(mine);                // (r, g, b, depth)
  const uint32_t* ids = reinterpret_cast<const uint32_t*>(mine + 16 * cells);
  const float4* nrm = reinterpret_cast<const float4*>(mine + 16 * cells);   // NRM: (n.xyz, self weight) instead of ids
  const uint32_t lds0 = static_cast<uint32_t>(reinterpret_cast<size_t>((__attribute__((address_space(3))) unsigned char*)mine));
  const uint32_t lds_col = lds0, lds_ids = lds0 + 16u * static_cast<uint32_t>(cells);
  // EXTA with RTPT_FLAG_EXT_VARIANCE: the variance plane this iteration reads is staged as a third plane (4 B per cell)
  constexpr bool use_var = EXTA && !NRM && VAR;  // the launch picks VAR iff (a.ext & kExtVariance) && a.var_in
  const float* varp = reinterpret_cast<const float*>(mine + 20 * cells);
  const uint32_t lds_var = lds0 + 20u * static_cast<uint32_t>(cells);

  // id-pair weight table -> LDS (plain loads; no DMA is in flight yet)
  for (int i = wave * 64 + lane; i < NP * NP; i += kShThreads) pairw[i] = a.pair_tab[i];
  __syncthreads();

  // Work list.  A logical block = four CONSECUTIVE chunks (one per wave) of one residue and one
  // column.  Each XCD (physical blocks b, b+8, ...) owns a contiguous eighth of the list; see
  // the work list below for the order inside it.  The grid is persistent: the pair table is loaded once
  // per block, not per work item.  Speed only, never correctness: any mapping filters every pixel exactly
  // once.  (Tried on top of order 1 and dropped: an L2 prefetch of the block's next item, one dword per
  // 128-byte line — 68 -> 82 us; the memory system is saturated by requests, not starved of them.)
  const uint32_t per_res = static_cast<uint32_t>(a.tiles_x) * static_cast<uint32_t>(a.tiles_y);  // tiles_y = chunk groups
  const uint32_t nlb = ROLE ? lb_hi - lb_lo : per_res * static_cast<uint32_t>(k);
  const uint32_t xcd = (ROLE ? b : blockIdx.x) & 7u, jx = (ROLE ? b : blockIdx.x) >> 3, per_xcd = (ROLE ? nb : gridDim.x) >> 3;
  const uint32_t x_lo = (ROLE ? lb_lo : 0u) + static_cast<uint32_t>((static_cast<uint64_t>(nlb) * xcd) >> 3);
  const uint32_t x_hi = (ROLE ? lb_lo : 0u) + static_cast<uint32_t>((static_cast<uint64_t>(nlb) * (xcd + 1)) >> 3);
  const int row_lo = a.g.row_base, row_hi = a.g.row_base + a.rows_stored - 1;
  const bool tail_lane = lane < 2 * R * k;  // columns 64 .. 64+2Rk-1
  const EdgeStop es{a.sigma_z, a.sigma_l, a.cz, a.cl};

  // row-major list (residue, chunk group, column), dealt to the XCD's blocks item by item: the blocks
  // resident on an XCD work on a few consecutive row bands at any time, so the column halos of x-neighbours
  // and the rows shared by consecutive bands meet in that XCD's L2 (PMC: 245 -> 200 MB fetched per 4K
  // launch against round 2's order, each block walking down a column; 4K 66-72 -> 64-68 us, 1080p 20.5 -> 18.5 us)
#pragma unroll 1
  for (uint32_t lb = x_lo + jx; lb < x_hi; lb += per_xcd) {
  const uint32_t r_u = lb / per_res, rem_u = lb - r_u * per_res;
  const uint32_t cg_u = rem_u / static_cast<uint32_t>(a.tiles_x);
  const int r_now = __builtin_amdgcn_readfirstlane(static_cast<int>(r_u));
  const int cg_now = __builtin_amdgcn_readfirstlane(static_cast<int>(cg_u));
  const int bx_now = __builtin_amdgcn_readfirstlane(static_cast<int>(rem_u - cg_u * static_cast<uint32_t>(a.tiles_x)));
  const int yg = a.g.y0 + cg_now * (kShWaves * kCombM * k) + r_now;  // first output row of the group
  if (yg >= a.g.y1) continue;                                      // block-uniform
  const int x0 = bx_now * (kBlockX * kShHalves);
  uint32_t o16[kShHalves + 1], o4[kShHalves + 1];  // per-lane source offsets of the full chunks and the tail chunk
#pragma unroll
  for (int hf = 0; hf <= kShHalves; hf++) {
    int gx = x0 - R * k + hf * 64 + lane;
    gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);  // :136
    o16[hf] = static_cast<uint32_t>(gx) * 16u;
    o4[hf] = static_cast<uint32_t>(gx) * 4u;
  }
  // every wave is done reading the previous group's rows before anybody overwrites them
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  // waves run at priority 3 while they issue an item's DMAs, ahead of the other waves' arithmetic: 4K 67.0 -> 65.5 us
  // (in-process A/B)
  __builtin_amdgcn_s_setprio(3);
  // wave w stages rows w*M+1 .. w*M+M; wave 0 also row 0, the last wave also row 4M+1
  const int j_lo = wave * kCombM + (wave == 0 ? 0 : R);
  const int j_hi = wave * kCombM + kCombM + R - 1 + (wave == kShWaves - 1 ? R : 0);
  for (int j = j_lo; j <= j_hi; j++) {
    int gy = yg + (j - R) * k;
    gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);              // :136
    gy = gy < row_lo ? row_lo : (gy > row_hi ? row_hi : gy);  // rows only masked outputs could reach
    const size_t grow = static_cast<size_t>(gy - a.g.row_base) * W;  // wave-uniform
    const float4* rin = a.in + grow;
    const uint32_t* rvis = a.vis + grow;
    const float4* rnrm = NRM ? a.normals + grow : nullptr;
    const float* rvar = use_var ? a.var_in + grow : nullptr;
    const uint32_t cj = static_cast<uint32_t>(j * CWp);
#pragma unroll
    for (int hf = 0; hf < kShHalves; hf++) {
      dma_b128(rin, o16[hf], lds_col + (cj + 64u * hf) * 16u);
      if (NRM)
        dma_b128(rnrm, o16[hf], lds_ids + (cj + 64u * hf) * 16u);
      else
        dma_b32(rvis, o4[hf], lds_ids + (cj + 64u * hf) * 4u);
      if (use_var) dma_b32(rvar, o4[hf], lds_var + (cj + 64u * hf) * 4u);
    }
    if (tail_lane) {
      dma_b128(rin, o16[kShHalves], lds_col + (cj + 64u * kShHalves) * 16u);
      if (NRM)
        dma_b128(rnrm, o16[kShHalves], lds_ids + (cj + 64u * kShHalves) * 16u);
      else
        dma_b32(rvis, o4[kShHalves], lds_ids + (cj + 64u * kShHalves) * 4u);
      if (use_var) dma_b32(rvar, o4[kShHalves], lds_var + (cj + 64u * kShHalves) * 4u);
    }
  }
  __builtin_amdgcn_s_setprio(0);
  // final pass: world positions fetched with the staging DMA and the history ahead of the taps.  Measured at 4K: it pays
  // in the per-pixel-normal variant (1.15M triangles: 155.8 -> 144.1 us; its taps compute x^128 per tap and leave time to
  // hide the fetch) and costs in the id-pair variant (110.5 -> 125.6 us: the 2 KiB of world positions per wave lengthen the
  // wait in front of the workgroup barrier, which the other workgroups' taps no longer cover) — so NRM decides.
  // FINAL: the world positions of this wave's output pixels depend on nothing staged — fetch them now, in flight together
  // with the DMA and waited for by the same vmcnt(0)
  f3 wp_pre[kCombM * kShHalves];
  if (FINAL && NRM && !RLOAD) {
#pragma unroll
    for (int mh = 0; mh < kCombM * kShHalves; mh++) {
      const int m = mh / kShHalves, hf = mh % kShHalves;
      const int x = x0 + hf * 64 + lane;
      const int y = yg + (wave * kCombM + m) * k;
      wp_pre[mh] = f3{0.f, 0.f, 0.f};
      if (x < W && y < a.g.y1) wp_pre[mh] = xyz(a.worldpos[static_cast<size_t>(y - a.g.row_base) * W + x]);
    }
  }
  // RLOAD: the wave's packed cells, 4 bytes per output pixel — in flight with the DMA (placement 2) or issued as soon as
  // nothing waits on this wave (placement 1)
  uint32_t cell_pre[kCombM * kShHalves];
  f3 hc_pre[kCombM * kShHalves];
  auto load_cells = [&]() {
#pragma unroll
    for (int mh = 0; mh < kCombM * kShHalves; mh++) {
      const int m = mh / kShHalves, hf = mh % kShHalves;
      const int x = x0 + hf * 64 + lane;
      const int y = yg + (wave * kCombM + m) * k;
      cell_pre[mh] = kReprojOutside;
      if (x < W && y < a.g.y1) cell_pre[mh] = a.reproj_in[static_cast<size_t>(y - a.g.row_base) * W + x];
    }
  };
  if (kLoadPlace == 2) load_cells();
  // own DMA landed, then the barrier publishes every wave's rows to the block
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  if (kLoadPlace == 1) load_cells();
  if (kLoadPlace == 2) {
#pragma unroll
    for (int mh = 0; mh < kCombM * kShHalves; mh++) {
      int qx, qy;
      reproj_unpack(cell_pre[mh], qx, qy);
      hc_pre[mh] = f3{0.f, 0.f, 0.f};
      if (a.frame > 0) hc_pre[mh] = history_at(qx, qy, W, a.hist_y0, a.hist_y1, a.history, a.hist_row_base);
    }
  }

#pragma unroll
  for (int mh = 0; mh < kCombM * kShHalves; mh++) {
    const int m = mh / kShHalves, hf = mh % kShHalves;
    const int x = x0 + hf * 64 + lane;
    const int y = yg + (wave * kCombM + m) * k;
    if (x >= W || y >= a.g.y1) continue;
    const int cc = (wave * kCombM + m + R) * CWp + hf * 64 + lane + R * k;
    const float4 cp4 = col[cc];
    const f3 cp = xyz(cp4);
    const float dp = cp4.w;
    const size_t ip = static_cast<size_t>(y - a.g.row_base) * W + x;
    const float4 np4 = NRM ? nrm[cc] : make_float4(0.f, 0.f, 0.f, 0.f);
    const f3 np = xyz(np4);
    const uint32_t idp = NRM ? (FINAL && !RLOAD ? a.vis[ip] : 0u) : ids[cc];  // NRM: the id is only needed for the reprojection
    const float* prow = pairw + idp * NP;
    const float wself = NRM ? np4.w : prow[idp];
    // FINAL: reproject first (:213-239) so that the history fetch is in flight under the taps' arithmetic
    int ppx = x, ppy = y;
    f3 hc{0.f, 0.f, 0.f};
    if (FINAL && NRM && !RLOAD) {
      reproject_pixel(W, H, a.PVprev, idp, wp_pre[mh], a.lut_prev, x, y, ppx, ppy);
      if (a.frame > 0) hc = history_at(ppx, ppy, W, a.hist_y0, a.hist_y1, a.history, a.hist_row_base);  // :251,:253
    }
    if (kLoadPlace == 1) {
      reproj_unpack(cell_pre[mh], ppx, ppy);
      if (a.frame > 0) hc = history_at(ppx, ppy, W, a.hist_y0, a.hist_y1, a.history, a.hist_row_base);
    }
    if (kLoadPlace == 2) hc = hc_pre[mh];
    f3 num{0.f, 0.f, 0.f};
    float den = 0.f, vsum = 0.f;
    const VarGuide vg = var_guide(a.sigma_l, cp, use_var, use_var ? (a.var_scale ? a.var_scale[ip] : varp[cc]) : 0.0f);
#pragma unroll
    for (int i = -R; i <= R; i++) {  // :132 (x offset outer: the reference's accumulation order)
#pragma unroll
      for (int jj = -R; jj <= R; jj++) {  // :133
        float w;
        f3 cq;
        if (!EXTA && i == 0 && jj == 0) {
          cq = cp;
          w = centre_weight(wself, cp, dp);  // centre tap: q == p, both exponentials are exactly 1
        } else {
          const int qi = cc + jj * CWp + i * k;
          const float4 cq4 = col[qi];
          cq = xyz(cq4);
          float wn;
          if (NRM) {
            // :62 (pow_sigma: with exact::powi's loop this variant was SALU-bound at 166 us)
            wn = pow_sigma(glsl_max(0.0f, exact::dot(np, xyz(nrm[qi]))), a.sigma_n);
          } else
            wn = prow[ids[qi]];  // :62 via the id-pair table
          w = edge_weight<EXACT>(es, wn, cp, cq, dp, cq4.w, use_var, vg);
        }
        if (EXTA) {
          // the extension family keeps the tap's own h (gaussianKernel2D / 273, :93-99, or 1/9, :145)
          const float hw = (R == 2 ? gauss5(i, jj) * (1.0f / 273.0f) : 1.0f / 9.0f) * w;
          tap_add_h(num, den, hw, cq);
          if (use_var) vsum = fmaf_(hw * hw, varp[cc + jj * CWp + i * k], vsum);
        } else
          tap_add<EXACT>(num, den, w, cq);
      }
    }
    const f3 filtered = normalise<EXACT || EXTA>(num, den);
    if (EXTA && use_var && a.var_out) a.var_out[ip] = vsum / (den * den);
    if (!FINAL) {
      // non-temporal stores for the k < N passes (the pass does not re-read its output): 65 -> 62.5 us in a frame; a pass
      // repeated on the SAME buffers drops to 54 us (77 %) because its input then stays in the 256 MB memory-side cache —
      // in a frame the input was just written by the previous pass.  Tried without gain: nt on the final pass's store, nt
      // on the staging loads (66-69 us), alternating the walk direction per pass so a pass starts on the rows written last
      typedef float v4f_ __attribute__((ext_vector_type(4)));
      v4f_ o4 = {filtered.x, filtered.y, filtered.z, a.alpha_zero ? 0.0f : dp};  // :152 (+ depth in alpha)
      __builtin_nontemporal_store(o4, reinterpret_cast<v4f_*>(a.out + ip));
      continue;
    }
    if (!NRM && !RLOAD) {
      reproject_pixel(W, H, a.PVprev, idp, xyz(a.worldpos[ip]), a.lut_prev, x, y, ppx, ppy);  // :213-239
      if (a.frame > 0) hc = history_at(ppx, ppy, W, a.hist_y0, a.hist_y1, a.history, a.hist_row_base);
    }
    if (RLOAD && !kLoadEarly) {
      reproj_unpack(a.reproj_in[ip], ppx, ppy);
      if (a.frame > 0) hc = history_at(ppx, ppy, W, a.hist_y0, a.hist_y1, a.history, a.hist_row_base);
    }
    if (!RLOAD) {  // (the host never asks a loading pass for either: the raw integers are not in the cell)
      if (a.prev_pixel) a.prev_pixel[ip] = make_int2(ppx, ppy);
      if (!EXTA && a.reproj_out) a.reproj_out[ip] = reproj_pack(ppx, ppy, W, H);
    }
    f3 blend = filtered;             // :258
    bool use_history = a.frame > 0;  // :251
    float alpha = a.alpha;
    if (EXTA) {  // the final pass of the extension modes
      if (use_history && (a.ext & kExtDisocclusion))
        use_history = same_primitive_at(a.prev_vis, W, H, a.pvis_row_base, a.pvis_y0, a.pvis_y1, ppx, ppy, idp);
      if (a.ext & kExtAdaptiveAlpha) alpha = adaptive_alpha(alpha, a.gradient[ip].x);
    }
    if (use_history) blend = temporal_blend(filtered, hc, alpha);
    a.out[ip] = make_float4(blend.x, blend.y, blend.z, 0.0f);  // :263 (D1: distinct buffer)
    // main.cpp:1338-1361, fused: the blit reads exactly the value stored above (alpha 0), k_present's conversion
    // (not in the per-pixel-normal variant: its final pass sits at 79 VGPRs = 6 waves per SIMD, and the store's operands
    // cost it a wave — 142 -> 176 us at 4K; k_present serves those scenes)
    if (!NRM && a.present && y >= a.present_y0 && y < a.present_y1)  // index = ip minus a wave-uniform row offset: no new per-lane address
      (a.present - static_cast<ptrdiff_t>(a.present_y0 - a.g.row_base) * W)[ip] = pack_bgra8(blend, 0.0f);
  }
  }  // work list
}

}  // namespace
}  // namespace rt
