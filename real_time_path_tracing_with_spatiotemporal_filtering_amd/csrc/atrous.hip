// atrous.hip — K3: one iteration of the edge-stopping a-trous filter
// (temporalFiltering.comp.glsl:191-265): 3x3 taps at stride k, h = 1/9, weights on normal / depth /
// colour; the FINAL variants fuse reprojection + temporal blend (:213-263).
//
//   k_atrous_comb   the shipping kernel: wave-private LDS staging by LDS-DMA, comb row assignment
//   k_atrous        direct global-load kernel: scenes whose id-pair weight table does not fit LDS
//                   (> 63 triangles; a comb variant gathering per-id normals from an 18 MB table was
//                   measured SLOWER on the 1.15M-triangle scene: 197 vs 149 us), strides k > 16, and
//                   RTPT_FLAG_DIRECT_FILTER
//
// Measured on MI355X at 3840x2160 (profiles/): the direct kernel is bound by the vector-memory pipe
// (27 load instructions per pixel: 107 us even with every tap an L1 hit); tile kernels with a
// workgroup barrier run the chip in load/compute lockstep.  The comb kernel has neither problem.
//
// Colour planes are "rgbd" while a frame is being filtered: the alpha channel, which the reference
// always writes as 0 (raytrace.comp.glsl:343, temporalFiltering.comp.glsl:152), carries the pixel's
// G-buffer depth from rtpt_raytrace through every non-final pass, so a tap is ONE 16-byte cell
// (colour + depth) plus the 4-byte id instead of three separate planes — 36 instead of 40 bytes of
// HBM traffic per pixel and a third fewer load instructions.  The final pass writes alpha 0 again;
// the C-ABI layer hides the convention (rtpt_readback masks alpha, rtpt_set_plane re-stamps depth).
#include <cstdlib>

#include "atrous_comb.hpp"
#include "atrous_math.hpp"
#include "device_common.hpp"
#include "lds_dma.hpp"
#include "select.hpp"

#ifndef RTPT_TILE_TIMELINE
#define RTPT_TILE_TIMELINE 0  // timeline build (scripts/tile_timeline.py): when the workgroups of the single-pass launches lived
#endif

namespace rt {
namespace {

#if RTPT_TILE_TIMELINE
#define RTPT_SPAN_SLOTS 2  // k_atrous_comb_sh: an iteration k < N, the final pass
#define RTPT_SPAN_READER rtpt_debug_comb_span
#define RTPT_SPAN_DEVICE
#include "experiments/span_instrumentation.inc"
#undef RTPT_SPAN_DEVICE
#endif

// XCD-aware tile mapping.  Workgroups are dealt round-robin over the 8 XCDs (block b and b+8 share an
// XCD and its private 4 MiB L2).  The stencil re-reads every input row at y-k, y and y+k, so the three
// uses must meet in ONE L2 while the rows in between are streamed through it.  Tiles are therefore
// enumerated strip-major — vertical strips kStripTiles tiles (512 px) wide, row-major inside a strip,
// so the reuse window of 2k+few rows is a few hundred KB — and each XCD gets one contiguous chunk of
// that enumeration (bijective for any block count).  Placement is a speed assumption only; any
// dispatch order computes the same pixels.
constexpr int kStripTiles = 1 << 20;  // one strip = the whole width: row-major bands (strips measured slower)
__device__ __forceinline__ void xcd_strip_tile(int tiles_x, int tiles_y, int& bx, int& by) {
  const uint32_t tx = static_cast<uint32_t>(tiles_x), ty = static_cast<uint32_t>(tiles_y);
  const uint32_t nb = tx * ty;
  const uint32_t b = blockIdx.x;
  const uint32_t q = nb >> 3, r = nb & 7u, xcd = b & 7u, j = b >> 3;
  const uint32_t lb = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
  const uint32_t full = tx / kStripTiles;           // full-width strips
  const uint32_t per_strip = kStripTiles * ty;
  uint32_t strip, rem, sw;
  if (lb < full * per_strip) {
    strip = lb / per_strip;
    rem = lb - strip * per_strip;
    sw = kStripTiles;
  } else {
    strip = full;
    rem = lb - full * per_strip;
    sw = tx - full * kStripTiles;
  }
  const uint32_t row = rem / sw;
  by = static_cast<int>(row);
  bx = static_cast<int>(strip * kStripTiles + (rem - row * sw));
}

// PX (launch_atrous's px_normals; RTPT_FLAG_EXT_SMOOTH_GUIDE): a pixel's normal is its cell of a.normals, which covers every row
// read, instead of normal_tab[id]; every tap's weight is computed from the two cells (two pixels of one triangle no longer share
// a normal), the centre takes its cell's self weight — the comb kernel's NRM form tap for tap, so the two agree bit for bit on any
// plane.  The id is read only for the final pass's reprojection.
template <bool FINAL, bool EXACT, bool PX = false>
__global__ __launch_bounds__(kThreads) void k_atrous(AtrousArgs a) {
  int bx, by;
  xcd_strip_tile(a.tiles_x, a.tiles_y, bx, by);
  // blockDim.x == 64: a wave is one row segment, so the row index is wave-uniform (SGPR) and every
  // tap row resolves to a scalar base address + a 32-bit per-lane column offset
  const int ty = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.y));
  const int x = bx * kBlockX + static_cast<int>(threadIdx.x);
  const int y = a.g.y0 + by * kBlockY + ty;
  if (x >= a.g.W || y >= a.g.y1) return;
  const int W = a.g.W, H = a.g.H, k = a.k;
  const size_t rowp = static_cast<size_t>(y - a.g.row_base) * W;
  const float4 cp4 = a.in[rowp + x];
  const f3 cp = xyz(cp4);
  const float dp = cp4.w;  // rgbd
  const uint32_t idp = (!PX || FINAL) ? a.vis[rowp + x] : 0u;
  const float4 np4 = PX ? a.normals[rowp + x] : a.normal_tab[idp];
  const f3 np = xyz(np4);
  const EdgeStop es{a.sigma_z, a.sigma_l, a.cz, a.cl};
  f3 num{0.f, 0.f, 0.f};
  float den = 0.f;
  int qxs[3], qys[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int qx = x + (i - 1) * k, qy = y + (i - 1) * k;  // :135
    qxs[i] = qx < 0 ? 0 : (qx > W - 1 ? W - 1 : qx);  // :136
    qys[i] = qy < 0 ? 0 : (qy > H - 1 ? H - 1 : qy);
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {  // :132 (x offset outer, as in the reference's accumulation order)
#pragma unroll
    for (int j = 0; j < 3; j++) {  // :133
      float w;
      f3 cq;
      if (i == 1 && j == 1) {
        // centre tap: q == p, so both exponentials are exactly 1 and w = pow(max(0,dot(np,np)),sigma_n)
        cq = cp;
        w = centre_weight(np4.w, cp, dp);
      } else {
        const size_t rowq = static_cast<size_t>(qys[j] - a.g.row_base) * W;
        const int qx = qxs[i];
        const float4 cq4 = a.in[rowq + qx];
        cq = xyz(cq4);
        float wn;
        if constexpr (PX) {
          wn = pow_sigma(glsl_max(0.0f, exact::dot(np, xyz(a.normals[rowq + qx]))), a.sigma_n);  // :62
        } else {
          const uint32_t idq = a.vis[rowq + qx];
          if (idq == idp) {
            wn = np4.w;  // same primitive: the per-id self weight (same bits as recomputing it)
          } else {
            const f3 nq = xyz(a.normal_tab[idq]);
            wn = pow_sigma(glsl_max(0.0f, exact::dot(np, nq)), a.sigma_n);  // :62
          }
        }
        w = edge_weight<EXACT>(es, wn, cp, cq, dp, cq4.w);  // rgbd
      }
      tap_add<EXACT>(num, den, w, cq);
    }
  }
  const f3 filtered = normalise<EXACT>(num, den);
  if (!FINAL) {
    a.out[rowp + x] = make_float4(filtered.x, filtered.y, filtered.z, a.alpha_zero ? 0.0f : dp);  // :152 (+ depth in alpha)
    return;
  }
  int ppx, ppy;
  reproject_pixel(W, H, a.PVprev, idp, xyz(a.worldpos[rowp + x]), a.lut_prev, x, y, ppx, ppy);  // :213-239
  if (a.prev_pixel) a.prev_pixel[rowp + x] = make_int2(ppx, ppy);
  f3 blend = filtered;                                                          // :258
  if (a.frame > 0) blend = temporal_blend(filtered, history_at(ppx, ppy, W, a.hist_y0, a.hist_y1, a.history, a.hist_row_base), a.alpha);  // :251-254
  a.out[rowp + x] = make_float4(blend.x, blend.y, blend.z, 0.0f);  // :263 (D1: distinct buffer)
}


// Extension modes (RTPT_FLAG_EXT_*): the pieces of the textbook A-SVGF the reference declares but does not
// use — the 5x5 gaussianKernel2D table (temporalFiltering.comp.glsl:93-99), 2^(k-1) tap stride, the
// gradient-adaptive alpha (:247-248, commented out) and a disocclusion test on previousVisibilityBuffer
// (main.cpp:1367: copied every frame, never read).  Opt-in and outside the reference's behaviour, so this is
// one generic direct-load kernel (k_atrous_ext, atrous_math.hpp's arithmetic like every other) rather than a tuned one.

// RTPT_FLAG_EXT_VARIANCE (extension, see include/rtpt.h): first and second luminance moments accumulated along the
// reprojected pixel, history length, and the variance the filter iterations are guided by.
__global__ __launch_bounds__(kThreads) void k_moments(MomentsArgs a) {
  const int x = blockIdx.x * kBlockX + threadIdx.x;
  const int y = a.g.y0 + blockIdx.y * kBlockY + threadIdx.y;
  if (x >= a.g.W || y >= a.g.y1) return;
  const int W = a.g.W, H = a.g.H;
  const size_t ip = static_cast<size_t>(y - a.g.row_base) * W + x;
  const uint32_t id = a.vis[ip];
  const float lum = luminance(xyz(a.traced[ip]));
  int ppx, ppy;
  reproject_pixel(W, H, a.PVprev, id, xyz(a.worldpos[ip]), a.lut_prev, x, y, ppx, ppy);
  // the previous frame's id and moment planes hold frame rows [hist_y0, hist_y1) from hist_row_base on: the context's
  // own rows, or the bands gathered from the other strips (rtpt_set_external_guides); inside the frame but outside
  // those rows cannot happen when the host registered the rows the strip's pixels can reach
  bool valid = a.frame > 0 && ppx >= 0 && ppx < W && ppy >= 0 && ppy < H && ppy >= a.hist_y0 && ppy < a.hist_y1;
  const size_t iq = valid ? static_cast<size_t>(ppy - a.hist_row_base) * W + ppx : 0;
  if (valid) valid = a.prev_vis[iq] == id;
  float m1 = lum, m2 = lum * lum, n = 1.0f;
  if (valid) {
    const float4 mp = a.moments_prev[iq];
    const float al = glsl_max(a.alpha, 1.0f / (mp.z + 1.0f)), oma = 1.0f - al;
    m1 = fmaf_(lum, al, mp.x * oma);
    m2 = fmaf_(lum * lum, al, mp.y * oma);
    n = glsl_min(mp.z + 1.0f, 255.0f);
  }
  float var = glsl_max(0.0f, fmaf_(-m1, m1, m2));
  if (n < 4.0f) {
    if (a.svgf) {
      // SVGF: a history this short says nothing about the variance yet — estimate it from the current frame's luminance
      // over the 7x7 neighbourhood, taps on the same primitive only (the centre always counts), clamped at the frame border.
      // On a strip the window of the outermost rows would leave the stored rows: those reads are clamped to what is stored
      // (memory safety only — a strip stores 3 traced rows beyond the rows whose variance anything consumes, strips.py)
      const int r_lo = a.g.row_base, r_hi = a.g.row_base + a.rows_stored - 1;
      float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
      for (int dy = -3; dy <= 3; dy++)
        for (int dx = -3; dx <= 3; dx++) {
          int qx = x + dx, qy = y + dy;
          qx = qx < 0 ? 0 : (qx > W - 1 ? W - 1 : qx);
          qy = qy < 0 ? 0 : (qy > H - 1 ? H - 1 : qy);
          qy = qy < r_lo ? r_lo : (qy > r_hi ? r_hi : qy);
          const size_t iqn = static_cast<size_t>(qy - a.g.row_base) * W + qx;
          if (a.vis[iqn] != id) continue;
          const float l = luminance(xyz(a.traced[iqn]));
          s1 = s1 + l;
          s2 = fmaf_(l, l, s2);
          cnt = cnt + 1.0f;
        }
      const float m1s = s1 / cnt, m2s = s2 / cnt;
      var = glsl_max(0.0f, fmaf_(-m1s, m1s, m2s));
    }
    var = var * (4.0f / n);
  }
  a.moments_out[ip] = make_float4(m1, m2, n, var);
  a.var_out[ip] = var;
}

// RTPT_FLAG_EXT_SVGF_VARIANCE: the variance that scales an iteration's luminance weight is the 3x3 Gaussian of the variance
// plane around the pixel (SVGF's variance prefilter), unit spacing whatever the iteration's stride: a pass of its own (8 B/px)
// because the staged filter kernels hold rows k apart
__global__ __launch_bounds__(kThreads) void k_var_prefilter(FrameGeom g, int rows_stored, const float* __restrict__ var, float* __restrict__ out) {
  const int x = blockIdx.x * kBlockX + threadIdx.x;
  const int y = g.y0 + blockIdx.y * kBlockY + threadIdx.y;
  if (x >= g.W || y >= g.y1) return;
  float acc = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      int qx = x + dx, qy = y + dy;
      qx = qx < 0 ? 0 : (qx > g.W - 1 ? g.W - 1 : qx);
      qy = qy < 0 ? 0 : (qy > g.H - 1 ? g.H - 1 : qy);
      qy = qy < g.row_base ? g.row_base : (qy > g.row_base + rows_stored - 1 ? g.row_base + rows_stored - 1 : qy);  // memory safety on strips
      const float gw = (dx == 0 ? 2.0f : 1.0f) * (dy == 0 ? 2.0f : 1.0f);
      acc = fmaf_(gw, var[static_cast<size_t>(qy - g.row_base) * g.W + qx], acc);
    }
  out[static_cast<size_t>(y - g.row_base) * g.W + x] = acc * 0.0625f;
}

// PX: as in k_atrous — every tap, the centre included, weighs the two pixels' cells of a.normals
template <bool FINAL, bool EXACT, bool PX = false>
__global__ __launch_bounds__(kThreads) void k_atrous_ext(AtrousArgs a) {
  int bx, by;
  xcd_strip_tile(a.tiles_x, a.tiles_y, bx, by);
  const int ty = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.y));
  const int x = bx * kBlockX + static_cast<int>(threadIdx.x);
  const int y = a.g.y0 + by * kBlockY + ty;
  if (x >= a.g.W || y >= a.g.y1) return;
  const int W = a.g.W, H = a.g.H, k = a.stride;
  const bool gauss = (a.ext & kExtGauss5) != 0;
  const int R = gauss ? 2 : 1;
  const size_t rowp = static_cast<size_t>(y - a.g.row_base) * W;
  const float4 cp4 = a.in[rowp + x];
  const f3 cp = xyz(cp4);
  const float dp = cp4.w;  // rgbd
  const uint32_t idp = (!PX || FINAL) ? a.vis[rowp + x] : 0u;
  const float4 np4 = PX ? a.normals[rowp + x] : a.normal_tab[idp];
  const f3 np = xyz(np4);
  f3 num{0.f, 0.f, 0.f};
  float den = 0.f, vsum = 0.f;
  const bool use_var = (a.ext & kExtVariance) && a.var_in;
  const EdgeStop es{a.sigma_z, a.sigma_l, a.cz, a.cl};
  const VarGuide vg = var_guide(a.sigma_l, cp, use_var, use_var ? (a.var_scale ? a.var_scale : a.var_in)[rowp + x] : 0.0f);
  for (int i = -R; i <= R; i++) {    // :132
    for (int j = -R; j <= R; j++) {  // :133
      int qx = x + i * k, qy = y + j * k;  // :135
      qx = qx < 0 ? 0 : (qx > W - 1 ? W - 1 : qx);  // :136
      qy = qy < 0 ? 0 : (qy > H - 1 ? H - 1 : qy);
      const size_t rowq = static_cast<size_t>(qy - a.g.row_base) * W;
      const float4 cq4 = a.in[rowq + qx];
      const f3 cq = xyz(cq4);
      f3 nq;
      if constexpr (PX) {
        nq = xyz(a.normals[rowq + qx]);
      } else {
        const uint32_t idq = a.vis[rowq + qx];
        nq = xyz(a.normal_tab[idq]);
      }
      const float wn = pow_sigma(glsl_max(0.0f, exact::dot(np, nq)), a.sigma_n);  // :62
      const float w = edge_weight<EXACT>(es, wn, cp, cq, dp, cq4.w, use_var, vg);
      const float h = gauss ? gauss5(i, j) * (1.0f / 273.0f) : 1.0f / 9.0f;  // :145
      const float hw = h * w;
      tap_add_h(num, den, hw, cq);
      if (use_var) vsum = fmaf_(hw * hw, a.var_in[rowq + qx], vsum);
    }
  }
  const f3 filtered = normalise<true>(num, den);
  if (use_var && a.var_out) a.var_out[rowp + x] = vsum / (den * den);
  if (!FINAL) {
    a.out[rowp + x] = make_float4(filtered.x, filtered.y, filtered.z, a.alpha_zero ? 0.0f : dp);
    return;
  }
  int ppx, ppy;
  reproject_pixel(W, H, a.PVprev, idp, xyz(a.worldpos[rowp + x]), a.lut_prev, x, y, ppx, ppy);
  if (a.prev_pixel) a.prev_pixel[rowp + x] = make_int2(ppx, ppy);
  bool use_history = a.frame > 0;  // :251
  if (use_history && (a.ext & kExtDisocclusion))
    use_history = same_primitive_at(a.prev_vis, W, H, a.pvis_row_base, a.pvis_y0, a.pvis_y1, ppx, ppy, idp);
  f3 blend = filtered;  // :258
  if (use_history) {
    const f3 hc = history_at(ppx, ppy, W, a.hist_y0, a.hist_y1, a.history, a.hist_row_base);
    float alpha = a.alpha;
    if (a.ext & kExtAdaptiveAlpha) alpha = adaptive_alpha(alpha, a.gradient[rowp + x].x);
    blend = temporal_blend(filtered, hc, alpha);
  }
  a.out[rowp + x] = make_float4(blend.x, blend.y, blend.z, 0.0f);
}

// The comb kernel: its description, constants and body are atrous_comb.hpp's (the tracing launch runs the body too).

// RLOAD (FINAL, plain family only): the reprojected pixel comes from a.reproj_in, written by an earlier frame's final pass
// from the same world-position plane, id plane, LUT_PREV and PVprev (api_passes.hip: ReprojKey) — no world position, no LUT
// gather, no id read in the NRM variant, none of reproject_pixel's arithmetic.
template <int CWp, bool FINAL, bool EXACT, bool NRM = false, int R = 1, bool EXTA = false, bool VAR = false, bool RLOAD = false>
__global__ __launch_bounds__(kShThreads)
// the per-pixel-normal final pass sits at the edge of six waves per SIMD (79-81 VGPRs as the surrounding code changes;
// 142-147 us with six waves, 169-176 us with five at 4K): pin it.  Every other instantiation keeps what it gets.
__attribute__((amdgpu_waves_per_eu(FINAL && NRM && R == 1 && !EXTA && !VAR && !EXACT ? 6 : (FINAL && !NRM && R == 1 && !EXTA && !VAR && !EXACT ? (RLOAD ? RTPT_REPROJ_LOAD_WAVES : kFinalWaves) : 1))))
void k_atrous_comb_sh(AtrousArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
#if RTPT_TILE_TIMELINE
  SpanScope span_(FINAL ? 1u : 0u, false);
#endif
  comb_items<CWp, FINAL, EXACT, NRM, R, EXTA, VAR, RLOAD>(a, lds_raw);
}

// copy the G-buffer depth into the alpha channel of a colour plane (used when a plane was injected
// through rtpt_set_plane / rtpt_bind_plane and does not carry it yet)
__global__ __launch_bounds__(kThreads) void k_stamp_depth(FrameGeom g, float4* color, const float* depth) {
  const int x = blockIdx.x * kBlockX + threadIdx.x;
  const int y = g.y0 + blockIdx.y * kBlockY + threadIdx.y;
  if (x >= g.W || y >= g.y1) return;
  const size_t i = static_cast<size_t>(y - g.row_base) * g.W + x;
  reinterpret_cast<float*>(color + i)[3] = depth[i];
}

__global__ __launch_bounds__(kThreads) void k_present(FrameGeom g, const float4* __restrict__ image, uint32_t* __restrict__ dst) {
  const int x = blockIdx.x * kBlockX + threadIdx.x;
  const int y = g.y0 + blockIdx.y * kBlockY + threadIdx.y;
  if (x >= g.W || y >= g.y1) return;
  const float4 c = image[static_cast<size_t>(y - g.row_base) * g.W + x];
  dst[static_cast<size_t>(y - g.y0) * g.W + x] = pack_bgra8(xyz(c), c.w);
}

// RTPT_FLAG_EXT_DEMODULATE.  The blit of the shaded frame without the shaded frame: the products are rounded to binary32 (the
// file is compiled -ffp-contract=off) and converted like k_present converts, so the bytes are the conversion of k_modulate's
// output; 36 B/px
__global__ __launch_bounds__(kThreads) void k_present_modulated(FrameGeom g, const float4* __restrict__ image, const float4* __restrict__ albedo,
                                                                uint32_t* __restrict__ dst) {
  const int x = blockIdx.x * kBlockX + threadIdx.x;
  const int y = g.y0 + blockIdx.y * kBlockY + threadIdx.y;
  if (x >= g.W || y >= g.y1) return;
  const size_t i = static_cast<size_t>(y - g.row_base) * g.W + x;
  const float4 c = image[i], al = albedo[i];
  dst[static_cast<size_t>(y - g.y0) * g.W + x] = pack_bgra8(f3{c.x * al.x, c.y * al.y, c.z * al.z}, 0.0f);
}

// shaded = (image.rgb * albedo.rgb, 0): one pixel per lane, two 16-byte loads and one 16-byte store, a wave covers 1 KiB of
// each row; the grid is the 64 x 4 tiles of the rows asked for
__global__ __launch_bounds__(kThreads) void k_modulate(FrameGeom g, const float4* __restrict__ image, const float4* __restrict__ albedo,
                                                       float4* __restrict__ shaded) {
  const int x = blockIdx.x * kBlockX + threadIdx.x;
  const int y = g.y0 + blockIdx.y * kBlockY + threadIdx.y;
  if (x >= g.W || y >= g.y1) return;
  const size_t i = static_cast<size_t>(y - g.row_base) * g.W + x;
  const float4 c = image[i], al = albedo[i];
  shaded[i] = make_float4(c.x * al.x, c.y * al.y, c.z * al.z, 0.0f);
}

}  // namespace

#if RTPT_TILE_TIMELINE
#define RTPT_SPAN_HOST
#include "experiments/span_instrumentation.inc"
#undef RTPT_SPAN_HOST
#endif

void launch_present(const FrameGeom& g, const float4* image, const float4* albedo, uint32_t* dst, hipStream_t s) {
  if (g.y1 <= g.y0) return;
  if (albedo)
    hipLaunchKernelGGL(k_present_modulated, grid_for(g), dim3(kBlockX, kBlockY), 0, s, g, image, albedo, dst);
  else
    hipLaunchKernelGGL(k_present, grid_for(g), dim3(kBlockX, kBlockY), 0, s, g, image, dst);
}

void launch_modulate(const FrameGeom& g, const float4* image, const float4* albedo, float4* shaded, hipStream_t s) {
  if (g.y1 <= g.y0) return;
  hipLaunchKernelGGL(k_modulate, grid_for(g), dim3(kBlockX, kBlockY), 0, s, g, image, albedo, shaded);
}

void launch_var_prefilter(const FrameGeom& g, int rows_stored, const float* var, float* out, hipStream_t s) {
  if (g.y1 <= g.y0) return;
  hipLaunchKernelGGL(k_var_prefilter, grid_for(g), dim3(kBlockX, kBlockY), 0, s, g, rows_stored, var, out);
}

void launch_moments(const MomentsArgs& a, hipStream_t s) {
  if (a.g.y1 <= a.g.y0) return;
  hipLaunchKernelGGL(k_moments, grid_for(a.g), dim3(kBlockX, kBlockY), 0, s, a);
}

void launch_stamp_depth(const FrameGeom& g, float4* color, const float* depth, hipStream_t s) {
  if (g.y1 <= g.y0) return;
  hipLaunchKernelGGL(k_stamp_depth, grid_for(g), dim3(kBlockX, kBlockY), 0, s, g, color, depth);
}

// THE two lists of k_atrous_comb_sh instantiations (each x FINAL x EXACT): the plain family (id-pair table or per-pixel
// normals, 3x3 taps; a staged row is 64 + 2 k cells) and the extension family (EXTA; id-pair table only; 64 + 2 R s cells,
// R = 2: 5x5 taps; VAR: the variance plane staged too).  prepare_device_atrous() raises the LDS limit of every entry;
// launch_atrous() and ext_staged() take the narrowest row that holds a launch's halo from them.
template <int CW, bool NRM, int R = 1, bool EXTA = false, bool VAR = false>
struct CombInst {
  static constexpr int cw = CW, r = R;
  static constexpr bool nrm = NRM, exta = EXTA, var = VAR;
};
constexpr int kCombW = kBlockX * kShHalves;  // pixels per wave row
using CombInsts = type_list<CombInst<kCombW + 8, false>, CombInst<kCombW + 16, false>, CombInst<kCombW + 32, false>,
                            CombInst<kCombW + 8, true>, CombInst<kCombW + 16, true>, CombInst<kCombW + 32, true>>;
using CombExtInsts = type_list<CombInst<72, false, 1, true, false>, CombInst<96, false, 1, true, false>,
                               CombInst<72, false, 1, true, true>, CombInst<96, false, 1, true, true>,
                               CombInst<72, false, 2, true, false>, CombInst<96, false, 2, true, false>, CombInst<128, false, 2, true, false>,
                               CombInst<72, false, 2, true, true>, CombInst<96, false, 2, true, true>, CombInst<128, false, 2, true, true>>;
// the narrowest staged row (cells) the list has for (nrm, r, var) that holds `need` cells; 0: none
template <class... E>
constexpr int comb_row(type_list<E...>, int need, bool nrm, int r, bool var) {
  int cw = 0;
  ((cw = E::nrm == nrm && E::r == r && E::var == var && E::cw >= need && (cw == 0 || E::cw < cw) ? E::cw : cw), ...);
  return cw;
}
static_assert(comb_row(CombInsts{}, kCombW + 2 * 16, false, 1, false) != 0 && comb_row(CombInsts{}, kCombW + 2 * 16, true, 1, false) != 0,
              "launch_atrous() stages every stride up to 16");
// RL: the final pass that loads the cached reprojection; only the FINAL instances of the plain family have one (for every
// other entry RL names the instance without it)
template <class I, class FIN, class EX, class RL = std::false_type>
constexpr auto comb_kernel(I, FIN, EX, RL = {}) {
  return &k_atrous_comb_sh<I::cw, FIN::value, EX::value, I::nrm, I::r, I::exta, I::var, RL::value && FIN::value && !I::exta>;
}

// Kernels that ask for more than 64 KiB of dynamic LDS need the attribute raised once per DEVICE (it is a
// property of the function on the current device, not of the process): rtpt_create calls this after
// hipSetDevice, so contexts on different GPUs of one process are independent.
hipError_t prepare_device_atrous() {
  hipError_t e = hipSuccess;
  auto raise = [&](auto inst) {
    each_final_exact([&](auto fin, auto ex) {
      for (const void* f : {reinterpret_cast<const void*>(comb_kernel(inst, fin, ex)), reinterpret_cast<const void*>(comb_kernel(inst, fin, ex, std::true_type{}))})
        if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    });
  };
  visit_all(CombExtInsts{}, raise);
  visit_all(CombInsts{}, raise);
  return e;
}
// the entry (cw, nrm, r, var) of `list`, FINAL x EXACT as asked; false: the list has no such entry
template <class List>
static bool launch_comb(List list, int cw, bool nrm, int r, bool var, bool final_pass, dim3 grid, size_t lds, const AtrousArgs& a, hipStream_t s) {
  return visit_first(list, [&](auto inst) {
    using I = decltype(inst);
    if (I::cw != cw || I::nrm != nrm || I::r != r || I::var != var) return false;
    with_final_exact(final_pass, a.exact != 0, [&](auto fin, auto ex) {
      with_bool(final_pass && !I::exta && a.reproj_in, [&](auto rl) {
        hipLaunchKernelGGL(comb_kernel(inst, fin, ex, rl), grid, dim3(kBlockX, kShWaves), lds, s, a);
      });
    });
    return true;
  });
}

// true when a FINAL launch of `a` runs in the LDS-staged kernel, whose epilogue can also write the swapchain format
// (AtrousArgs::present); every other final variant leaves the blit to k_present
// the extension modes run LDS-staged (k_atrous_comb_sh<..., R, EXTA>) when the scene has an id-pair table and the halo
// 2 R s fits the widest staged row: every flag combination, final pass included (round 3; before: tap shapes of k < N only)
static int ext_row(const AtrousArgs& a) {  // the staged row of an extension-mode launch, 0: its halo fits none
  const int R = (a.ext & kExtGauss5) ? 2 : 1;
  return comb_row(CombExtInsts{}, kBlockX + 2 * R * a.stride, false, R, (a.ext & kExtVariance) && a.var_in);
}
static bool ext_staged(const AtrousArgs& a) {
  const int np = static_cast<int>(a.n_tris) + 1;
  return a.ext && !a.direct && a.pair_tab && np <= kPairMax && a.stride >= 1 && ext_row(a) != 0;
}
bool atrous_final_fuses_present(const AtrousArgs& a) {
  const int np = static_cast<int>(a.n_tris) + 1;
  const bool pair_mode = a.pair_tab && np <= kPairMax;
  if (a.ext) return ext_staged(a);
  // (pair mode only: the per-pixel-normal final pass does not carry the store — register budget, see the kernel)
  return !a.direct && pair_mode && a.k >= 1 && a.k <= 16;
}

// Workgroups per XCD of the persistent comb kernel: every resident slot, but no more workgroups than work items (an XCD takes an
// eighth of the list and deals it to its workgroups item by item).  Giving every workgroup the same number of items instead
// (1 050 workgroups x 2 items rather than 2 048 slots for the 2 100 items of a strip's final pass) was measured in round 4
// and changes nothing (strip final 22.0 -> 23.1 us, 4K 110.8 -> 106.8, within the spread): the launch is bound by bytes in
// flight, not by its last items.
static uint32_t comb_blocks_per_xcd(uint32_t nlb, uint32_t slots_per_xcd) {
  const uint32_t items_xcd = (nlb + 7u) / 8u;
  return slots_per_xcd > items_xcd ? (items_xcd ? items_xcd : 1u) : (slots_per_xcd ? slots_per_xcd : 1u);
}

bool atrous_final_plain_comb(const AtrousArgs& a) {
  const int np = static_cast<int>(a.n_tris) + 1;
  const bool pair_mode = a.pair_tab && np <= kPairMax;
  const bool nrm_mode = !pair_mode && a.normals != nullptr;
  return !a.ext && !a.direct && (pair_mode || nrm_mode) && a.k >= 1 && a.k <= 16;
}

// what launch_atrous() sets for a launch of the plain comb kernel over a's rows: the fast weights' factors and the work list's shape
static void comb_list(AtrousArgs& a) {
  a.cz = -1.44269504088896341f / a.sigma_z;
  a.cl = -1.44269504088896341f / a.sigma_l;
  a.tiles_x = (a.g.W + kCombW - 1) / kCombW;
  const int nrows = a.g.y1 - a.g.y0;
  const int chunks = (nrows + kCombM * a.k - 1) / (kCombM * a.k);
  a.tiles_y = (chunks + kShWaves - 1) / kShWaves;  // chunk groups (kShWaves consecutive chunks per block)
}
bool atrous_final_role(AtrousArgs& a) {
  const int np = static_cast<int>(a.n_tris) + 1;
  if (!(atrous_final_plain_comb(a) && a.pair_tab && np <= kPairMax && !a.exact && a.k <= kFinalRoleMaxK && a.stride == a.k && a.g.y1 > a.g.y0 &&
        a.reproj_in && !a.reproj_out && !a.prev_pixel && !a.present))
    return false;
  comb_list(a);
  return true;
}

void launch_atrous(const AtrousArgs& a0, bool final_pass, hipStream_t s, bool px_normals) {
  if (a0.g.y1 <= a0.g.y0) return;
  if (px_normals && (!a0.normals || a0.pair_tab)) std::abort();  // (api_passes.hip: filter_launch sees to both)
  AtrousArgs a = a0;
  a.cz = -1.44269504088896341f / a.sigma_z;
  a.cl = -1.44269504088896341f / a.sigma_l;
  dim3 block(kBlockX, kBlockY);
  const int np = static_cast<int>(a.n_tris) + 1;
  {
    // the extension modes run LDS-staged when the scene has an id-pair table and the halo 2*R*s fits a staged row the
    // kernel is instantiated for — tap shapes, variance guidance and the final pass's adaptive alpha / disocclusion test
    // alike (round 3); what does not fit runs in the generic direct-load kernel k_atrous_ext (same arithmetic)
    const int R = (a.ext & kExtGauss5) ? 2 : 1, sk = a.stride;
    if (ext_staged(a)) {
      const int seg_w = kBlockX;
      a.tiles_x = (a.g.W + seg_w - 1) / seg_w;
      const int nrows = a.g.y1 - a.g.y0;
      const int chunks = (nrows + kCombM * sk - 1) / (kCombM * sk);
      a.tiles_y = (chunks + kShWaves - 1) / kShWaves;
      const int n_cu = a.n_cu > 0 ? a.n_cu : 256;
      const uint32_t nlb = static_cast<uint32_t>(a.tiles_x) * static_cast<uint32_t>(a.tiles_y) * static_cast<uint32_t>(sk);
      const int cw = ext_row(a);  // != 0: ext_staged()
      const bool use_var = (a.ext & kExtVariance) && a.var_in;
      const size_t lds = static_cast<size_t>((np * np * 4 + 15) & ~15) + static_cast<size_t>(kShWaves * kCombM + 2 * R) * cw * (use_var ? 24 : 20);
      uint32_t per_cu = static_cast<uint32_t>((160u * 1024u) / lds);
      if (per_cu > 32u / kShWaves) per_cu = 32u / kShWaves;
      if (per_cu < 1u) per_cu = 1u;
      const uint32_t per_xcd = comb_blocks_per_xcd(nlb, static_cast<uint32_t>((n_cu + 7) / 8) * per_cu);
      if (!launch_comb(CombExtInsts{}, cw, false, R, use_var, final_pass, dim3(per_xcd * 8u), lds, a, s)) std::abort();  // unreachable: cw is an entry's
      return;
    }
  }
  if (a.ext) {
    const dim3 g2 = grid_for(a.g);
    a.tiles_x = static_cast<int32_t>(g2.x);
    a.tiles_y = static_cast<int32_t>(g2.y);
    dim3 grid(g2.x * g2.y);
    with_final_exact(final_pass, a.exact != 0, [&](auto fin, auto ex) {
      with_bool(px_normals, [&](auto px) {
        hipLaunchKernelGGL((k_atrous_ext<decltype(fin)::value, decltype(ex)::value, decltype(px)::value>), grid, block, 0, s, a);
      });
    });
    return;
  }
  const bool pair_mode = a.pair_tab && np <= kPairMax;
  const bool nrm_mode = !pair_mode && a.normals != nullptr;
  if (atrous_final_plain_comb(a)) {
    comb_list(a);
    const int n_cu = a.n_cu > 0 ? a.n_cu : 256;  // of the context's device (rtpt_create)
    const uint32_t nlb = static_cast<uint32_t>(a.tiles_x) * static_cast<uint32_t>(a.tiles_y) * static_cast<uint32_t>(a.k);
    // staged row stride (cells): segment + 2k, rounded to the template instances (k <= 16: one fits)
    const int cw = comb_row(CombInsts{}, kCombW + 2 * a.k, nrm_mode, 1, false);
    const size_t lds = nrm_mode ? static_cast<size_t>(kShWaves * kCombM + 2) * cw * 32
                                : static_cast<size_t>((np * np * 4 + 15) & ~15) + static_cast<size_t>(kShWaves * kCombM + 2) * cw * 20;
    // persistent grid: as many blocks per CU as 160 KiB of LDS and 32 waves admit
    uint32_t per_cu = static_cast<uint32_t>((160u * 1024u) / lds);
    if (per_cu > 32u / kShWaves) per_cu = 32u / kShWaves;
    if (per_cu < 1u) per_cu = 1u;
    const uint32_t per_xcd = comb_blocks_per_xcd(nlb, static_cast<uint32_t>((n_cu + 7) / 8) * per_cu);
    if (!launch_comb(CombInsts{}, cw, nrm_mode, 1, false, final_pass, dim3(per_xcd * 8u), lds, a, s)) std::abort();  // unreachable: cw is an entry's
    return;
  }
  const dim3 g2 = grid_for(a.g);
  a.tiles_x = static_cast<int32_t>(g2.x);
  a.tiles_y = static_cast<int32_t>(g2.y);
  dim3 grid(g2.x * g2.y);
  with_final_exact(final_pass, a.exact != 0, [&](auto fin, auto ex) {
    with_bool(px_normals, [&](auto px) {
      hipLaunchKernelGGL((k_atrous<decltype(fin)::value, decltype(ex)::value, decltype(px)::value>), grid, block, 0, s, a);
    });
  });
}

}  // namespace rt
