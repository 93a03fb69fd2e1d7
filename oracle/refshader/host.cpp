/*
 * ORACLE — TEST INFRASTRUCTURE ONLY.
 *
 * host.cpp — runs the reference's compute shader text (translated by prep.py into <name>.gen.hpp, which exist only
 * under oracle/_ref/) on the CPU, one invocation per grid point, the way vkCmdDispatch would: the grid is the image
 * size rounded up to the workgroup size, so the out-of-image early returns and temporalGradient's store-before-check
 * (D10) are executed; out-of-image stores are dropped and out-of-image loads return 0 (D2).
 *
 * Compiled once per arithmetic (-DREFSHADER_REAL=float -DREFSHADER_SUF=f32 / double, f64); plane arguments are arrays
 * of that Real with the layouts of oracle/oracle.py's wrappers.  Images are held in Real, so R64 does not round at an
 * imageStore: it is the high-precision reading of the arithmetic, not a model of rgba32f storage.
 */
#include "glsl_compat.hpp"

#include "../rtpt_oracle.h"

#include "raytrace.gen.hpp"
#include "temporal_gradient.gen.hpp"
#include "temporal_filter.gen.hpp"

#include <limits>

using namespace glsl;

#define CAT2(a, b) a##b
#define CAT(a, b) CAT2(a, b)
#define ENTRY(name) CAT(CAT(name, _), REFSHADER_SUF)

namespace {

typedef uint32_t (*closest_fn)(const float*, uint32_t, const float*, const float*, float, float*, float*, float*);
closest_fn g_contract_closest = nullptr;  // the oracle's exported closest hit (contract ray-triangle routine, D4)

/* R32: the contract's routine.  The ray query is the driver's black box, not shader text. */
uint32_t closest_contract(const accelerationStructureEXT& as, vec3 o, vec3 d, Real tmax, Real* t, Real* b1, Real* b2) {
  float oo[3] = {(float)o.x, (float)o.y, (float)o.z}, dd[3] = {(float)d.x, (float)d.y, (float)d.z};
  float ft = 0.f, f1 = 0.f, f2 = 0.f;
  uint32_t id = g_contract_closest(as.tris, as.n, oo, dd, (float)tmax, &ft, &f1, &f2);
  *t = (Real)ft; *b1 = (Real)f1; *b2 = (Real)f2;
  return id;
}

/* R64: Moller & Trumbore 1997 as printed, in double; both faces, 0 < t < tmax; ties keep the lower id (D4). */
uint32_t closest_textbook(const accelerationStructureEXT& as, vec3 o, vec3 d, Real tmax, Real* t_out, Real* b1, Real* b2) {
  uint32_t best = 0;
  double bt = 0, bu = 0, bv = 0;
  const double O[3] = {(double)o.x, (double)o.y, (double)o.z}, D[3] = {(double)d.x, (double)d.y, (double)d.z};
  for (uint32_t i = 0; i < as.n; i++) {
    const float* T = as.tris + 9 * (size_t)i;
    double e1[3], e2[3], tv[3], p[3], q[3];
    for (int k = 0; k < 3; k++) { e1[k] = (double)T[3 + k] - (double)T[k]; e2[k] = (double)T[6 + k] - (double)T[k]; tv[k] = O[k] - (double)T[k]; }
    p[0] = D[1] * e2[2] - D[2] * e2[1]; p[1] = D[2] * e2[0] - D[0] * e2[2]; p[2] = D[0] * e2[1] - D[1] * e2[0];
    double det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
    if (!(det != 0.0)) continue;
    double u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) / det;
    if (!(u >= 0.0) || !(u <= 1.0)) continue;
    q[0] = tv[1] * e1[2] - tv[2] * e1[1]; q[1] = tv[2] * e1[0] - tv[0] * e1[2]; q[2] = tv[0] * e1[1] - tv[1] * e1[0];
    double v = (D[0] * q[0] + D[1] * q[1] + D[2] * q[2]) / det;
    if (!(v >= 0.0) || !(u + v <= 1.0)) continue;
    double t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) / det;
    if (!(t > 0.0) || !(t < (double)tmax)) continue;
    if (best == 0 || t < bt) { best = i + 1; bt = t; bu = u; bv = v; }
  }
  if (best) { *t_out = (Real)bt; *b1 = (Real)bu; *b2 = (Real)bv; }
  return best;
}

template <class PC>
void fill_pc(PC& d, const oracle_push_constants* s) {
  d.sample_batch = s->sample_batch;
  d.frameNumber = s->frameNumber;
  d.cameraPos = vec3((Real)s->cameraPos[0], (Real)s->cameraPos[1], (Real)s->cameraPos[2]);
  d.lightPos = vec3((Real)s->lightPos[0], (Real)s->lightPos[1], (Real)s->lightPos[2]);
  d.lightPosPrev = vec3((Real)s->lightPosPrev[0], (Real)s->lightPosPrev[1], (Real)s->lightPosPrev[2]);
  d.currentCameraColor = vec3((Real)s->currentCameraColor[0], (Real)s->currentCameraColor[1], (Real)s->currentCameraColor[2]);
  d.previousCameraColor = vec3((Real)s->previousCameraColor[0], (Real)s->previousCameraColor[1], (Real)s->previousCameraColor[2]);
  d.waveletIteration = s->waveletIteration;
  d.maxWaveletIteration = s->maxWaveletIteration;
}

/* visibility LUT: (n+1) records of three vec3 at 16-byte offsets (stride 48 B), as oracle_lut writes them */
template <class VD>
std::vector<VD> fill_lut(const float* lut, uint32_t n_records) {
  std::vector<VD> v(n_records);
  for (uint32_t i = 0; i < n_records; i++) {
    const float* p = lut + 12 * (size_t)i;
    v[i].v1 = vec3((Real)p[0], (Real)p[1], (Real)p[2]);
    v[i].v2 = vec3((Real)p[4], (Real)p[5], (Real)p[6]);
    v[i].v3 = vec3((Real)p[8], (Real)p[9], (Real)p[10]);
  }
  return v;
}

image2D make_image(int w, int h, int chan, const Real* load, Real* store) {
  image2D im;
  im.w = w; im.h = h; im.chan = chan; im.load = load; im.store = store;
  return im;
}

mat4 make_mat(const float* m) {
  mat4 r;
  for (int j = 0; j < 4; j++)
    for (int i = 0; i < 4; i++) r.c[j][i] = (Real)m[4 * j + i];
  return r;
}

template <class S, class F>
void dispatch(S& sh, int w, int h, int wgw, int wgh, F&& per_invocation) {
  const int gw = (w + wgw - 1) / wgw * wgw, gh = (h + wgh - 1) / wgh * wgh;
  for (int y = 0; y < gh; y++)
    for (int x = 0; x < gw; x++) {
      sh.gl_GlobalInvocationID.x = (uint)x;
      sh.gl_GlobalInvocationID.y = (uint)y;
      sh.gl_GlobalInvocationID.z = 0;
      per_invocation(x, y);
    }
}

}  // namespace

extern "C" {

void ENTRY(ref_set_closest_hit)(void* fn) { g_contract_closest = (closest_fn)fn; }
int ENTRY(ref_real_bytes)(void) { return (int)sizeof(Real); }

/* the text's RNG and Box-Muller, callable on their own (raytrace.comp.glsl:71-92) */
void ENTRY(ref_rng_floats)(uint32_t* state, int n, Real* out) {
  raytrace::Shader sh;
  uint s = *state;
  for (int i = 0; i < n; i++) out[i] = sh.stepAndOutputRNGFloat(s);
  *state = s;
}
void ENTRY(ref_random_gaussian)(uint32_t* state, Real* out2) {
  raytrace::Shader sh;
  uint s = *state;
  vec2 g = sh.randomGaussian(s);
  out2[0] = g.x; out2[1] = g.y;
  *state = s;
}

/* K2.  image: H*W*4.  Per pixel the host records every ray query of the invocation: seq_id[H*W*max_rec] (id + 1, 0 =
 * none), seq_t (nullable), seq_n[H*W] = number of queries, dir0[H*W*3] (nullable) = direction of the first query,
 * seq_od[H*W*max_rec*6] (nullable) = origin and direction of every query.
 * returns the total number of queries. */
uint64_t ENTRY(ref_raytrace)(uint32_t w, uint32_t h, const oracle_push_constants* pc, const float* tris, uint32_t n,
                             int max_segments, int num_samples, Real* image, uint16_t* seq_id, Real* seq_t, int32_t* seq_n,
                             int max_rec, Real* dir0, Real* seq_od) {
  raytrace::Shader sh;
  sh.ref_max_segments = max_segments;
  sh.ref_num_samples = num_samples;
  fill_pc(sh.pushConstants, pc);
  sh.storageImage = make_image((int)w, (int)h, 4, nullptr, image);
  /* the shader reads world-space vertices through an index buffer: triangle i = vertices 3i, 3i+1, 3i+2 */
  std::vector<vec3> verts(3 * (size_t)n);
  std::vector<uint> idx(3 * (size_t)n);
  for (size_t i = 0; i < 3 * (size_t)n; i++) {
    verts[i] = vec3((Real)tris[3 * i], (Real)tris[3 * i + 1], (Real)tris[3 * i + 2]);
    idx[i] = (uint)i;
  }
  sh.vertices = verts.data();
  sh.indices = idx.data();
  std::vector<RayRecord> rec;
  sh.tlas.tris = tris;
  sh.tlas.n = n;
  sh.tlas.record = &rec;
  sh.tlas.closest = REFSHADER_IS_F32 ? closest_contract : closest_textbook;
  if (REFSHADER_IS_F32 && !g_contract_closest) return ~0ull;
  uint64_t total = 0;
  dispatch(sh, (int)w, (int)h, raytrace::WG_W, raytrace::WG_H, [&](int x, int y) {
    rec.clear();
    sh.main_invocation();
    if (x >= (int)w || y >= (int)h) return;
    size_t i = (size_t)y * w + x;
    total += rec.size();
    seq_n[i] = (int32_t)rec.size();
    for (size_t k = 0; k < rec.size() && (int)k < max_rec; k++) {
      seq_id[i * max_rec + k] = (uint16_t)rec[k].id;
      if (seq_t) seq_t[i * max_rec + k] = rec[k].t;
      if (seq_od) {
        Real* q = seq_od + 6 * (i * max_rec + k);
        q[0] = rec[k].o.x; q[1] = rec[k].o.y; q[2] = rec[k].o.z; q[3] = rec[k].d.x; q[4] = rec[k].d.y; q[5] = rec[k].d.z;
      }
    }
    if (dir0 && !rec.empty()) { dir0[3 * i] = rec[0].d.x; dir0[3 * i + 1] = rec[0].d.y; dir0[3 * i + 2] = rec[0].d.z; }
  });
  return total;
}

/* K1.  vis: H*W ids; worldpos H*W*4; lut / lut_prev n_records*12 floats; grad H*W*4 (the caller pre-fills it with a
 * sentinel: the shader's own :119 store has to clear it) */
void ENTRY(ref_temporal_gradient)(uint32_t w, uint32_t h, const oracle_push_constants* pc, const uint32_t* vis, const Real* worldpos,
                                  const float* lut, const float* lut_prev, uint32_t n_records, Real* grad) {
  temporal_gradient::Shader sh;
  fill_pc(sh.pushConstants, pc);
  std::vector<Real> visf((size_t)w * h);
  for (size_t i = 0; i < visf.size(); i++) visf[i] = (Real)vis[i];
  auto l0 = fill_lut<temporal_gradient::Shader::VisibilityData>(lut, n_records);
  auto l1 = fill_lut<temporal_gradient::Shader::VisibilityData>(lut_prev, n_records);
  sh.visibilitylut = l0.data();
  sh.visibilitylutPrev = l1.data();
  sh.visibilityBuffer = make_image((int)w, (int)h, 1, visf.data(), nullptr);
  sh.worldPosImage = make_image((int)w, (int)h, 4, worldpos, nullptr);
  sh.storageImage = make_image((int)w, (int)h, 4, nullptr, grad);
  dispatch(sh, (int)w, (int)h, temporal_gradient::WG_W, temporal_gradient::WG_H, [&](int, int) { sh.main_invocation(); });
}

/* K3, one iteration (pc->waveletIteration of pc->maxWaveletIteration).
 *   in        colorImage as the pass finds it (H*W*4)
 *   filtered  storageImage stores (:152)
 *   blend     colorImage stores (:263); the caller pre-fills it with NaN, pixels never stored keep it
 *   prev_pixel  2 ints per pixel: coordinate of the previousFrameImage load (:253); untouched where no load happened
 *   serial_in_place != 0: D1 NOT applied — colorImage loads and stores share one buffer (a copy of `in`, returned in
 *   `blend`) and the invocations run in plain raster order: one possible outcome of the race the reference has. */
void ENTRY(ref_temporal_filter)(uint32_t w, uint32_t h, const oracle_push_constants* pc, const oracle_ubo* ubo, const Real* in,
                                const Real* depth, const uint32_t* vis, const float* lut, const float* lut_prev, uint32_t n_records,
                                const Real* worldpos, const Real* history, Real* filtered, Real* blend, int32_t* prev_pixel,
                                int serial_in_place) {
  temporal_filter::Shader sh;
  fill_pc(sh.pushConstants, pc);
  sh.ubo.model = make_mat(ubo->model); sh.ubo.view = make_mat(ubo->view); sh.ubo.proj = make_mat(ubo->proj);
  sh.ubo.modelPrev = make_mat(ubo->modelPrev); sh.ubo.viewPrev = make_mat(ubo->viewPrev); sh.ubo.projPrev = make_mat(ubo->projPrev);
  std::vector<Real> visf((size_t)w * h);
  for (size_t i = 0; i < visf.size(); i++) visf[i] = (Real)vis[i];
  auto l0 = fill_lut<temporal_filter::Shader::VisibilityData>(lut, n_records);
  auto l1 = fill_lut<temporal_filter::Shader::VisibilityData>(lut_prev, n_records);
  sh.visibilitylut = l0.data();
  sh.visibilitylutPrev = l1.data();
  if (serial_in_place) memcpy(blend, in, sizeof(Real) * 4 * (size_t)w * h);
  sh.storageImage = make_image((int)w, (int)h, 4, nullptr, filtered);
  sh.colorImage = make_image((int)w, (int)h, 4, serial_in_place ? blend : in, blend);
  sh.depthImage = make_image((int)w, (int)h, 1, depth, nullptr);
  sh.visibilityBuffer = make_image((int)w, (int)h, 1, visf.data(), nullptr);
  sh.previousFrameImage = make_image((int)w, (int)h, 4, history, nullptr);
  sh.worldPosImage = make_image((int)w, (int)h, 4, worldpos, nullptr);
  sh.temporalGradient = make_image((int)w, (int)h, 4, nullptr, nullptr);
  dispatch(sh, (int)w, (int)h, temporal_filter::WG_W, temporal_filter::WG_H, [&](int x, int y) {
    sh.previousFrameImage.n_loads = 0;
    sh.main_invocation();
    if (x >= (int)w || y >= (int)h || !prev_pixel || !sh.previousFrameImage.n_loads) return;
    size_t i = (size_t)y * w + x;
    prev_pixel[2 * i] = sh.previousFrameImage.last_load.x;
    prev_pixel[2 * i + 1] = sh.previousFrameImage.last_load.y;
  });
}

}  // extern "C"
