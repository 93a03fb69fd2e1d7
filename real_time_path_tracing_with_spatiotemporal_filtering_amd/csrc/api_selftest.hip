// api_selftest.hip — what needs a context and is nothing a frame calls: the self tests of the device arithmetic, of the traversal
// and of the sampler (rtpt_selftest_*), and the checks of the acceleration structure as it stands on the device
// (rtpt_debug_bvh_*).  The context-free helpers (rtpt_util_*) are api_util.hip's.
#include "api_internal.hpp"
#include "texture_host.hpp"

extern "C" {

// ------------------------------------------------------------------------------------------ self tests
int rtpt_selftest_math(rtpt_ctx* c, int op, const float* in, float* out, size_t n) {
  if (!c || !in || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  float *din = nullptr, *dout = nullptr;
  HIP_TRY(hipMalloc(&din, n * 4));
  if (hipMalloc(&dout, n * 4) != hipSuccess) {
    (void)hipFree(din);
    return fail(RTPT_E_NOMEM, "hipMalloc");
  }
  hipError_t e = hipMemcpyAsync(din, in, n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_math(op, din, dout, n, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(din);
  (void)hipFree(dout);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_math: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_exhaustive(rtpt_ctx* c, int op, uint64_t* mismatches, uint32_t first_bad[4]) {
  if (!c || !mismatches) return fail(RTPT_E_INVALID, "NULL argument");
  if (op != 3 && op != 4) return fail(RTPT_E_INVALID, "rtpt_selftest_exhaustive: op must be 3 (sqrt) or 4 (1/x)");
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long* d = nullptr;
  HIP_TRY(hipMalloc(&d, 5 * sizeof(unsigned long long)));
  unsigned long long h[5] = {0, 0, 0, 0, 0};
  hipError_t e = hipMemsetAsync(d, 0, sizeof h, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_exhaustive(op, d, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_exhaustive: ") + hipGetErrorString(e));
  *mismatches = h[0];
  if (first_bad)
    for (int i = 0; i < 4; i++) first_bad[i] = static_cast<uint32_t>(h[1 + i]);
  return RTPT_OK;
}

int rtpt_selftest_div(rtpt_ctx* c, int mode, uint32_t first_pass, uint32_t n_passes, uint64_t* mismatches, uint32_t first_bad[2]) {
  if (!c || !mismatches) return fail(RTPT_E_INVALID, "NULL argument");
  if (mode < 0 || mode > 3)
    return fail(RTPT_E_INVALID, "rtpt_selftest_div: mode must be 0 (significand pairs), 1 (arbitrary bits), 2 (quotient_positive, arbitrary bits) or 3 (div2_, arbitrary bits)");
  if (mode == 0 && (first_pass >= 256u || n_passes > 256u - first_pass))
    return fail(RTPT_E_INVALID, "rtpt_selftest_div: the enumeration has 256 passes");
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long* d = nullptr;
  HIP_TRY(hipMalloc(&d, 3 * sizeof(unsigned long long)));
  unsigned long long h[3] = {0, 0, 0};
  hipError_t e = hipMemsetAsync(d, 0, sizeof h, c->stream);
  for (uint32_t p = 0; e == hipSuccess && p < n_passes; p++) {
    rt::launch_selftest_div(mode, first_pass + p, d, c->stream);
    e = hipGetLastError();
    if (e == hipSuccess && (p & 7u) == 7u) e = hipStreamSynchronize(c->stream);  // ~0.15 s per pass: keep the queue short
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_div: ") + hipGetErrorString(e));
  *mismatches = h[0];
  if (first_bad) {
    first_bad[0] = static_cast<uint32_t>(h[1]);
    first_bad[1] = static_cast<uint32_t>(h[2]);
  }
  return RTPT_OK;
}

int rtpt_selftest_contract(rtpt_ctx* c, int fn, const uint32_t* in, uint32_t* out, size_t n) {
  if (!c || !in || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (fn < 0 || fn >= rt::kContractFns) return fail(RTPT_E_INVALID, "rtpt_selftest_contract: no such fn (the table of include/rtpt.h)");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t in_bytes = n * rt::kContractWords[fn][0] * 4, out_bytes = n * rt::kContractWords[fn][1] * 4;
  Buf din, dout;
  int rc;
  if ((rc = alloc_buf(din, in_bytes)) || (rc = alloc_buf(dout, out_bytes))) return rc;
  hipError_t e = hipMemcpyAsync(din.ptr, in, in_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_contract(fn, static_cast<const uint32_t*>(din.ptr), static_cast<uint32_t*>(dout.ptr), n, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_contract: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_bounce(rtpt_ctx* c, const float* in, float* out, size_t n) {
  if (!c || !in || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t in_bytes = n * 9 * sizeof(float), out_bytes = n * 4 * sizeof(float);
  Buf din, dout;
  int rc;
  if ((rc = alloc_buf(din, in_bytes)) || (rc = alloc_buf(dout, out_bytes))) return rc;
  hipError_t e = hipMemcpyAsync(din.ptr, in, in_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_bounce(static_cast<const float*>(din.ptr), static_cast<float*>(dout.ptr), n, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_bounce: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_refract(rtpt_ctx* c, const float* in, float* out, size_t n) {
  if (!c || !in || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t in_bytes = n * 9 * sizeof(float), out_bytes = n * 5 * sizeof(float);
  Buf din, dout;
  int rc;
  if ((rc = alloc_buf(din, in_bytes)) || (rc = alloc_buf(dout, out_bytes))) return rc;
  hipError_t e = hipMemcpyAsync(din.ptr, in, in_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_refract(static_cast<const float*>(din.ptr), static_cast<float*>(dout.ptr), n, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_refract: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_light_sample(rtpt_ctx* c, const uint32_t* in, uint32_t* out, size_t n) {
  if (!c || !in || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t in_bytes = n * 19 * sizeof(uint32_t), out_bytes = n * 9 * sizeof(uint32_t);
  Buf din, dout;
  int rc;
  if ((rc = alloc_buf(din, in_bytes)) || (rc = alloc_buf(dout, out_bytes))) return rc;
  hipError_t e = hipMemcpyAsync(din.ptr, in, in_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_light_sample(static_cast<const uint32_t*>(din.ptr), static_cast<uint32_t*>(dout.ptr), n, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_light_sample: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_sphere_sample(rtpt_ctx* c, const uint32_t* in, uint32_t* out, size_t n) {
  if (!c || !in || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t in_bytes = n * 12 * sizeof(uint32_t), out_bytes = n * 6 * sizeof(uint32_t);
  Buf din, dout;
  int rc;
  if ((rc = alloc_buf(din, in_bytes)) || (rc = alloc_buf(dout, out_bytes))) return rc;
  hipError_t e = hipMemcpyAsync(din.ptr, in, in_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_sphere_sample(static_cast<const uint32_t*>(din.ptr), static_cast<uint32_t*>(dout.ptr), n, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_sphere_sample: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_mis_weight(rtpt_ctx* c, const float* in, float* out, size_t n) {
  if (!c || !in || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t in_bytes = n * 20 * sizeof(float), out_bytes = n * 3 * sizeof(float);
  Buf din, dout;
  int rc;
  if ((rc = alloc_buf(din, in_bytes)) || (rc = alloc_buf(dout, out_bytes))) return rc;
  hipError_t e = hipMemcpyAsync(din.ptr, in, in_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_mis_weight(static_cast<const float*>(din.ptr), static_cast<float*>(dout.ptr), n, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_mis_weight: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_shading_normal(rtpt_ctx* c, const float* in, float* out, size_t n) {
  if (!c || !in || !out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t in_bytes = n * 36 * sizeof(float), out_bytes = n * 8 * sizeof(float);
  Buf din, dout;
  int rc;
  if ((rc = alloc_buf(din, in_bytes)) || (rc = alloc_buf(dout, out_bytes))) return rc;
  hipError_t e = hipMemcpyAsync(din.ptr, in, in_bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_shading_normal(static_cast<const float*>(din.ptr), static_cast<float*>(dout.ptr), n, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout.ptr, out_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_shading_normal: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_environment(rtpt_ctx* c, const float* dirs, size_t n, float* rgb_out) {
  if (!c || !dirs || !rgb_out) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->envmap.texels.ptr) return fail(RTPT_E_INVALID, "the context has no environment map (rtpt_set_environment)");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = n * 3 * sizeof(float);
  Buf din, dout;
  int rc;
  if ((rc = alloc_buf(din, bytes)) || (rc = alloc_buf(dout, bytes))) return rc;
  hipError_t e = hipMemcpyAsync(din.ptr, dirs, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_environment(env_view(c), static_cast<const float*>(din.ptr), n, static_cast<float*>(dout.ptr), c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(rgb_out, dout.ptr, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_environment: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_light_find(rtpt_ctx* c, const uint32_t* ids, size_t n, const uint32_t* queries, size_t k, uint32_t* index_out) {
  if (!c || !queries || !index_out || (n && !ids)) return fail(RTPT_E_INVALID, "NULL argument");
  if (n > (static_cast<size_t>(1) << 24)) return fail(RTPT_E_INVALID, "a light list has at most 2^24 entries");
  if (k == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  Buf dids, dq, di;
  int rc;
  if ((n && (rc = alloc_buf(dids, n * sizeof(uint32_t)))) || (rc = alloc_buf(dq, k * sizeof(uint32_t))) || (rc = alloc_buf(di, k * sizeof(uint32_t))))
    return rc;
  hipError_t e = n ? hipMemcpyAsync(dids.ptr, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) : hipSuccess;
  if (e == hipSuccess) e = hipMemcpyAsync(dq.ptr, queries, k * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_light_find(static_cast<const uint32_t*>(dids.ptr), static_cast<uint32_t>(n), static_cast<const uint32_t*>(dq.ptr), k,
                                   static_cast<uint32_t*>(di.ptr), c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(index_out, di.ptr, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_light_find: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_light_table(rtpt_ctx* c, const float* w, size_t n, uint64_t* cdf_out) {
  if (!c || !w || !cdf_out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0) return RTPT_OK;
  if (n > (static_cast<size_t>(1) << 24)) return fail(RTPT_E_INVALID, "a light table has at most 2^24 entries");
  HIP_TRY(hipSetDevice(c->device));
  Buf dw, dcdf, scratch;
  int rc;
  if ((rc = alloc_buf(dw, n * sizeof(float))) || (rc = alloc_buf(dcdf, n * sizeof(uint64_t))) ||
      (rc = alloc_buf(scratch, rt::light_table_scratch_bytes(n))))
    return rc;
  hipError_t e = hipMemcpyAsync(dw.ptr, w, n * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_light_table_weights(static_cast<const float*>(dw.ptr), n, static_cast<uint64_t*>(dcdf.ptr), scratch.ptr, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(cdf_out, dcdf.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_light_table: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_light_pick(rtpt_ctx* c, const uint64_t* cdf, size_t n, const float* u_l, size_t k, uint32_t* index_out, float* inv_p_out) {
  if (!c || !cdf || !u_l || !index_out || !inv_p_out) return fail(RTPT_E_INVALID, "NULL argument");
  if (n == 0 || n > (static_cast<size_t>(1) << 24)) return fail(RTPT_E_INVALID, "a light table has 1 to 2^24 entries");
  if (k == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  Buf dcdf, du, di, dp;
  int rc;
  if ((rc = alloc_buf(dcdf, n * sizeof(uint64_t))) || (rc = alloc_buf(du, k * sizeof(float))) || (rc = alloc_buf(di, k * sizeof(uint32_t))) ||
      (rc = alloc_buf(dp, k * sizeof(float))))
    return rc;
  hipError_t e = hipMemcpyAsync(dcdf.ptr, cdf, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(du.ptr, u_l, k * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_light_pick(static_cast<const uint64_t*>(dcdf.ptr), static_cast<uint32_t>(n), static_cast<const float*>(du.ptr), k,
                                   static_cast<uint32_t*>(di.ptr), static_cast<float*>(dp.ptr), c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(index_out, di.ptr, k * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(inv_p_out, dp.ptr, k * sizeof(float), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_light_pick: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_trace(rtpt_ctx* c, const float* rays, size_t n, uint32_t* out_id, float* out_t) {
  if (!c || !rays || !out_id) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);  // a recorded G-buffer call holds the scene view, and with it the stack's spill area, which may move below
  float *drays = nullptr, *dt = nullptr;
  uint32_t* did = nullptr;
  hipError_t e = hipMalloc(&drays, n * 24);
  if (e == hipSuccess) e = hipMalloc(&did, n * 4);
  if (e == hipSuccess) e = hipMalloc(&dt, n * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(drays, rays, n * 24, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    if (int rcs = ensure_stack_spill(c, std::max(frame_blocks(c), (n + 255) / 256))) {
      (void)hipFree(drays);
      (void)hipFree(did);
      (void)hipFree(dt);
      return rcs;
    }
    rt::launch_selftest_trace(scene_view(c), drays, n, c->cfg.ray_tmax, did, dt, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out_id, did, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && out_t) e = hipMemcpyAsync(out_t, dt, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(drays);
  (void)hipFree(did);
  (void)hipFree(dt);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_trace: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_texture(rtpt_ctx* c, uint32_t texture, const float* uv, size_t n, float* rgba_out) {
  if (!c || !uv || !rgba_out) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  const Scene::Textures& t = c->scene.textures;
  if (!t.desc.ptr || texture >= t.n_textures) return fail(RTPT_E_INVALID, "no such texture (rtpt_scene_set_textures)");
  for (size_t i = 0; i < 2 * n; i++)
    if (!std::isfinite(uv[i])) return fail(RTPT_E_INVALID, "a uv coordinate is not finite");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  Buf duv, dout;
  int rc;
  if ((rc = alloc_buf(duv, n * 8)) || (rc = alloc_buf(dout, n * 16))) return rc;
  hipError_t e = hipMemcpyAsync(duv.ptr, uv, n * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_texture(static_cast<const rt::TexDesc*>(t.desc.ptr) + texture, static_cast<const float4*>(t.texels.ptr),
                                static_cast<const float*>(duv.ptr), n, static_cast<float4*>(dout.ptr), c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(rgba_out, dout.ptr, n * 16, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_texture: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_texture_lod(rtpt_ctx* c, uint32_t texture, const float* uv, const float* lod, size_t n, float* rgba_out) {
  if (!c || !uv || !lod || !rgba_out) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  const Scene::Textures& t = c->scene.textures;
  if (!t.desc.ptr || texture >= t.n_textures) return fail(RTPT_E_INVALID, "no such texture (rtpt_scene_set_textures)");
  for (size_t i = 0; i < 2 * n; i++)
    if (!std::isfinite(uv[i])) return fail(RTPT_E_INVALID, "a uv coordinate is not finite");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  Buf duv, dlod, dout, drow;
  int rc;
  if ((rc = alloc_buf(duv, n * 8)) || (rc = alloc_buf(dlod, n * 4)) || (rc = alloc_buf(dout, n * 16))) return rc;
  // a scene without any mip chain has no level table: its textures have the one level of their descriptor
  const uint32_t* row = t.levels.ptr ? static_cast<const uint32_t*>(t.levels.ptr) + static_cast<size_t>(rtpt_tex::kLevelRow) * texture : nullptr;
  uint32_t one_level[rtpt_tex::kLevelRow] = {};
  hipError_t e = hipSuccess;
  if (!row) {
    rtpt_texture d;
    if ((rc = alloc_buf(drow, sizeof one_level))) return rc;
    e = hipMemcpy(&d, static_cast<const rtpt_texture*>(t.desc.ptr) + texture, sizeof d, hipMemcpyDeviceToHost);
    one_level[0] = d.first_texel;
    one_level[rtpt_tex::kLevelRowCount] = 1;
    if (e == hipSuccess) e = hipMemcpyAsync(drow.ptr, one_level, sizeof one_level, hipMemcpyHostToDevice, c->stream);
    row = static_cast<const uint32_t*>(drow.ptr);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(duv.ptr, uv, n * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dlod.ptr, lod, n * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_texture_lod(static_cast<const rt::TexDesc*>(t.desc.ptr) + texture, row, static_cast<const float4*>(t.texels.ptr),
                                    static_cast<const float*>(duv.ptr), static_cast<const float*>(dlod.ptr), n, static_cast<float4*>(dout.ptr),
                                    c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(rgba_out, dout.ptr, n * 16, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // one_level is read by its copy until here
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_texture_lod: ") + hipGetErrorString(e));
  return RTPT_OK;
}

int rtpt_selftest_texture_footprint(rtpt_ctx* c, const float* rays, size_t n, uint32_t bounce, uint32_t* out_id, float* out_lod) {
  if (!c || !rays || !out_id || !out_lod) return fail(RTPT_E_INVALID, "NULL argument");
  if (bounce > 1) return fail(RTPT_E_INVALID, "bounce is 0 (the rule of segment 0) or 1 (of every later segment)");
  if (!c->scene.n_tris) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  if (n == 0) return RTPT_OK;
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);  // as rtpt_selftest_trace
  Buf drays, did, dlod;
  int rc;
  if ((rc = alloc_buf(drays, n * 24)) || (rc = alloc_buf(did, n * 4)) || (rc = alloc_buf(dlod, n * 4))) return rc;
  if ((rc = ensure_stack_spill(c, std::max(frame_blocks(c), (n + 255) / 256)))) return rc;
  hipError_t e = hipMemcpyAsync(drays.ptr, rays, n * 24, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    rt::launch_selftest_footprint(scene_view(c), tex_view(c), static_cast<const float*>(drays.ptr), n, c->cfg.ray_tmax, bounce == 0,
                                  c->cfg.fov_slope, static_cast<int>(c->cfg.height), static_cast<uint32_t*>(did.ptr),
                                  static_cast<float*>(dlod.ptr), c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out_id, did.ptr, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_lod, dlod.ptr, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(RTPT_E_DEVICE, std::string("selftest_texture_footprint: ") + hipGetErrorString(e));
  return RTPT_OK;
}

// ------------------------------------------------------------------------------------------ the tree on the device
// The acceleration structure AS IT STANDS ON THE DEVICE (after rtpt_scene_upload, or after a model matrix re-posed and
// refit it inside rtpt_gbuffer): nodes, grid, posed triangles and leaf order are read back and checked on the host.
//   stats[0] nodes, [1] leaves, [2] deepest level, [3] largest leaf, [4] triangles not referenced exactly once,
//   [5] decoded (origin + q * cell, binary32) child boxes that do not contain every vertex below them,
//   [6] child boxes wider than the padded scene (a box that was never rewritten), [7] dangling references
int rtpt_debug_bvh_check(rtpt_ctx* c, uint64_t stats[8]) {
  if (!c || !stats) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris || !c->scene.tree.nodes.ptr) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  const uint32_t n = c->scene.n_tris, nn = c->scene.tree.n_nodes;
  std::vector<rt::BvhNodeQ> q(nn);
  std::vector<float> tris(static_cast<size_t>(n) * 9);
  std::vector<uint32_t> leaf(n);
  float g[8];
  HIP_TRY(hipMemcpyAsync(q.data(), c->scene.tree.nodes.ptr, q.size() * sizeof(rt::BvhNodeQ), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(tris.data(), c->scene.tris.ptr, tris.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(leaf.data(), c->scene.tree.leaf_order.ptr, leaf.size() * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(g, c->scene.bvh_grid_dev.ptr, sizeof g, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int i = 0; i < 8; i++) stats[i] = 0;
  stats[0] = nn;
  std::vector<uint32_t> seen(n, 0);
  for (uint32_t id : leaf) {
    if (id >= n)
      stats[4]++;
    else
      seen[id]++;
  }
  for (uint32_t i = 0; i < n; i++)
    if (seen[i] != 1) stats[4]++;
  struct Bounds { float mn[3], mx[3]; };
  std::vector<Bounds> sub(nn);
  std::vector<uint8_t> done(nn, 0);
  std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}};  // node, level
  while (!st.empty()) {
    const uint32_t ni = st.back().first, lvl = st.back().second;
    stats[2] = std::max<uint64_t>(stats[2], lvl);
    const rt::BvhNodeQ& nd = q[ni];
    bool ready = true;
    for (uint32_t ref : {nd.lref, nd.rref}) {
      if (ref == rt::kBvhEmpty || (ref & 0x80000000u)) continue;
      if (ref >= nn || ref <= ni) {  // pre-order: a child comes after its parent
        stats[7]++;
        continue;
      }
      if (!done[ref]) {
        st.push_back({ref, lvl + 1});
        ready = false;
      }
    }
    if (!ready) continue;
    st.pop_back();
    Bounds me{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
    for (int side = 0; side < 2; side++) {
      const uint32_t ref = side ? nd.rref : nd.lref;
      if (ref == rt::kBvhEmpty) continue;
      Bounds cb{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
      if (ref & 0x80000000u) {
        const uint32_t first = (ref & 0x7FFFFFFFu) >> 2, cnt = (ref & 3u) + 1u;
        stats[1]++;
        stats[3] = std::max<uint64_t>(stats[3], cnt);
        if (static_cast<uint64_t>(first) + cnt > n) {
          stats[7]++;
          continue;
        }
        if (c->scene.tree.leaf_pairs && !rt::pair_leaf_ok(first, cnt, leaf.data(), n)) stats[7]++;  // read as ONE pair record
        for (uint32_t j = 0; j < cnt; j++)
          for (int v = 0; v < 3; v++)
            for (int a = 0; a < 3; a++) {
              const float x = tris[9 * static_cast<size_t>(leaf[first + j]) + 3 * v + a];
              cb.mn[a] = std::min(cb.mn[a], x);
              cb.mx[a] = std::max(cb.mx[a], x);
            }
      } else {
        if (ref >= nn || !done[ref]) continue;
        cb = sub[ref];
      }
      for (int a = 0; a < 3; a++) {
        const float qlo = std::fmaf(static_cast<float>(nd.box[rt::bvh_box_lo(side, a)]), g[3 + a], g[a]);  // the decode refit.hip checks against
        const float qhi = std::fmaf(static_cast<float>(nd.box[rt::bvh_box_hi(side, a)]), g[3 + a], g[a]);  // the decode refit.hip checks against
        if (!(qlo <= cb.mn[a] && qhi >= cb.mx[a])) stats[5]++;
        me.mn[a] = std::min(me.mn[a], cb.mn[a]);
        me.mx[a] = std::max(me.mx[a], cb.mx[a]);
      }
    }
    sub[ni] = me;
    done[ni] = 1;
  }
  // no child box may be wider than the root's: the grid spans the padded scene plus one cell at either end
  if (nn) {
    const Bounds& sc = sub[0];
    float diag = 0.f, mag = 0.f;
    for (int a = 0; a < 3; a++) {
      diag += (sc.mx[a] - sc.mn[a]) * (sc.mx[a] - sc.mn[a]);
      mag = std::max(mag, std::max(std::fabs(sc.mn[a]), std::fabs(sc.mx[a])));
    }
    const float pad = 1e-5f * std::max(std::sqrt(diag), mag);  // bvh.cpp / refit.hip: the padding of every box
    for (uint32_t ni = 0; ni < nn; ni++)
      for (int side = 0; side < 2; side++) {
        if ((side ? q[ni].rref : q[ni].lref) == rt::kBvhEmpty) continue;
        for (int a = 0; a < 3; a++) {
          const float slack = 4.0f * g[3 + a] + 2.0f * pad;
          const float qlo = std::fmaf(static_cast<float>(q[ni].box[rt::bvh_box_lo(side, a)]), g[3 + a], g[a]);  // the decode refit.hip checks against
          const float qhi = std::fmaf(static_cast<float>(q[ni].box[rt::bvh_box_hi(side, a)]), g[3 + a], g[a]);  // the decode refit.hip checks against
          if (qlo < sc.mn[a] - slack || qhi > sc.mx[a] + slack) stats[6]++;
        }
      }
  }
  return RTPT_OK;
}

int rtpt_debug_bvh_topology(rtpt_ctx* c, uint32_t* child_refs, uint32_t* n_nodes, uint32_t* leaf_order, uint32_t* n_leaf_ids) {
  if (!c || !n_nodes || !n_leaf_ids) return fail(RTPT_E_INVALID, "NULL argument");
  if (!c->scene.n_tris || !c->scene.tree.nodes.ptr) return fail(RTPT_E_NO_SCENE, "rtpt_scene_upload has not been called");
  const uint32_t n = c->scene.n_tris, nn = c->scene.tree.n_nodes;
  if (!child_refs && !leaf_order) {
    *n_nodes = nn;
    *n_leaf_ids = n;
    return RTPT_OK;
  }
  if (!child_refs || !leaf_order) return fail(RTPT_E_INVALID, "both arrays, or neither");
  if (*n_nodes < nn || *n_leaf_ids < n) return fail(RTPT_E_INVALID, "arrays shorter than the counts the first call returned");
  HIP_TRY(hipSetDevice(c->device));
  FLUSH_FILTER(c);
  std::vector<rt::BvhNodeQ> q(nn);
  HIP_TRY(hipMemcpyAsync(q.data(), c->scene.tree.nodes.ptr, q.size() * sizeof(rt::BvhNodeQ), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(leaf_order, c->scene.tree.leaf_order.ptr, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (uint32_t i = 0; i < nn; i++) {
    child_refs[2 * static_cast<size_t>(i)] = q[i].lref;
    child_refs[2 * static_cast<size_t>(i) + 1] = q[i].rref;
  }
  *n_nodes = nn;
  *n_leaf_ids = n;
  return RTPT_OK;
}

}  // extern "C"
