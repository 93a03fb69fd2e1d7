/*
 * rtpt.h — C ABI of the MI355X-native hot path (G-buffer -> temporal gradient -> 1-spp path
 * trace -> N edge-stopping a-trous passes with reprojection + temporal blend).
 *
 * The reference (OnurBasci/Real_Time_Path_Tracing_With_SpatioTemporal_Filtering) has no FFI:
 * its seam is the Vulkan compute dispatch (pipeline + descriptor set + 112-byte push
 * constants + grid).  Every entry point below replaces one such dispatch site (or the
 * resource/scene call that feeds it) and cites it as `file:line` relative to the reference
 * tree.  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 (RTPT_OK) or a negative RTPT_E_* code; the message is
 *     available from rtpt_last_error().  No exception crosses the ABI.
 *     (reference: NVVK_CHECK aborts / std::runtime_error never caught, main.cpp:99-111,:1532)
 *   - all work is enqueued on ONE HIP stream per context in program order, which gives the
 *     same observable ordering as the reference's vkQueueWaitIdle after each dispatch
 *     (main.cpp:110-111) without the waits.  rtpt_sync / rtpt_readback are the blocking calls.
 *   - a context is not thread-safe; distinct contexts (one per GPU) are independent.
 *   - images are linear row-major, element (x,y) of a plane at index (y-row_begin)*width+x.
 */
#ifndef RTPT_H
#define RTPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTPT_ABI_VERSION 5

/* ---- status codes -------------------------------------------------------------------- */
#define RTPT_OK 0
#define RTPT_E_INVALID (-1)  /* bad argument / bad call order */
#define RTPT_E_NOMEM (-2)    /* host or device allocation failed */
#define RTPT_E_DEVICE (-3)   /* HIP runtime error (message in rtpt_last_error) */
#define RTPT_E_NO_SCENE (-4) /* a pass needs rtpt_scene_upload first */
#define RTPT_E_NO_GPU (-5)   /* no HIP device visible: the product path never falls back to CPU */

/* ---- structs shared with the reference host -------------------------------------------- */

/* PushConstants — main.cpp:35-49, raytrace.comp.glsl:9-23 (identical copies in
 * temporalGradient.comp.glsl:11-25 and temporalFiltering.comp.glsl:11-25).
 * Offsets 0,4,16,32,48,64,80,92,96, sizeof 112 (verified against the three .spv). */
typedef struct rtpt_push_constants {
  uint32_t sample_batch;        /* @0  */
  uint32_t frameNumber;         /* @4  */
  uint32_t _pad0[2];
  float cameraPos[3];           /* @16 */
  float _pad1;
  float lightPos[3];            /* @32 */
  float _pad2;
  float lightPosPrev[3];        /* @48 */
  float _pad3;
  float currentCameraColor[3];  /* @64 */
  float _pad4;
  float previousCameraColor[3]; /* @80 */
  int32_t waveletIteration;     /* @92 */
  int32_t maxWaveletIteration;  /* @96 */
  uint32_t _pad5[3];
} rtpt_push_constants;

/* UniformBufferObject — main.cpp:82-90, temporalFiltering.comp.glsl:43-51,
 * visibility.vert.glsl:3-11.  Six column-major mat4 (m[col][row]) @0,64,...,320. */
typedef struct rtpt_ubo {
  float model[16];
  float view[16];
  float proj[16];
  float modelPrev[16];
  float viewPrev[16];
  float projPrev[16];
} rtpt_ubo;

/* VisibilityData — temporalGradient.comp.glsl:5-9 (std430: vec3 padded to 16, stride 48).
 * LUT[t+1] holds the world-space vertices of triangle t; LUT[0] is the background slot
 * (visibility.geom.glsl:56-59). */
typedef struct rtpt_visibility_data {
  float v1[3];
  float _p1;
  float v2[3];
  float _p2;
  float v3[3];
  float _p3;
} rtpt_visibility_data;

/* ---- configuration: the reference's compile-time constants made explicit ---------------- */
#define RTPT_FLAG_EXACT_FILTER 0x1u /* strict-parity filter: contract exp/sqrt/div instead of the
                                       hardware v_exp/v_sqrt/v_rcp (slower; bit-identical to the oracle) */
#define RTPT_FLAG_FORCE_BVH 0x2u    /* traverse the BVH even for scenes small enough for the
                                       wave-uniform brute-force path (<= 64 triangles) */

#define RTPT_FLAG_DIRECT_FILTER 0x4u /* a-trous taps by direct global loads instead of the LDS-staged
                                       tile kernel (the fallback for strides whose halo exceeds LDS) */

#define RTPT_FLAG_NO_PATH_COMPACTION 0x8u /* path tracer: keep one pixel per lane for the whole path instead of
                                            compacting the surviving paths of a tile after every segment */

#define RTPT_FLAG_SINGLE_LAUNCH_PATHS 0x200u /* path tracer: run all segments of a path in the tile kernel instead of
                                              handing the paths that survive 4 / 8 / 16 segments to follow-up launches
                                              through a queue (A/B switch; the image is the same) */

#define RTPT_FLAG_NO_FILTER_FUSION 0x400u /* launch every pass when it is called, one kernel per call, instead of
                                             recording rtpt_temporal_filter's calls of a frame (consecutive iterations
                                             then run chained in one launch) and rtpt_gbuffer (which runs in one launch
                                             with the rtpt_temporal_gradient that follows it) (A/B switch; same pixels) */

/* Extension modes — NOT reference behaviour, default off.  They switch on the pieces of the textbook
 * A-SVGF that the reference declares but leaves unused; any of them routes K3 to a
 * generic direct-load kernel.  They cannot be parity-checked against the reference; tests/ check them
 * against the oracle's restatement of the same definitions. */
#define RTPT_FLAG_EXT_ADAPTIVE_ALPHA 0x10u /* alpha = (1-g)*alpha + g, g = temporalGradient.r
                                              (temporalFiltering.comp.glsl:247-248, commented out there) */
#define RTPT_FLAG_EXT_GAUSS5 0x20u         /* 5x5 taps weighted by gaussianKernel2D/273 (:93-99, unused there) */
#define RTPT_FLAG_EXT_POW2_STRIDE 0x40u    /* tap stride 2^(k-1) instead of k (:135) */
#define RTPT_FLAG_EXT_DISOCCLUSION 0x80u   /* blend history only where the reprojected pixel of the previous
                                              frame's id plane (previousVisibilityBuffer, main.cpp:1367: copied,
                                              never read) shows the same primitive */
#define RTPT_FLAG_EXT_VARIANCE 0x100u      /* SVGF-style variance guidance: before the first filter iteration the first
                                              and second moments of the traced luminance are accumulated along the
                                              reprojected pixel (history only where the previous id plane agrees;
                                              a = max(alpha, 1/(n+1)); short histories n < 4 scale the variance by
                                              4/n); the colour term of the tap weight becomes
                                              exp(-|lum_p - lum_q| / (sigma_l * sqrt(var_p) + 1e-4)) and the variance
                                              is filtered along with weights (h w)^2.  RTPT_PLANE_MOMENTS / _VARIANCE.
                                              On strip contexts every stored row must have been traced (redundant
                                              halo rows), and under camera motion the host gathers the previous
                                              frame's id and moment rows the strip can reach from the other strips
                                              (rtpt_set_external_guides) like it does for the history image. */

#define RTPT_FLAG_EXT_SVGF_VARIANCE 0x800u /* with RTPT_FLAG_EXT_VARIANCE (required), the two pieces of SVGF's variance handling
                                              (Schied et al. 2017) that flag leaves out: a pixel whose moment history is shorter
                                              than 4 frames takes its variance from the 7x7 neighbourhood of the current frame's
                                              luminance (taps on the same primitive only) instead of the temporal estimate, still
                                              scaled by 4/n; and the variance that scales an iteration's luminance weight is the 3x3
                                              Gaussian (1 2 1 / 2 4 2 / 1 2 1) / 16 of the variance plane around the pixel.
                                              On strip contexts the traced rows must reach 3 rows beyond every row whose variance
                                              an iteration reads (the hosts' strip plans do that: strips.py / host/strips.cpp). */

#define RTPT_FLAG_DEVICE_BVH_BUILD 0x1000u /* rtpt_scene_upload builds the tree on the device (csrc/bvh_build.hip: a linear BVH
                                              over 63-bit Morton keys) instead of running the 32-bin SAH builder on one CPU
                                              thread.  Same node format, same traversal, same pixels (boxes only cull and
                                              order); what changes is cost: the upload no longer stalls for the host build
                                              (0.3 s of tree construction for 1,152,000 triangles), and a Morton tree traces somewhat
                                              slower than the SAH tree.  RTPT_DEVICE_BVH=1 in rtpt_create's environment sets it
                                              too.  A device-built tree has no host copy: it is always refit on the device,
                                              RTPT_HOST_REFIT does not apply to it.  ABI version 5 */
#define RTPT_FLAG_DEVICE_BVH_SAH 0x2000u   /* together with RTPT_FLAG_DEVICE_BVH_BUILD (alone it is ignored): the device build is
                                              the SAH builder of csrc/bvh_build_sah.hip, a level-synchronous restatement of the
                                              host's 32-bin SAH builder that reproduces the host's tree node for node (same
                                              child references, same leaf order up to the order inside a two-triangle leaf), so
                                              the frame costs what it costs with the host-built tree (measured equal within the
                                              run-to-run spread) and the build runs on the device.
                                              rtpt_scene_upload and rtpt_scene_rebuild both use it; it blocks one to three times
                                              per level of the tree for a readback of a few words.  No depth fallback: the tree has
                                              the host tree's (bounded) depth.  RTPT_DEVICE_BVH=sah in rtpt_create's environment
                                              sets both bits.  Purely additive (a flag bit, a builder value, one debug entry
                                              point): the ABI version stays 5 */

#define RTPT_FLAG_DEVICE_FLATTEN 0x4000u   /* together with RTPT_FLAG_DEVICE_BVH_BUILD (alone it is ignored, like the SAH bit), for
                                              scenes of more than 64 triangles (smaller ones need the triangles on the host for
                                              their screen bounds and keep the host path): rtpt_scene_upload copies only the mesh
                                              and the instance transforms (12 n_verts + 12 n_tris + 48 n_instances bytes), expands
                                              them into triangles and detects the fan pairs on the device (csrc/scene_flatten.hip:
                                              the host's arithmetic and the host's memcmp, so the same bits and the same decision),
                                              then builds there.  One word (paired or not) is read back before the build.  If the
                                              LBVH comes back deeper than the stack the upload falls back to the host path in the
                                              same call (host flatten + host SAH, HOST_SAH / FALLBACK_DEPTH).  Same tree, same
                                              pixels; what changes is the cost of an upload.  Additive: the ABI version stays 5 */

#define RTPT_FLAG_EXT_DEMODULATE 0x8000u  /* albedo demodulation (SVGF, Schied et al. 2017; NOT reference behaviour, default off): the
                                              filter and the history run on ILLUMINATION, colour with the albedo of the primary
                                              surface divided out, so that a material border between coplanar surfaces (same
                                              normal, same depth: only the colour term stops there, weakly) stays sharp.
                                              rtpt_raytrace leaves out the multiply by the first hit's albedo (raytrace.comp.glsl:244
                                              at segment 0) and stores that albedo in RTPT_PLANE_ALBEDO instead; a path that ends at
                                              its first query (analytic light, sky, emissive material) stores albedo (1, 1, 1) and the
                                              colour it has without the flag.  Colour without the flag = demodulated colour x ALBEDO up
                                              to the order of the multiplies; random stream, ray count and HIT_ID are the same.
                                              IMAGE, FILTERED, PREVIOUS and the blended history then hold demodulated colour; the
                                              filter kernels are the ones of the same flags without this bit (it is not an
                                              extension mode of K3: no wider halo, no other kernel).  rtpt_modulate writes the shaded
                                              frame to RTPT_PLANE_SHADED and rtpt_present multiplies on the fly.  ALBEDO is valid
                                              from rtpt_raytrace until the next rtpt_raytrace of the context, for the rows traced.
                                              samples_per_pixel > 1 with this flag is refused by rtpt_create (RTPT_E_INVALID): the
                                              mean of products is not the product of means, and the multi-sample accumulators in
                                              LDS have no room for a second sum.  Known limitation: a pixel on a material border
                                              takes the albedo this frame's jittered sample met, so it can alternate between the
                                              two materials from frame to frame (1-spp aliasing that the filter blurs away without
                                              the flag); ALBEDO is not accumulated over frames.  Additive: the ABI version stays 5 */

#define RTPT_FLAG_EXT_NEE 0x10000u /* next-event estimation (NOT reference behaviour, default off; DESIGN.md 8, csrc/light_sample.hpp states
                                      the rules): rtpt_raytrace samples the scene's emissive triangles.  rtpt_scene_set_materials and
                                      rtpt_scene_set_materials_ext build the LIGHT LIST beside the material records — id + 1 of every
                                      posed triangle whose material has Ke != 0, ascending; more than 2^24 of them are refused with
                                      the scene untouched (RTPT_E_INVALID).  Everything below holds only while the list has L > 0
                                      entries; without an emitter, without materials and without the flag the frames, the ray counts
                                      and the kernels are those of a context without it, bit for bit.
                                      At a DIFFUSE hit that is not the path's last segment (seg + 1 < max_segments), after the albedo
                                      went into the throughput T (or, at segment 0 with RTPT_FLAG_EXT_DEMODULATE, into ALBEDO), after
                                      the faceforward and the offset origin x, and before the bounce's two draws, three draws u_l,
                                      u_a, u_b pick entry min(uint(u_l * L), L - 1) and a point y uniform on that triangle; if x
                                      faces y and y's plane from a distance and the triangle has an area, ONE closest-hit query goes
                                      from x towards y (the path's own query: same tmax, same tie rule; counted in RAYCOUNT), and if
                                      it returns that triangle the pixel's radiance R gains (T * Ke) * g per channel, g = cos(x)
                                      cos(y) 2 area L / (2 pi r^2).  The hit sets the path's sampled bit, valid sample or not; a
                                      specular or dielectric hit takes no light draw and clears it; the primary ray starts with it
                                      clear.  A path that meets an emissive triangle with the bit set ends with colour 0 (its light
                                      was collected at the hit before), with the bit clear with T * Ke as without the flag.  The
                                      analytic sphere light, the sky and the end of the segment budget end a path as without the
                                      flag; none of them is sampled.  The pixel stores R + the path's terminal colour; with
                                      samples_per_pixel > 1 that sum goes into the sample mean and R restarts at 0 per sample.  With
                                      RTPT_FLAG_EXT_DEMODULATE the gain of segment 0 is illumination (T lacks the first albedo), so
                                      IMAGE x ALBEDO is the frame without that flag up to the order of the multiplies.
                                      Such a launch runs every segment in the tile kernel (as RTPT_FLAG_SINGLE_LAUNCH_PATHS) and
                                      carries no deferred final filter pass.  Instances moved, a rebuilt tree, a changed model and
                                      rtpt_resize keep the list; rtpt_scene_upload drops it with the materials.  Additive: the ABI
                                      version stays 5 */

#define RTPT_FLAG_EXT_NEE_SPHERE 0x20000u /* next-event estimation of the ANALYTIC SPHERE LIGHT (NOT reference behaviour, default off;
                                      DESIGN.md 8, csrc/light_sample.hpp states the rules and the arithmetic): independent of
                                      RTPT_FLAG_EXT_NEE and combinable with it; without it every frame, ray count and kernel is
                                      that of a context without it, bit for bit.
                                      At a DIFFUSE hit that is not the path's last segment (seg + 1 < max_segments), where the
                                      triangle sample sits — after the albedo, the faceforward and the offset origin x, before the
                                      bounce's two draws — two draws u_c, u_p (behind the triangle sample's three where that one is
                                      taken; drawn whether or not the sample is valid; a specular or dielectric hit and a last
                                      segment take none) pick a direction in the cone the light subtends from x:
                                      dc = c - x, d2 = dot(dc, dc), w = normalize(dc), q = r2 / d2, cm = sqrt(1 - q),
                                      k = q / (1 + cm), ct = fma(-u_c, k, 1), st = sqrt(max(0, fma(-ct, ct, 1))),
                                      (sp, cp) = sincos2pi(u_p), (t, b) the branch-free orthonormal pair around w that
                                      light_sample.hpp states, wd = normalize((st cp) t + (st sp) b + ct w), cs = dot(nf, wd).
                                      TAKEN when d2 > r2 (NaN fails, x inside or on the sphere fails); VALID when taken and cs > 0.
                                      A valid sample adds ((T.c * light_col.c) * g) per channel to the pixel's radiance R,
                                      g = (2 cs) k, light_col never light_col_first; no query is sent and no ray is counted (the
                                      reference's light is never occluded).  Where a hit takes both samples the sphere's gain goes
                                      into R first, the triangle's after its shadow query.  The path's SPHERE BIT is set by a
                                      diffuse non-last hit whose sample was taken, valid or not, cleared by one whose sample was not
                                      taken and by a specular or dielectric hit, and clear on the primary ray; a segment that meets
                                      the sphere light with the bit set ends the path with terminal colour 0, with the bit clear as
                                      without the flag.  The bit does not touch emissive triangles, RTPT_FLAG_EXT_NEE's sampled bit
                                      not the sphere.  With RTPT_FLAG_EXT_DEMODULATE the gain of segment 0 is illumination.
                                      Such a launch has the limits of a RTPT_FLAG_EXT_NEE launch, whatever the scene's materials:
                                      every segment in the tile kernel, no queue kernels, no deferred final filter pass.
                                      Additive: the ABI version stays 5 */

#define RTPT_FLAG_EXT_NEE_POWER 0x40000u /* next-event estimation picks its emissive triangle BY POWER, not uniformly (NOT reference
                                      behaviour, default off; DESIGN.md 8, csrc/light_sample.hpp states the rules and the
                                      arithmetic).  It works together with RTPT_FLAG_EXT_NEE on a scene whose light list has
                                      entries; alone, or with only RTPT_FLAG_EXT_NEE_SPHERE, it is ignored (as the SAH bit is
                                      without the build bit), and without it every frame, ray count, kernel and allocation is that
                                      of a context without it, bit for bit.  It combines with RTPT_FLAG_EXT_NEE_SPHERE, with
                                      demodulation, textures, samples_per_pixel > 1, strips and two frames in flight exactly where
                                      RTPT_FLAG_EXT_NEE does.  Every rule of RTPT_FLAG_EXT_NEE holds unchanged — the place of the
                                      sample, the three draws and their order, the sampled bit, the shadow query and its tie rule,
                                      R — except two: which entry the draw u_l names, and that float(L) in g becomes inv_p, the
                                      inverse of the pick's probability.
                                      Entry i (posed id, vertices from its shade record, Ke from material record (id - 1) %
                                      n_base_tris) weighs w_i = a2_i * k_i, a2_i the sample's a2 (twice the area), k_i =
                                      max(|Ke.r|, |Ke.g|, |Ke.b|); a w_i that is NaN, infinite or not > 0 counts as 0: a degenerate
                                      emitter is never picked.  w_max = max w_i.  q_i = 1 for every entry if w_max == 0 (the uniform
                                      pick), else max(1, uint32((w_i / w_max) * 65536.0f)) where w_i > 0 and 0 elsewhere.
                                      C_i = sum_{j <= i} q_j as uint64, S = C_{L-1} <= 2^40; 8 bytes an entry, on a context with both
                                      bits and L > 0 only, beside the builder's scratch.  Pick: m = uint32(u_l * 2^24),
                                      t = (uint64(m) * S) >> 24, the entry is the smallest i with C_i > t (binary search),
                                      inv_p = float(S) / float(q_i) (uint64 -> binary32 to nearest even, a correctly rounded
                                      division), g = ((cs * cl) * (a2 * inv_p)) / (2 pi * r2).
                                      The table is built on the device, on the context's stream, when the list joins the scene and
                                      after every re-pose (rtpt_scene_set_instances, a changed ubo.model, rtpt_scene_rebuild), so
                                      that it belongs to the posed triangles a trace reads; it is dropped with the list.
                                      Known limit: an entry with q_i * 2^24 < S can be skipped by every value of the draw (needs
                                      S > 2^24: hundreds of full-weight lights beside a tiny one); its share of the light is lost.
                                      Such a launch has the limits of a RTPT_FLAG_EXT_NEE launch.
                                      Additive: the ABI version stays 5 */

#define RTPT_FLAG_EXT_NEE_MIS 0x80000u /* next-event estimation WEIGHS its light sample against the bounce that meets the same emitter
                                      (multiple importance sampling with the POWER HEURISTIC, beta = 2; NOT reference behaviour,
                                      default off; DESIGN.md 8, csrc/light_sample.hpp states the rules and the arithmetic).  It works
                                      together with RTPT_FLAG_EXT_NEE on a scene whose light list has L > 0 entries, with the uniform
                                      or the weighted pick, and combines with RTPT_FLAG_EXT_NEE_SPHERE; alone, with only the sphere
                                      flag, or on an empty list it is ignored (as the POWER bit is without the NEE bit), and in every
                                      ignored case and without it every frame, ray count, kernel and allocation is that of a context
                                      without it, bit for bit.  Everything not named here is as RTPT_FLAG_EXT_NEE / _POWER state it:
                                      the place of the sample, the three draws and their order, the sampled bit, the shadow query and
                                      its tie rule, R, the order of the sphere's and the triangle's additions, demodulation.  THE
                                      SPHERE SAMPLE AND THE SPHERE BIT ARE UNCHANGED: the cone sample of a sphere is already close to
                                      the bounce's own density, and its weighing is left for later.
                                      With g2 = g * g: the light side weighs m(g) = 1 / (1 + g2), the bounce side wb(g) = g2 / (1 +
                                      g2) where g2 < +inf and 1 elsewhere (a NaN takes 1); g is the ratio of the bounce's density
                                      cos(x) / pi to the light sample's density in solid angle, so these are p_l^2 / (p_l^2 + p_b^2)
                                      and p_b^2 / (p_l^2 + p_b^2).
                                      1. The light sample's g becomes gm = g * m(g), one multiply behind the division; the gain is
                                      ((T.c * Ke.c) * gm) per channel; gm <= 0.5.  Validity, the query and the ray count are unchanged.
                                      2. A diffuse hit that is not the path's last segment and took the triangle draw records cb =
                                      dot(nf, d') of its normalised diffuse direction d'.  cb travels with the path like the sampled
                                      bit and is read only while that bit is set.
                                      3. An emissive triangle met with the sampled bit set ends the path with (T * Ke) * wb(g_hit) —
                                      the multiply by Ke as before, then one multiply by wb per channel — no longer with 0; with the
                                      bit clear with T * Ke as before.  g_hit = ((cb * cl) * (a2 * inv_p)) / (2 pi * r2) at the point
                                      the ray hit: y from the hit's barycentrics on its shade record, r2 = |y - o|^2, cl = |dot(nl,
                                      d)| with the ray's own d, a2 as the sample computes it; inv_p = float(L) for the uniform pick,
                                      for the weighted pick float(S) / float(q_i) of the hit triangle's entry i, found by binary
                                      search in the ascending list (every index read in [0, L)).  Where q_i == 0 (the pick never
                                      reaches that emitter) or the id is not in the list (which no frame can produce) wb = 1.
                                      Known limits, inherited: an entry the weighted pick's 24-bit draw can skip (q_i * 2^24 < S)
                                      still loses that share; such a launch has the limits of a RTPT_FLAG_EXT_NEE launch (every
                                      segment in the tile kernel, no queues, no deferred final filter pass).
                                      Additive: the ABI version stays 5 */

#define RTPT_FLAG_EXT_SMOOTH_GUIDE 0x100000u /* the filter's edge stop reads INTERPOLATED normals (NOT reference behaviour, default off;
                                      DESIGN.md 8, csrc/shading_normal.hpp states the rules G1-G5).  It is ACTIVE while the context has
                                      the flag and the scene holds normals (rtpt_scene_set_normals); in every other case it is ignored
                                      (as the POWER bit is without the NEE bit), and then every frame, plane, ray count, kernel and
                                      allocation is that of a context without it, bit for bit.
                                      While active, K0 (rtpt_gbuffer, alone or inside the tracing launch) writes, for every pixel whose
                                      pixel-centre ray hits a triangle, the GUIDE NORMAL into a per-pixel plane of 16 bytes a pixel,
                                      which the context then holds for any triangle count: the corner normals interpolated with K0's
                                      own barycentrics, carried through the hit instance's pose and normalised (rules 1-3 of smooth
                                      shading); the triangle's normal where the record is not smooth or the result is NaN, infinite or
                                      zero; turned to the side of the triangle's unfaced normal (inverted vn records and mirrored poses
                                      agree with their not-smooth neighbours); independent of the ray.  The cell's fourth word is
                                      pow(max(0, dot(ns, ns)), sigma_n).  Pixels that hit nothing keep (0, 0, 1).
                                      Every filter kernel then weighs a tap by pow(max(0, dot(n_p, n_q)), sigma_n) of the two pixels'
                                      cells: the LDS-staged per-pixel-normal kernel for every scene size (a scene of at most 63
                                      triangles is treated as if it had no id-pair table: no chained launches, no deferred final pass),
                                      the per-pixel form of the direct-load kernel for strides above 16 and RTPT_FLAG_DIRECT_FILTER, and
                                      the per-pixel form of the generic kernel for every RTPT_FLAG_EXT_* filter mode.  K1's Phong normal,
                                      the LUT, the reprojection, the same-primitive tests of RTPT_FLAG_EXT_DISOCCLUSION / _VARIANCE and
                                      the id plane keep the triangle's normal and id.
                                      STALE PLANE: a filter call whose rows read are not all covered by what K0 wrote of the plane in
                                      this frame (rtpt_set_plane(RTPT_PLANE_VIS_ID) is one cause: the plane no longer matches the ids)
                                      is filtered with the triangles' normals, by the kernels of a context without the flag.
                                      The guide is part of what frame reuse keys K0 on; rtpt_scene_set_normals, setting or removing,
                                      makes the next frame run K0 again.  Additive: the ABI version stays 5 */

typedef struct rtpt_config {
  uint32_t struct_size;          /* = sizeof(rtpt_config), ABI guard */
  uint32_t width, height;        /* full frame; main.cpp:52-53 (1000x800) */
  uint32_t row_begin, row_end;   /* rows stored by this context (0,height on one GPU);
                                    multi-GPU strips allocate strip +- halo rows */
  uint32_t max_segments;         /* raytrace.comp.glsl:204 (32) */
  uint32_t samples_per_pixel;    /* raytrace.comp.glsl:306 (1).  > 1 is an extension: every sample draws fresh bounce
                                    directions from one stream per pixel, whereas the reference text (rngState by value, :200)
                                    would replay sample 0's */
  int32_t sigma_n;               /* temporalFiltering.comp.glsl:203 (128; integer exponent) */
  float sigma_z;                 /* :204 (1.0) */
  float sigma_l;                 /* :205 (4.0) */
  float alpha;                   /* :243 (0.3) */
  float light_radius;            /* raytrace.comp.glsl:280 (0.20) */
  float light_intensity;         /* :281 (30) */
  float first_hit_light_divisor; /* :229 (5.0) */
  float fov_slope;               /* tan(FOV), common.h:16, raytrace.comp.glsl:300 (0.20271003) */
  float pixel_jitter;            /* :314 (0.375) */
  float ray_offset;              /* :250 (1e-4) */
  float ray_tmax;                /* :216 (10000) */
  uint32_t flags;
  int32_t device;                /* HIP device ordinal, -1 = current device */
} rtpt_config;

/* planes = the reference's images/buffers (createBuffers main.cpp:357-407) */
typedef enum rtpt_plane {
  RTPT_PLANE_IMAGE = 0,     /* `image`              RGBA32F  main.cpp:359 */
  RTPT_PLANE_FILTERED = 1,  /* `filteredImageBuffer` RGBA32F  main.cpp:400 */
  RTPT_PLANE_PREVIOUS = 2,  /* `previousImage`      RGBA32F  main.cpp:365 */
  RTPT_PLANE_WORLDPOS = 3,  /* `positionBuffer`     RGBA32F  main.cpp:383 */
  RTPT_PLANE_GRADIENT = 4,  /* `temporalGradientBuffer` RGBA32F main.cpp:397 */
  RTPT_PLANE_DEPTH = 5,     /* `depthImage`         f32 (D32F read as .r, D8) main.cpp:378 */
  RTPT_PLANE_VIS_ID = 6,    /* `visibilityBuffer`   u32 (reference: R16F, D9) main.cpp:371 */
  RTPT_PLANE_PREV_VIS_ID = 7, /* `previousVisibilityBuffer` u32 main.cpp:375 */
  RTPT_PLANE_LUT = 8,       /* `visibilityLUT`  (T+1) x rtpt_visibility_data main.cpp:390 */
  RTPT_PLANE_LUT_PREV = 9,  /* `visibilityLUTprevious` main.cpp:395 */
  RTPT_PLANE_PREV_PIXEL = 10, /* build-only observable: reprojected pixel (int32 x,y) written
                                 by the final filter pass; temporalFiltering.comp.glsl:238 */
  RTPT_PLANE_RAYCOUNT = 11, /* build-only: u64[1] closest-hit queries issued by rtpt_raytrace
                               since rtpt_reset_counters (SURVEY 8d "ray").  On the device it is kept as 256
                               partial sums (one counter serialised 32 400 atomics per 4K launch); rtpt_readback
                               adds them up, rtpt_plane_ptr returns the u64[256] array */
  RTPT_PLANE_HIT_ID = 12,   /* build-only observable (debug): u32 first-hit primitive id+1 of the
                               jittered primary ray of rtpt_raytrace, only if enabled */
  RTPT_PLANE_MOMENTS = 13,  /* extension RTPT_FLAG_EXT_VARIANCE: (m1, m2, history length, variance) float4 */
  RTPT_PLANE_VARIANCE = 14, /* extension: f32 variance written by the last filter iteration (or by the moments pass) */
  RTPT_PLANE_MOMENTS_PREV = 15, /* extension: the previous frame's moments (what this frame's accumulation reads) */
  RTPT_PLANE_ALBEDO = 16,   /* RTPT_FLAG_EXT_DEMODULATE: RGBA32F like IMAGE, (albedo of the first hit of this frame's jittered
                               primary ray, 0), (1, 1, 1, 0) where the path ended at its first query; written by rtpt_raytrace */
  RTPT_PLANE_SHADED = 17,   /* RTPT_FLAG_EXT_DEMODULATE: RGBA32F, (frame.rgb * ALBEDO.rgb, 0), written by rtpt_modulate.  Without
                               the flag neither plane is allocated: rtpt_plane_ptr returns NULL, rtpt_readback RTPT_E_INVALID */
  RTPT_PLANE_COUNT = 18
} rtpt_plane;

typedef struct rtpt_ctx rtpt_ctx;

/* ---- lifetime ------------------------------------------------------------------------- */

/* fills the reference's constants (citations on rtpt_config) for a width x height frame */
int rtpt_config_default(rtpt_config* cfg, uint32_t width, uint32_t height);

/* createBuffers (main.cpp:357-407) + createCommandPool/Context init: allocates every plane on
 * the device and one stream.  Returns RTPT_E_NO_GPU when no HIP device is present. */
int rtpt_create(const rtpt_config* cfg, rtpt_ctx** out);
/* freeRessources (main.cpp:1477-1528) */
int rtpt_destroy(rtpt_ctx* ctx);
/* The reference re-creates its size-dependent resources when the framebuffer changes
 * (framebufferResizeCallback main.cpp:275-278, swapChain.acquireAutoResize :1310).  Re-allocates every
 * per-pixel plane for a width x height frame storing rows [row_begin,row_end) (0,0 = the whole frame),
 * zeroes them and restarts the history (the next final pass is a frame-0 pass for the blend unless the
 * caller injects PREVIOUS); the uploaded scene, LUTs and configuration constants are kept.  Planes bound
 * with rtpt_bind_plane are dropped and must be bound again.  Blocks until the stream is idle. */
int rtpt_resize(rtpt_ctx* ctx, uint32_t width, uint32_t height, uint32_t row_begin, uint32_t row_end);
/* last error message of this thread's most recent failing call (ctx may be NULL) */
const char* rtpt_last_error(const rtpt_ctx* ctx);

/* run subsequent passes on a caller-owned hipStream_t (e.g. the stream RCCL halo exchanges are
 * ordered on).  NULL restores the context's own stream. */
int rtpt_set_stream(rtpt_ctx* ctx, void* hip_stream);

/* Bind caller-owned device memory as the storage of one colour/guide plane, like the reference
 * app owning every VkImage bound into the descriptor sets (createAndBindDescriptorSet,
 * main.cpp:744-908).  bytes must be >= rtpt_plane_bytes.  NULL returns to context-owned memory. */
int rtpt_bind_plane(rtpt_ctx* ctx, rtpt_plane which, void* device_ptr, size_t bytes);
/* current device pointer playing the role `which`.  Roles ROTATE among the three colour buffers — at the final filter
 * pass, when iterations run chained, and at rtpt_end_frame — so re-query after those calls; a buffer bound as IMAGE
 * does not stay IMAGE.  Alpha convention on the device: IMAGE after the last iteration of a frame and PREVIOUS after
 * rtpt_end_frame have alpha 0 like the reference's vec4(rgb, 0); between rtpt_raytrace and the last iteration the
 * colour planes carry the G-buffer depth in alpha ("rgbd"), and FILTERED is scratch whose alpha may hold it at any
 * time.  rtpt_readback always returns alpha 0. */
int rtpt_plane_ptr(rtpt_ctx* ctx, rtpt_plane which, void** device_ptr);
int rtpt_plane_bytes(const rtpt_ctx* ctx, rtpt_plane which, size_t* bytes);

/* Multi-GPU strips: the final filter pass fetches previousFrameImage at the REPROJECTED pixel
 * (temporalFiltering.comp.glsl:253), which under camera motion can lie in another rank's strip.
 * The host all-gathers the strips of the previous frame into one buffer covering frame rows
 * [row_begin,row_end) and registers it here; the final pass then reads history from it instead of
 * the context's own PREVIOUS plane.  NULL returns to the PREVIOUS plane. */
int rtpt_set_external_history(rtpt_ctx* ctx, const void* device_ptr, uint32_t row_begin, uint32_t row_end);

/* The same for the other two per-pixel planes of the previous frame that a strip reads at reprojected pixels: the id
 * plane (RTPT_FLAG_EXT_DISOCCLUSION, RTPT_FLAG_EXT_VARIANCE) and the moment plane (RTPT_FLAG_EXT_VARIANCE; may be NULL
 * otherwise).  Both buffers cover frame rows [row_begin,row_end), u32 and float4 per pixel.  NULL, NULL returns to the
 * context's own planes. */
int rtpt_set_external_guides(rtpt_ctx* ctx, const void* prev_vis, const void* moments_prev, uint32_t row_begin, uint32_t row_end);

/* Two frames in flight.  The reference serialises everything with vkQueueWaitIdle (main.cpp:110-111); the only
 * dependency between consecutive frames of this path is the final pass's history fetch, so a host may render
 * even frames in one context and odd frames in another (each on its own stream) and hand the finished frame
 * across: rtpt_stream_wait(ctx, other) makes everything submitted to `ctx` from now on start only after
 * everything submitted to `other` so far has finished (an event, no host block); the history itself is passed
 * with rtpt_set_external_history(ctx, <other's PREVIOUS plane>, ...).  Same device only. */
int rtpt_stream_wait(rtpt_ctx* ctx, rtpt_ctx* other);

/* ---- scene ---------------------------------------------------------------------------- */

/* loadMesh's RT arrays (main.cpp:416-428: objVertices tightly packed xyz, objIndices u32) +
 * buildAccelerationStructure (main.cpp:687-742: one BLAS, instances with 3x4 row-major
 * transforms; NULL/0 = the reference's single identity instance).  Builds the flattened
 * world-space triangle set, the BVH and sizes the LUTs.  Triangle id = instance*n_tris + t. */
int rtpt_scene_upload(rtpt_ctx* ctx, const float* xyz, uint32_t n_verts, const uint32_t* idx,
                      uint32_t n_tris, const float* instance_xforms, uint32_t n_instances);

/* Per-triangle materials (SURVEY.md 8(f) rank 4 — NOT reference behaviour: the reference keys its colours on the
 * normal, raytrace.comp.glsl:155-163, and ships no material library).  tri_material[t] indexes `materials` for
 * triangle t of the mesh given to rtpt_scene_upload (instances share them).  A hit then takes Kd as its albedo
 * instead of the normal-keyed colour (:244), and a surface with Ke != 0 ends the path like the analytic light does
 * (:226-234): throughput *= Ke.  NULL / 0 returns to the reference's colours; rtpt_scene_upload drops them. */
typedef struct rtpt_material {
  float albedo[3];   /* .mtl Kd */
  float emission[3]; /* .mtl Ke */
} rtpt_material;
int rtpt_scene_set_materials(rtpt_ctx* ctx, const uint32_t* tri_material, uint32_t n_tris, const rtpt_material* materials,
                             uint32_t n_materials);

/* Specular materials (NOT reference behaviour, off until this call; additive: RTPT_ABI_VERSION stays 5).  A
 * material is diffuse (flags 0: `albedo` and `emission` mean what they mean in rtpt_material, `specular` and `roughness` are
 * only checked), specular (RTPT_MAT_SPECULAR) or a dielectric (RTPT_MAT_DIELECTRIC, below), never a mixture; a specular
 * material has no Fresnel term and does not refract.  A hit on a specular
 * material takes `specular` (.mtl Ks) where a diffuse hit takes Kd — texel multiply, albedo plane, throughput multiply and
 * mip level apply to it unchanged — and leaves along d' = normalize(reflect(d, n) + roughness * s), s the point of the unit
 * sphere the diffuse bounce would add to the normal, from the same two draws (csrc/specular.hpp states the arithmetic;
 * roughness 0 is a perfect mirror).  A d' that does not leave the surface ends the path with colour 0 (absorbed); the last
 * segment of a path returns its throughput before any bounce, as for a diffuse hit.
 * The call replaces whatever material set the scene has, and rtpt_scene_set_materials replaces a set given here; NULL / 0
 * drops the set.  Lifetime and synchronisation are rtpt_scene_set_materials': dropped by rtpt_scene_upload, kept by
 * rtpt_scene_set_instances, rtpt_scene_rebuild, a changed model and rtpt_resize; no plane tag changes, so frame reuse and
 * reprojection reuse go on.  Device memory held: 32 bytes per triangle, as after rtpt_scene_set_materials.
 * RTPT_E_INVALID, the scene and its set untouched: another n_tris than the uploaded mesh's, an index >= n_materials, an
 * unknown flag, a component of any material that is not finite, a specular material with a roughness outside [0, 1] or with
 * a non-zero emission.  The kernels that know the specular bounce run exactly when some TRIANGLE's material is specular.
 * Known limitation: the filter's guides (normal, depth, id, world position, reprojection) are the mirror's own, so a
 * reflected image is blurred over the filter's reach and reprojected with the mirror's surface.
 *
 * Dielectrics (RTPT_MAT_DIELECTRIC; additive as well): a perfectly smooth interface between the outside (index 1) and a medium
 * of index `ior` >= 1, whose triangles' normals point out of the medium.  A hit takes `specular` as its colour exactly as a
 * specular hit does, takes the segment's two draws, and is reflected with the probability of Schlick's Fresnel term F = R0 +
 * (1 - R0)(1 - cos)^5 — R0 = ((ior - 1) / (ior + 1))^2, the cosine taken on the rarer side — exactly when its first draw is
 * below F or the angle is beyond the critical one; otherwise it is refracted by Snell's law and goes on from the far side of
 * the surface (csrc/dielectric.hpp states the arithmetic).  Never absorbed; the second draw is unused.  The word after `flags`
 * carries `ior` when the flag is set and is ignored without it (the struct keeps its size and layout; `_pad` still names the
 * word).  RTPT_E_INVALID as above, too, for: both flags on one material; a dielectric with a roughness other than 0, with a
 * non-zero emission, or with an ior that is not finite or is < 1.  The kernels that know the interface run exactly when some
 * TRIANGLE's material is a dielectric.  Known limitation: the filter's guides are the pane's own, so what is seen through glass
 * is blurred and reprojected with the pane, as in a mirror. */
#define RTPT_MAT_SPECULAR 0x1u
#define RTPT_MAT_DIELECTRIC 0x2u
typedef struct rtpt_material_ext {
  float albedo[3];   /* .mtl Kd */
  float emission[3]; /* .mtl Ke */
  float specular[3]; /* .mtl Ks: the colour of a specular or dielectric hit */
  float roughness;   /* [0, 1] when specular; 0: mirror.  0 when dielectric */
  uint32_t flags;    /* RTPT_MAT_* */
  union {
    uint32_t _pad; /* without RTPT_MAT_DIELECTRIC: ignored */
    float ior;     /* with it: the index of refraction, finite and >= 1 (.mtl Ni) */
  };
} rtpt_material_ext;
int rtpt_scene_set_materials_ext(rtpt_ctx* ctx, const uint32_t* tri_material, uint32_t n_tris, const rtpt_material_ext* materials,
                                 uint32_t n_materials);

/* Albedo textures (NOT reference behaviour, off until this call): the albedo of a hit becomes (Kd, or the
 * normal-keyed colour without materials) x texel.rgb — one binary32 multiply per channel, taken before the throughput
 * multiply — at EVERY segment of a path, in every kernel that shades (csrc/texture.hpp is the one sampler).  A surface with
 * Ke != 0 ends the path before any texture is read, as without textures.  With RTPT_FLAG_EXT_DEMODULATE, RTPT_PLANE_ALBEDO
 * holds that product for the first hit.
 * tri_uv: 6 floats per triangle of the uploaded MESH (u0 v0 u1 v1 u2 v2, corner order of idx); tri_texture[t]: 0 =
 * untextured, i + 1 = textures[i]; instances share both (triangle id reads record id % n_tris).  texels: RGBA32F, linear,
 * row-major, row 0 is v in [0, 1/height); texture i owns texels [first_texel, first_texel + width * height); alpha is
 * carried and ignored.  Coordinates repeat (s = u - floor(u)); the filter is bilinear unless RTPT_TEX_NEAREST is set; no
 * mip-mapping unless RTPT_TEX_MIPMAP is set (below).  Everything is copied: the arrays may die at return.
 * Device memory held, counted by rtpt_debug_live_device_bytes: exactly 32 * n_tris + 16 * n_textures + 16 * n_texels bytes
 * when no texture has a mip flag.
 * Mip-mapping, opt-in per texture (RTPT_TEX_MIPMAP): level l of a W x H texture is max(1, W >> l) x max(1, H >> l) texels and
 * there are floor(log2(max(W, H))) + 1 levels (rtpt_util_texture_chain).  Texel (x, y) of level l + 1 is the binary32 value
 * ((a + b) + (c + d)) * 0.25f of the texels (2x, 2y), (min(2x + 1, w - 1), 2y) and the same columns of row min(2y + 1, h - 1)
 * of level l, all four channels: an odd last column or row is dropped, except where the level is one texel wide or high.
 * The library builds the levels on the device from `texels`, which holds level 0 only, as without the flag; with
 * RTPT_TEX_MIPS_GIVEN the caller supplies them: level l follows level l - 1 directly, from first_texel on, and the rectangle
 * checked against n_texels is the whole chain.  A hit reads level lambda = 0.5 * plog2(rho^2), clamped to [0, levels - 1]:
 * rho^2 = w^2 D / (n.d)^2, w the ray's footprint width at the hit (segment 0: t * 2 * fov_slope / height, the full frame's;
 * every later segment: t * 1/8, t that segment's length alone), D = |twice the triangle's area in level-0 texels| / |twice
 * its posed world area|, plog2 the piecewise-linear log2 (exponent + mantissa fraction: exact at powers of two, at most
 * 0.0861 from log2 elsewhere); a degenerate triangle reads level 0.  Bilinear textures blend the bilinear samples of levels
 * floor(lambda) and floor(lambda) + 1 (a level of weight 0 is not read); RTPT_TEX_NEAREST reads the nearest texel of level
 * floor(lambda + 0.5).  csrc/texture.hpp states the arithmetic.  Known bias: a bounce reads pre-filtered albedo, so the
 * converged image of a mip-mapped scene differs slightly from the un-mipped one (the mean of a product of albedos along a
 * path is not the product of their means); first hits that magnify the texture are unchanged.
 * With a mip flag on any texture the device holds exactly
 *   32 * n_tris + 16 * n_textures + 16 * n_texels + 16 * G + 80 * n_textures bytes,
 * G = the texels of levels 1.. of every texture with RTPT_TEX_MIPMAP and without RTPT_TEX_MIPS_GIVEN (the generated levels),
 * 80 bytes per texture the table of level offsets.
 * Lifetime, like the materials': rtpt_scene_upload drops the textures; rtpt_scene_set_materials, rtpt_scene_set_instances,
 * rtpt_scene_rebuild, a changed ubo->model and rtpt_resize keep them.  tri_uv, tri_texture, textures or texels NULL, or
 * n_textures / n_texels 0, drops them (every kernel is then the one of a scene that never had any).
 * Launches what is recorded first and blocks until the stream is idle, like rtpt_scene_set_materials.  K0, K1 and the filter
 * read no texture: frame reuse and reprojection reuse go on across the call.
 * RTPT_E_NO_SCENE before an upload.  RTPT_E_INVALID, with the scene and its textures untouched, for: n_tris other than the
 * uploaded mesh's; tri_texture[t] > n_textures; a zero width or height, or one above 65536; a rectangle that ends beyond
 * n_texels (or beyond 2^32 - 1 texels; the whole chain with RTPT_TEX_MIPS_GIVEN); generated levels that take the atlas
 * beyond 2^32 - 1 texels; an unknown flag (0x2, 0x4, 0x8 among them); RTPT_TEX_MIPS_GIVEN without RTPT_TEX_MIPMAP; a uv
 * that is not finite (or above 2^64 in magnitude).  No kernel can index outside the atlas: that is decided here, on the host. */
#define RTPT_TEX_NEAREST 0x1u     /* default: bilinear */
#define RTPT_TEX_MIPMAP 0x10u     /* sampled from a mip chain, the level chosen from the ray's footprint */
#define RTPT_TEX_MIPS_GIVEN 0x20u /* only with RTPT_TEX_MIPMAP: `texels` holds the whole chain of this texture */
typedef struct rtpt_texture {
  uint32_t width, height, first_texel, flags;
} rtpt_texture;
int rtpt_scene_set_textures(rtpt_ctx* ctx, const float* tri_uv, const uint32_t* tri_texture, uint32_t n_tris,
                            const rtpt_texture* textures, uint32_t n_textures, const float* texels, size_t n_texels);

/* Smooth shading: interpolated vertex normals (NOT reference behaviour, off until this call; additive:
 * RTPT_ABI_VERSION stays 5).  tri_normals: n_tris x 9 floats, the corners' normals of triangle t of the mesh given to
 * rtpt_scene_upload, in the mesh's own space and in that call's corner order (instance i, triangle t reads record t; the kernels
 * carry them through model x instance transform with the pose's cofactor matrix, mirrors included).  tri_smooth: n_tris words, 0 =
 * the triangle keeps its geometric normal; NULL = all smooth.  Normals need not be unit length and may hold anything, NaN and zero
 * included: a hit whose interpolated normal does not normalise to finite numbers shades with the geometric normal
 * (csrc/shading_normal.hpp states the rules: which normal each step of a bounce uses, and the side tests that keep rays off the
 * wrong side of the real surface).  The diffuse, specular and dielectric bounces and the light samples use the interpolated
 * normal; the offset origin, the normal-keyed colours, the texture footprint, K0, K1 and the LUT keep the triangle's, and so
 * does the filter unless the context has RTPT_FLAG_EXT_SMOOTH_GUIDE, which feeds interpolated normals to its edge stop.  A scene
 * that holds normals is traced through its BVH, as under RTPT_FLAG_FORCE_BVH, however small it is.
 * tri_normals == NULL with n_tris == 0 removes them; rtpt_scene_upload drops them with the materials; moved instances, a changed
 * ubo.model, rtpt_scene_rebuild and rtpt_resize keep them.  RTPT_E_NO_SCENE before an upload.  RTPT_E_INVALID, with the scene
 * untouched, for: n_tris other than the uploaded mesh's; tri_normals == NULL with n_tris != 0; a context created with
 * RTPT_FLAG_NO_PATH_COMPACTION (that A/B form of the tracing kernels has no smooth instantiation). */
int rtpt_scene_set_normals(rtpt_ctx* ctx, const float* tri_normals, const uint32_t* tri_smooth, uint32_t n_tris);

/* The environment map: a path that meets nothing reads an HDR image where the reference has its fixed sky (NOT reference
 * behaviour, off until this call; additive: RTPT_ABI_VERSION stays 5).  texels_rgba: n x n RGBA32F texels of an
 * OCTAHEDRAL map, row-major (alpha is carried and ignored); rotation: the 3 x 3 matrix, row-major, that takes a world direction into
 * the map's frame (NULL = identity); scale: one factor per colour channel (NULL = 1, 1, 1).  flags: RTPT_TEX_NEAREST or 0
 * (bilinear).  The lookup of a direction d, in binary32 with the contract's operations only (csrc/env.hpp states it for the device,
 * bit for bit):
 *   E1  e = (dot(r0, d), dot(r1, d), dot(r2, d)), r0, r1, r2 the rows of the rotation, dot(a, b) = fma(a.z, b.z, fma(a.y, b.y,
 *       a.x * b.x)); always computed (without a rotation the identity is stored).
 *   E2  s = (|e.x| + |e.y|) + |e.z|.  If !(s > 0) or s is infinite the colour is (0, 0, 0) and no texel is read: a NaN, the zero
 *       direction, an infinite or overflowing component.
 *   E3  p = e.x / s, q = e.z / s, correctly rounded.  The upper sheet is e.y >= 0.0f.
 *   E4  upper sheet: (u, v) = (p, q); lower sheet: u = copysign(1 - |q|, p), v = copysign(1 - |p|, q).
 *   E5  U = fma(u, 0.5, 0.5), V = fma(v, 0.5, 0.5); row 0 holds V in [0, 1/n), column 0 U in [0, 1/n).  Bilinear: x = U * n - 0.5,
 *       x0 = floor(x), f = x - x0, taps clamp(x0, 0, n - 1) and clamp(x0 + 1, 0, n - 1), likewise in V; the four texels combine as
 *       the albedo textures' do, a + f * (b - a) along x for both rows, then along y.  RTPT_TEX_NEAREST: the texel (min(n - 1,
 *       int(floor(U * n))), the same of V).  Addressing is CLAMPED, not repeated: the square's edges are the folds of the lower
 *       hemisphere, and the clamp costs half a texel of error along those four lines (a known limit).
 *   E6  colour = texel.rgb * scale.rgb, one multiply per channel.
 * What does not change: the analytic sphere light is tested first; a path that ends in the environment at its first segment
 * stores ALBEDO (1, 1, 1) under RTPT_FLAG_EXT_DEMODULATE; no path changes direction, length or random stream, so HIT_ID and
 * RAYCOUNT of a frame are those of the same frame without an environment.  The environment is collected by paths that miss, not
 * sampled by next-event estimation: a small bright sun is noisy.
 * The call acts on the CONTEXT, not on the scene, and needs none: the map survives rtpt_scene_upload, every rtpt_scene_set_*,
 * rtpt_scene_rebuild, moved instances and rtpt_resize.  texels_rgba == NULL or n == 0 drops it, and every launch is again the one of
 * a context that never had one, bit for bit.  Everything is copied; the call flushes what is recorded and blocks until the stream
 * is idle, like rtpt_scene_set_textures.  K0, K1 and the filter read nothing of it: frame reuse and reprojection reuse go on across
 * the call.  Device memory held, counted by rtpt_debug_live_device_bytes: exactly 16 * n * n bytes.
 * A launch with an environment has the limits of a launch that samples lights (RTPT_FLAG_EXT_NEE): every segment runs in the tile
 * kernel, there are no queue kernels and no deferred final filter pass rides in the tracing launch.  The tile kernels that read an
 * environment exist for every scene mode, DEMOD, textures with and without mips, every material and light-sampling mode, with and
 * without vertex normals, fused with K0 + K1 and unfused — and not for RTPT_FLAG_NO_PATH_COMPACTION: a context created with that
 * A/B flag refuses the call.
 * RTPT_E_INVALID, with the previous environment untouched, for: n above 4096; a flag other than RTPT_TEX_NEAREST; a texel, a
 * rotation entry or a scale that is not finite; a context with RTPT_FLAG_NO_PATH_COMPACTION.  No kernel can index outside the
 * map: that is decided here, on the host. */
int rtpt_set_environment(rtpt_ctx* ctx, const float* texels_rgba, uint32_t n, uint32_t flags, const float rotation[9], const float scale[3]);
/* A lat-long (equirectangular) image, width x height RGB32F pixels with row 0 at +y, to the n x n octahedral map above; runs on the
 * host in double.  For the centre of each texel it inverts E5, E4 and E3 and normalises; the column fraction of that direction is
 * atan2(d.x, -d.z) / (2 pi) + 0.5 (the image's centre is the camera's forward, -z), the row fraction acos(d.y) / pi; it takes ONE
 * bilinear sample there (x = fraction * size - 0.5; wrapped horizontally, clamped vertically) and rounds to binary32; alpha is 1.
 * Known limit: one sample per texel, no prefiltering when n is much smaller than the image.  RTPT_E_INVALID for a NULL pointer,
 * an image of no pixels or beyond 65536 in either dimension, n == 0 or n above 4096.  Needs no context and no device. */
int rtpt_util_environment_from_latlong(const float* rgb, uint32_t width, uint32_t height, uint32_t n, float* texels_rgba_out);
/* env::color (csrc/env.hpp, the rules above) of the context's environment on n directions of 3 floats, on the device: rgb_out = n x
 * 3 floats.  Directions are not checked: rule E2 is what meets a hostile one.  RTPT_E_INVALID without an environment. */
int rtpt_selftest_environment(rtpt_ctx* ctx, const float* dirs, size_t n, float* rgb_out);

/* What built the tree that is on the device now.  (A struct tag without a typedef: the entry point below carries the
 * same name, and C keeps tags and functions apart.) */
enum { RTPT_BVH_BUILDER_HOST_SAH = 0, RTPT_BVH_BUILDER_DEVICE_LBVH = 1 };
enum { RTPT_BVH_FALLBACK_NONE = 0, RTPT_BVH_FALLBACK_DEPTH = 1 };
enum { RTPT_BUILDER_DEVICE_SAH = 2 }; /* a third value of `builder`: RTPT_FLAG_DEVICE_BVH_SAH built the tree */
struct rtpt_scene_build_info {
  uint32_t builder, fallback; /* RTPT_BVH_BUILDER_* or RTPT_BUILDER_DEVICE_SAH, and why it is not the one asked for: RTPT_BVH_FALLBACK_* */
  uint32_t n_primitives;      /* what the tree was built over: fan pairs (leaf_pairs) or triangles */
  uint32_t n_nodes, depth;    /* child-pair nodes; level of the deepest leaf (the root pair's children are at 1) */
  uint32_t leaf_pairs;        /* 1: every leaf is one fan pair (2q, 2q + 1) */
  float build_ms;             /* tree construction alone.  Device: HIP events around the builder's kernels, the refit that
                                 fills the boxes and the leaf records (includes the one small readback in between).
                                 Host: the clock around the SAH build and the node packing */
  float upload_ms;            /* the whole rtpt_scene_upload / rtpt_scene_rebuild call, host clock */
};
/* RTPT_E_NO_SCENE before an upload.  After a device build it waits for that build's events. */
int rtpt_scene_build_info(rtpt_ctx* ctx, struct rtpt_scene_build_info* out);
/* With RTPT_FLAG_DEVICE_BVH_BUILD, rtpt_scene_upload keeps flattening the mesh and detecting fan pairs on the host
 * (RTPT_FLAG_DEVICE_FLATTEN moves both to the device too), uploads the triangles and builds the tree on the device, with one small readback (depth, node count, nodes per height) where the
 * host path has its final synchronisation.  A radix tree over 63 key bits and 32 tie-breaking bits can be deeper than
 * the traversal's 48-entry stack (nearly coincident geometry at very different scales): the upload then builds
 * with the host builder in the same call, returns RTPT_OK and reports HOST_SAH / FALLBACK_DEPTH.
 *
 * rtpt_scene_rebuild builds a NEW tree on the device over the triangles as currently posed (a refit keeps the topology
 * of the pose the tree was built for, however far the model has moved since) and replaces nodes, leaf order and leaf
 * records; un-posed triangles, model, LUTs, materials and history stay.  Allowed on any scene whatever built its tree
 * (afterwards it is a device tree, whatever the flag says); RTPT_E_NO_SCENE without one.  Frames after it equal the
 * frames without it bit for bit: it changes cost only.  Blocks for the readback.  If the new tree would be deeper than
 * the stack the old one stays and the call returns RTPT_E_INVALID. */
int rtpt_scene_rebuild(rtpt_ctx* ctx);

/* Replace ALL instance transforms of the uploaded mesh (n_instances x 12 floats, 3x4 row-major, as rtpt_scene_upload takes
 * them): instances move between frames without a new upload.  Call it between rtpt_end_frame and the next rtpt_gbuffer.
 * n_instances must equal the upload's count (a scene uploaded without transforms has count 1); triangle ids, LUT sizes,
 * materials, the model matrix and the history stay.  The next rtpt_gbuffer rebuilds the LUT, LUT_PREV keeps the previous
 * frame's pose (what K1 and the reprojection read), and frame reuse does not serve that frame.
 * Cost: scenes that are refit on the device (every BVH scene unless RTPT_HOST_REFIT=1, and every device-built tree — the
 * scenes whose changed ubo->model costs +0.27 ms) copy 48 bytes per instance and run flatten -> pose (current model) ->
 * refit -> leaf records on the context's stream, without a host synchronisation; the first call on a scene that was not
 * uploaded with RTPT_FLAG_DEVICE_FLATTEN also copies the mesh to the device, once.  Other scenes (brute force,
 * RTPT_HOST_REFIT=1) are flattened again on the host and take the host path of a changed model (blocks).
 * A refit keeps the TOPOLOGY of the pose the tree was built for: pixels stay exact however far the instances move (boxes
 * only cull and order), tracing gets slower as boxes of unrelated instances start to overlap.  After large moves the
 * caller may call rtpt_scene_rebuild.  Fan pairs stay fan pairs (both triangles share the vertices, the transform and
 * the arithmetic); transforms that would separate a pair straddling two instances (odd triangle count, coincident
 * instances) are refused.
 * RTPT_E_NO_SCENE before an upload, RTPT_E_INVALID for NULL arguments or another count; a failed call leaves the scene
 * untouched. */
int rtpt_scene_set_instances(rtpt_ctx* ctx, const float* instance_xforms, uint32_t n_instances);

/* How the last rtpt_scene_upload / rtpt_scene_set_instances moved the geometry, so that a test can tell the device path
 * from a host path that computes the same pixels.
 * out: [0] host-to-device bytes of geometry (mesh, transforms, triangles; not the tree) copied by that call,
 * [1] 1 if the triangles the scene now stands on were flattened on the device by that call, [2] 1 if its fan-pair decision
 * was taken on the device, [3] rtpt_scene_set_instances calls served without a host synchronisation since rtpt_create. */
int rtpt_debug_upload_info(rtpt_ctx* ctx, uint64_t out[4]);

/* Device memory the library holds right now, in bytes, over all contexts of the process: every buffer a context owns
 * (planes, scene, tree, tables, builder scratch, traversal spill area), counted where it is allocated and where it is
 * freed.  Not counted: pinned host staging, events and streams, and planes bound with rtpt_bind_plane (the caller's).
 * After rtpt_destroy of every context it is 0; a test compares readings instead of the device-wide hipMemGetInfo. */
int rtpt_debug_live_device_bytes(uint64_t* out);

/* The per-pixel normal plane of the filter's edge stop: stored rows x width cells of four floats (n.xyz, self weight), what K0
 * writes for scenes without an id-pair table (more than 63 triangles) and while RTPT_FLAG_EXT_SMOOTH_GUIDE is active.  Additive:
 * RTPT_ABI_VERSION stays 5.
 * rtpt_debug_guide_normals: blocking readback into out (bytes >= stored rows x width x 16).  RTPT_E_INVALID when the context has no
 * such plane; it works without the flag too.
 * rtpt_debug_set_guide_normals: blocking upload.  The plane then counts as written for all stored rows of the current frame, as if
 * K0 had, until the next K0 writes it; it is allocated if needed.  Only while RTPT_FLAG_EXT_SMOOTH_GUIDE is active or the scene has
 * no id-pair table (RTPT_E_INVALID otherwise: no filter kernel would read it). */
int rtpt_debug_guide_normals(rtpt_ctx* ctx, float* out, size_t bytes);
int rtpt_debug_set_guide_normals(rtpt_ctx* ctx, const float* src, size_t bytes);

/* Frame reuse.  K0 and K1 (rtpt_gbuffer, rtpt_temporal_gradient) read the camera, the light, the posed scene and the LUTs
 * and nothing that changes from frame to frame by itself: no frame number, no random stream.  While all of those rest,
 * both passes would store the bytes their planes already hold, so the context launches neither and rtpt_raytrace runs
 * the tracing kernel alone; every plane, the ray count and the finished frame equal those of a context that runs them.
 * The id plane rotates at rtpt_end_frame, so the third consecutive frame with equal inputs is the first one served.
 * A plane's content counts as known only while the passes are its only writer: rtpt_set_plane, rtpt_plane_ptr (the
 * caller can write through the pointer: write before the next rtpt_gbuffer, or ask again), rtpt_bind_plane,
 * rtpt_resize, rtpt_set_stream with another stream and rtpt_enable_debug with another mask make the next frame compute
 * it again, and a plane bound with rtpt_bind_plane is never reused.
 * RTPT_NO_FRAME_REUSE=1 in the environment of rtpt_create turns all of it off.
 * out: [0] frames whose K0 + K1 were not launched, [1] and [2] reserved and always 0 (the cached reprojection of the final
 * pass has counters of its own, rtpt_debug_reproj_info), [3] plane tags invalidated. */
int rtpt_debug_reuse_info(rtpt_ctx* ctx, uint64_t out[4]);

/* Reprojection reuse.  The pixel the final filter pass reprojects to is a function of the world-position plane, the id
 * plane, LUT_PREV, projPrev * viewPrev and the frame size.  Frame reuse already knows when the first three hold the bytes
 * of the frame before, so while they and the matrix rest the pass would compute the integers it computed a frame ago.  A
 * final pass whose inputs equal those of the previous frame's final pass therefore also stores the pair, packed to 4 bytes
 * per pixel (y << 16 | x, one sentinel for every pixel outside the frame, whose history reads 0 either way), and later
 * final passes with the same inputs load it instead of reading the world position, gathering the LUT and reprojecting.
 * The plane (4 bytes per stored pixel) is allocated at the first store; a camera that moves every frame never stores.
 * Only the single-launch final pass of the LDS-staged kernel takes part (id-pair table or per-pixel normals, 1 <= k <= 16,
 * frame at most 65535 x 65535); the direct kernel, the extension modes and a chain ending in the final pass reproject as
 * before.  Everything that makes frame reuse compute a frame again (see above) also drops the stored pairs, as does any
 * write to a LUT through rtpt_set_plane or a pointer from rtpt_plane_ptr; with RTPT_DEBUG_PREV_PIXEL enabled nothing is
 * stored or loaded (that plane wants the raw integers).  Every plane, the ray count and the finished frame equal those
 * of a context that reprojects every frame.  RTPT_NO_REPROJ_REUSE=1 in the environment of rtpt_create turns it off;
 * RTPT_NO_FRAME_REUSE=1 does too.
 * out: [0] final passes that stored, [1] final passes that loaded, [2] invalidations of the stored pairs, [3] bytes of
 * the plane (0 until the first store). */
int rtpt_debug_reproj_info(rtpt_ctx* ctx, uint64_t out[4]);

/* The deferred final pass.  On a frame at rest the tracing launch is bound by instruction issue and touches next to no
 * memory, the final filter pass by memory bandwidth, and as launches of their own they never run together.  The final pass
 * of frame n and rtpt_raytrace of frame n + 1 read and write disjoint planes, so a final pass that qualifies is prepared
 * where it is recorded and launched inside the next rtpt_raytrace's launch, as workgroups in front of and behind the
 * tracing tiles.  It qualifies when it is the frame's last recorded iteration, a single launch of the LDS-staged id-pair
 * kernel that loads its reprojected pixels (see above), with k <= 5, no extension flag, no RTPT_DEBUG_PREV_PIXEL, no
 * rtpt_present_target and no bound or external plane in the context.  rtpt_raytrace takes it when it runs the brute-force
 * tile kernel alone (K0 and K1 reused or not recorded) with one sample per pixel over all stored rows, without
 * demodulation, textures or specular materials; it then traces into a fourth colour buffer, allocated at the first such
 * call (16 bytes per stored pixel), because the pass still reads the buffer IMAGE named.  Every other entry point that
 * launches, exposes or changes a plane, a stream, the scene or the context launches the pass first, by itself, and what it
 * returns or leaves is what it would have been; rtpt_gbuffer, rtpt_temporal_gradient and rtpt_end_frame in their usual
 * order do not.  A pointer obtained from rtpt_plane_ptr, or one bound or registered as an external plane, is therefore
 * complete only after a call that flushes: ask rtpt_plane_ptr again (or call rtpt_sync) after rtpt_end_frame before
 * reading it on the device.  Every plane, the ray count and the finished frame equal those of a context that launches
 * the pass where it is recorded.  RTPT_NO_FINAL_DEFER=1 in the environment of rtpt_create turns it off;
 * RTPT_FINAL_FRONT=<workgroups per CU, or from 8 on workgroups in all>[,<percent of the pass's work>] sets how much of the
 * pass runs in front of the tiles (built in: one workgroup per CU; all of the pass on a frame as large as 4K, 75 % on a small one).
 * out: [0] passes recorded instead of launched, [1] of those launched inside a tracing launch, [2] launched alone,
 * [3] bytes of the fourth colour buffer (0 until the first such launch). */
int rtpt_debug_defer_info(rtpt_ctx* ctx, uint64_t out[4]);

/* Empty tile columns (additive: RTPT_ABI_VERSION stays 5).  rtpt_raytrace dispatches its 64 x 4 tiles column by column from
 * the middle of the frame outwards, and for a scene of at most 64 triangles it has every triangle's padded screen bounds.  In a
 * launch that carries a deferred final pass (above), the columns at the end of that order which no triangle's bounds reach within
 * the traced rows are not one workgroup per tile: a workgroup takes a run of R vertically consecutive tiles of one column and
 * traces their primary rays only, which end on the light or in the sky.  A column without triangles in front of a reached one
 * stays a column of tiles.  Every plane and the ray count equal those of a context without runs.  RTPT_EMPTY_RUN=<R> in the
 * environment of rtpt_create sets R; 0 turns the runs off.
 * out, for the last rtpt_raytrace launch: [0] tile columns served one workgroup per tile (every column of a launch without
 * runs), [1] run workgroups, [2] tiles served in runs, [3] R. */
int rtpt_debug_empty_run_info(rtpt_ctx* ctx, uint64_t out[4]);

/* ---- per-frame passes, one call per reference dispatch ----------------------------------- */

/* drawVisbilityBuffer (main.cpp:1187-1199; visibility.{vert,geom,frag}.glsl): id, world
 * position, NDC depth planes + LUT for all triangles.  Rows [y0,y1) of the frame (clamped to
 * the stored rows); y0=y1=0 means all stored rows.
 * ubo->model poses the scene (visibility.vert.glsl:24; recomputed per frame at main.cpp:1469, the identity there):
 * when it differs from the last call's, every triangle is re-posed (model * v, the LUT's arithmetic), the BVH is
 * refit and the tables are rebuilt before the pass runs, and rtpt_raytrace traces the posed scene too.  It must be
 * affine and invertible.  LUT_PREV keeps the previous frame's pose, which is what K1 and the reprojection read.
 * Cost of a changed model: BVH scenes (more than 64 triangles, or RTPT_FLAG_FORCE_BVH) are re-posed and refit ON THE
 * DEVICE, on the context's stream, without a host synchronisation (csrc/refit.hip: +0.27 ms for 1,152,000 triangles);
 * small brute-force scenes are re-posed on the host (microseconds) and the call then waits for the stream once. */
int rtpt_gbuffer(rtpt_ctx* ctx, const rtpt_ubo* ubo, uint32_t y0, uint32_t y1);
/* computeTemporalGradient (main.cpp:1201-1220; temporalGradient.comp.glsl:104-172).  Called right behind rtpt_gbuffer
 * (the reference's order, main.cpp:1105-1106) for rows that call covered, the two run as ONE launch: rtpt_gbuffer records
 * its dispatch, and every entry point other than this one launches it first, alone.  Since ABI version 4 the pair stays
 * recorded until rtpt_raytrace (below). */
int rtpt_temporal_gradient(rtpt_ctx* ctx, const rtpt_push_constants* pc, uint32_t y0, uint32_t y1);
/* drawSceneToImage (main.cpp:1222-1253; raytrace.comp.glsl:273-344).  Called right behind rtpt_gbuffer +
 * rtpt_temporal_gradient (main.cpp:1105-1107) whose rows contain [y0, y1), the three run as ONE launch (the G-buffer's
 * workgroups are dispatched behind the tracing ones and fill the trace's tail): any other entry point in between launches the
 * recorded passes first, so the planes always hold what the separate dispatches leave there.  RTPT_FLAG_NO_FILTER_FUSION (or
 * RTPT_NO_TRACE_FUSION=1 in rtpt_create's environment) keeps the launches apart. */
int rtpt_raytrace(rtpt_ctx* ctx, const rtpt_push_constants* pc, uint32_t y0, uint32_t y1);
/* one iteration of applyTemporalFiltering's loop body (main.cpp:1259-1305;
 * temporalFiltering.comp.glsl:191-265).  The host loops k = 1..maxWaveletIteration exactly
 * like main.cpp:1259.  Odd k reads IMAGE and writes FILTERED, even k the reverse
 * (main.cpp:1264-1281).  On k == max (odd) the fused reprojection + blend result becomes
 * IMAGE (D1: taps read the pre-pass snapshot).  ubo supplies viewPrev/projPrev and may be
 * NULL when k < max.
 * The calls of a frame are RECORDED, like the reference records its dispatches into command buffers
 * (main.cpp:1284-1303), and launched when the call with k == max arrives: consecutive iterations then run as one
 * chained kernel whose intermediate image stays in LDS instead of travelling through `filteredImageBuffer` / `image`
 * (same arithmetic per pixel, same bits).  Every other entry point that reads or changes a plane, a stream or the
 * frame state first launches what is recorded, one kernel per iteration, so between iterations each plane holds what
 * the separate dispatches leave there.  After the LAST iteration IMAGE holds the frame; FILTERED is scratch (the
 * reference's own last store to it, temporalFiltering.comp.glsl:152, is dead).  RTPT_FLAG_NO_FILTER_FUSION turns the
 * recording off.  An error of a recorded launch is reported by the call that triggers it. */
int rtpt_temporal_filter(rtpt_ctx* ctx, const rtpt_push_constants* pc, const rtpt_ubo* ubo,
                         uint32_t y0, uint32_t y1);
/* history hand-over of copyImageToSwapChainsCurrentImage (main.cpp:1364-1372):
 * previousImage <- image, previousVisibilityBuffer <- visibilityBuffer, LUTprev <- LUT,
 * done by rotating plane roles (no copy kernels). */
int rtpt_end_frame(rtpt_ctx* ctx);

/* the swapchain blit of copyImageToSwapChainsCurrentImage (main.cpp:1338-1361: `image`, RGBA32F, blitted to the acquired
 * swapchain image, VK_FORMAT_B8G8R8A8_UNORM): frame rows [y0,y1) of the finished frame (call after rtpt_end_frame, or
 * after the last rtpt_temporal_filter) are converted — clamp to [0,1], x*255 + 0.5 truncated, NaN -> 0; bytes B,G,R,A in
 * memory — and written to `dst_device`, a device buffer whose first byte is pixel (0, y0): 4*W bytes per row.  The
 * buffer is the caller's "swapchain image"; with several ranks each rank converts its own rows and the presenting rank
 * gathers them (4 B/px on the wire instead of 16).  Runs on the context's stream. */
int rtpt_present(rtpt_ctx* ctx, void* dst_device, uint32_t y0, uint32_t y1);
/* With RTPT_FLAG_EXT_DEMODULATE the blit multiplies on the fly: every channel of frame.rgb * ALBEDO.rgb is rounded to binary32
 * and then converted by the rule above, alpha 0 — the bytes are the conversion of RTPT_PLANE_SHADED, which is neither read nor
 * needed (36 B/px).  The final filter pass never fuses its swapchain store under the flag (it would store demodulated colour):
 * rtpt_present_target stays callable and rtpt_present does the work. */
/* Optional, before the frame's rtpt_temporal_filter calls: name the swapchain rows of this frame in advance.  The final
 * filter pass then writes them in swapchain format as it stores the frame (one launch and one 16 B/px read less), and the
 * later rtpt_present of the same rows and image returns at once; where the final pass runs in a kernel that cannot fuse
 * the store (extension modes, direct-load variants), rtpt_present does the work as before — the calling sequence is the
 * same either way.  The registration stays until changed; dst_device == NULL clears it. */
int rtpt_present_target(rtpt_ctx* ctx, void* dst_device, uint32_t y0, uint32_t y1);

/* RTPT_FLAG_EXT_DEMODULATE (RTPT_E_INVALID without it): multiply the albedo back.  SHADED.rgb = frame.rgb * ALBEDO.rgb for frame
 * rows [y0,y1) (the row conventions of the passes; 0,0 = all stored rows), one binary32 multiply per channel, alpha 0.  `frame`
 * is IMAGE until rtpt_end_frame and PREVIOUS after it, like rtpt_present.  Call it after the frame's last rtpt_temporal_filter
 * or after rtpt_end_frame, before the context's next rtpt_raytrace overwrites ALBEDO.  Per pixel: no halo, no guide, so a strip
 * context modulates the rows it owns.  Launches what is recorded first, like every entry point; runs on the context's stream. */
int rtpt_modulate(rtpt_ctx* ctx, uint32_t y0, uint32_t y1);

/* ---- synchronisation / data movement ---------------------------------------------------- */
int rtpt_sync(rtpt_ctx* ctx);
/* blocking copy of a whole plane (stored rows) to host memory */
int rtpt_readback(rtpt_ctx* ctx, rtpt_plane which, void* dst, size_t bytes);
/* blocking upload of a whole plane from host memory (inject fixtures / history; SURVEY 5
 * "checkpoint/resume": the only cross-frame state is PREVIOUS, PREV_VIS_ID, LUT_PREV) */
int rtpt_set_plane(rtpt_ctx* ctx, rtpt_plane which, const void* src, size_t bytes);
int rtpt_reset_counters(rtpt_ctx* ctx);
/* only closest-hit queries of pixels in frame rows [y0,y1) are added to RAYCOUNT (default: all
 * stored rows).  Strip ranks that trace halo rows redundantly set this to their owned rows so the
 * sum over ranks equals the single-GPU count. */
int rtpt_set_count_rows(rtpt_ctx* ctx, uint32_t y0, uint32_t y1);
/* enable build-only observables (off by default: they cost extra stores per pixel) */
#define RTPT_DEBUG_HIT_ID 0x1u     /* RTPT_PLANE_HIT_ID written by rtpt_raytrace */
#define RTPT_DEBUG_PREV_PIXEL 0x2u /* RTPT_PLANE_PREV_PIXEL written by the final filter pass */
int rtpt_enable_debug(rtpt_ctx* ctx, uint32_t mask);

/* per-kernel timing hooks for bench.py: HIP events recorded on the stream the kernel runs on.
 * rtpt_timing_enable(n), n >= 1, makes the passes of every n-th frame (frames are counted by
 * rtpt_end_frame) record a start/stop event pair — the pairs cost ~6 % of a 1 ms frame when every
 * launch is bracketed, so long runs sample; 0 turns it off.  rtpt_timing_collect blocks, sums the
 * durations per kernel since the last collect and returns them. */
typedef enum rtpt_kernel_id {
  RTPT_K_GBUFFER = 0,
  RTPT_K_LUT = 1,
  RTPT_K_GRADIENT = 2,
  RTPT_K_PATHTRACE = 3,
  RTPT_K_ATROUS = 4,
  RTPT_K_ATROUS_FINAL = 5,
  RTPT_K_ATROUS_CHAIN = 6,       /* several consecutive iterations k < N in one launch (intermediates in LDS) */
  RTPT_K_ATROUS_CHAIN_FINAL = 7, /* ... ending in the final pass */
  RTPT_K_GBUFFER_GRADIENT = 8,   /* K0 and K1 in one launch (rtpt_temporal_gradient right behind rtpt_gbuffer) */
  RTPT_K_PRESENT = 9,            /* rtpt_present: RGBA32F -> B8G8R8A8_UNORM */
  RTPT_K_GBUFFER_PATHTRACE = 10, /* K0, K1 and K2 in one launch (rtpt_raytrace right behind rtpt_gbuffer + rtpt_temporal_gradient,
                                    the reference's own order, main.cpp:1105-1107): ABI version 4 */
  RTPT_K_MODULATE = 11,          /* rtpt_modulate: SHADED = frame x ALBEDO (RTPT_FLAG_EXT_DEMODULATE) */
  RTPT_K_COUNT = 12
} rtpt_kernel_id;
int rtpt_timing_enable(rtpt_ctx* ctx, int enable);
int rtpt_timing_collect(rtpt_ctx* ctx, double ms_sum[RTPT_K_COUNT], uint32_t launches[RTPT_K_COUNT]);
const char* rtpt_kernel_name(rtpt_kernel_id k);

/* device-side evaluation of the deterministic math used on bit-exact paths, for parity tests
 * against the oracle: op 0 log, 1 sin(2*pi*u), 2 cos(2*pi*u), 3 sqrt, 4 1/x, 5 exp (filter
 * fast path), 6 pcg step float.  in/out are host arrays of n floats (u32 bits for op 6). */
int rtpt_selftest_math(rtpt_ctx* ctx, int op, const float* in, float* out, size_t n);
/* the product's correctly-rounded sqrt (op 3) and reciprocal (op 4) are shorter instruction sequences than the compiler's
 * IEEE expansions (csrc/rtpt_math.hpp): this runs ALL 2^32 binary32 patterns through both on the device and returns how
 * many results differ in any bit (the contract is 0) and the first few offending patterns.  ~0.1 s. */
int rtpt_selftest_exhaustive(rtpt_ctx* ctx, int op, uint64_t* mismatches, uint32_t first_bad[4]);
/* the product's division (csrc/rtpt_math.hpp, exact::div_) against the compiler's IEEE division, on the device.  mode 0:
 * passes [first_pass, first_pass + n_passes) of the 256-pass enumeration of ALL 2^23 x 2^23 pairs of binary32 significands
 * (~0.15 s per pass; all 256 is the proof that the short sequence is correctly rounded for operands of ordinary magnitude);
 * mode 1: n_passes x 2^33 operand pairs of arbitrary bits, pass numbers seeding the generator (range test + long path).
 * mode 2: mode 1's operand pairs through exact::quotient_positive(a, b) against a / b > 0.0f (the contract is 0 here too).
 * mode 3: mode 1's operand pairs and a third draw through exact::div2_(a0, a1, b) against a0 / b and a1 / b (either quotient
 * counts as one mismatch; first_bad = the offending numerator and b).
 * *mismatches = results that differ in any bit (two NaNs count as equal); first_bad = the bits of one offending (a, b). */
int rtpt_selftest_div(rtpt_ctx* ctx, int mode, uint32_t first_pass, uint32_t n_passes, uint64_t* mismatches, uint32_t first_bad[2]);
/* One function of the numerics contract per call, evaluated on the device item by item (one thread each) by the very
 * functions the frame kernels call (csrc/rtpt_math.hpp, device_common.hpp, shade_segment.hpp), for comparison with the oracle's
 * oracle_contract_array operand by operand.  in = n items of `in` words, out = n items of `out` words, host arrays of raw
 * 32-bit patterns: floats as their bits (NaN payloads and signed zeros pass unchanged), integers as they are.
 *   fn                          in -> out   words
 *    0 dot                       6 -> 1     a, b
 *    1 cross                     6 -> 3     a, b
 *    2 length                    3 -> 1
 *    3 normalize                 3 -> 3
 *    4 powi                      2 -> 1     x, n (int)
 *    5 f2i                       1 -> 1     out: int
 *    6 glsl_min, glsl_max        2 -> 2     x, y -> min, max
 *    7 rng_seed                  4 -> 1     px, py, frame, batch (uint)
 *    8 rng_next, rng_skip        1 -> 3     state -> state after rng_next, its float, state after rng_skip
 *    9 sincos2pi                 1 -> 2     u in [0, 1] (the contract's domain) -> sin, cos
 *   10 log_                      1 -> 1     x > 0, finite
 *   11 exact::exp_               1 -> 1
 *   12 mat_row_point            19 -> 4     M[16] column-major, p -> rows 0..3
 *   13 div_                      2 -> 1     a, b
 *   14 div2_                     3 -> 2     a0, a1, b -> a0 / b, a1 / b
 *   15 tri_area                  9 -> 1     a, b, c
 *   16 bary_coords              12 -> 3     p, a, b, c
 *   17 bary_coords_at           13 -> 3     p, a, b, c, area
 *   18 bary_mix                 12 -> 3     bc, a, b, c
 *   19 reproject_pixel          36 -> 2     W, H (int), PVprev[16], id (0..3), wp, the id's three lut_prev cells (float4 each),
 *                                           x, y (int) -> previous pixel x, y (int)
 *   20 ray_hits_light           10 -> 1     o, d, c, radius (r2 = radius * radius as rtpt_raytrace forms it) -> 0 / 1
 *   21 sky_color                 3 -> 3     d
 *   22 hit_barycentrics          3 -> 6     u (HitRec::u, negated), v, ad -> b0, b1, b2 of <true>, then of <false>
 * Operands outside a stated domain are not refused; what the functions do with them is not part of the contract. */
int rtpt_selftest_contract(rtpt_ctx* ctx, int fn, const uint32_t* in, uint32_t* out, size_t n);
/* closest-hit of arbitrary rays through the product's traversal (parity vs the oracle's brute
 * force): rays = n x {ox,oy,oz,dx,dy,dz}; out_id[n] = primitive id+1 or 0; out_t[n] may be NULL */
int rtpt_selftest_trace(rtpt_ctx* ctx, const float* rays, size_t n, uint32_t* out_id, float* out_t);

/* device-side evaluation of the sampler for arbitrary uv (parity with the tests' numpy restatement): rgba_out[4 i .. 4 i + 3]
 * = what a hit with texture coordinates (uv[2 i], uv[2 i + 1]) reads from textures[texture] (0-based) of the last
 * rtpt_scene_set_textures, alpha included.  RTPT_E_NO_SCENE without a scene; RTPT_E_INVALID without textures, for an index
 * >= n_textures or a uv that is not finite. */
int rtpt_selftest_texture(rtpt_ctx* ctx, uint32_t texture, const float* uv, size_t n, float* rgba_out);
/* device-side evaluation of the specular bounce (csrc/specular.hpp: faceforward, the sphere point of the two draws, the lobe),
 * one case per thread, by the function the tracing kernels call: in = n x 9 floats (d[3], n[3], u1, u2, g), out = n x 4
 * floats (d'[3], 1.0f if absorbed else 0.0f).  Operands are not checked: d and n are meant to be unit vectors, u1, u2 in
 * [0, 1], g in [0, 1]. */
int rtpt_selftest_bounce(rtpt_ctx* ctx, const float* in, float* out, size_t n);
/* the same for the dielectric interface (csrc/dielectric.hpp: the side, Snell's law, Schlick's term, the choice, the direction):
 * in = n x 9 floats (d[3], n[3], u1, u2, ior), out = n x 5 floats (d'[3], 1.0f if transmitted else 0.0f, F).  Operands are not
 * checked: d and n are meant to be unit vectors, u1, u2 in [0, 1], ior >= 1; 1 / ior and R0 are computed as the host computes
 * them for the record. */
int rtpt_selftest_refract(rtpt_ctx* ctx, const float* in, float* out, size_t n);
/* Next-event estimation (RTPT_FLAG_EXT_NEE; additive: RTPT_ABI_VERSION stays 5).  The light sample (csrc/light_sample.hpp: the pick, the point, the direction, the weight), one
 * case per thread: in = n x 19 words (v0[3], v1[3], v2[3] of the light, x[3] the bounce origin, nf[3] the faced normal, u_l,
 * u_a, u_b as floats, L as a uint32), out = n x 9 words (y[3], wd[3], g, 1.0f if valid else 0.0f as floats, the picked entry
 * min(uint(u_l * L), L - 1) as a uint32).  The light's unit normal is computed as for its shade record.  Operands are not
 * checked; L is meant to be in [1, 2^24]. */
int rtpt_selftest_light_sample(rtpt_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n);
/* The sphere sample of RTPT_FLAG_EXT_NEE_SPHERE (csrc/light_sample.hpp: sphere_sample), one case per thread: in = n x 12 words
 * (x[3] the bounce origin, nf[3] the faced normal, c[3] the light's centre, r2 its squared radius, u_c, u_p as floats), out = n x
 * 6 words (wd[3], g, 1.0f if taken else 0.0f, 1.0f if valid else 0.0f as floats; wd and g are written as 0 where the sample is
 * not taken).  Operands are not checked.  Additive: RTPT_ABI_VERSION stays 5. */
int rtpt_selftest_sphere_sample(rtpt_ctx* ctx, const uint32_t* in, uint32_t* out, size_t n);
/* The cumulative table of RTPT_FLAG_EXT_NEE_POWER (csrc/light_table.hip) from n given weights, 1 <= n <= 2^24: the maximum, the
 * quantisation and the scan as the context's builder runs them; cdf_out = n x uint64.  Needs neither a scene nor the flag.
 * Additive: RTPT_ABI_VERSION stays 5. */
int rtpt_selftest_light_table(rtpt_ctx* ctx, const float* w, size_t n, uint64_t* cdf_out);
/* The weighted pick (csrc/light_sample.hpp: pick_power) of k draws u_l on the table cdf[0, n), 1 <= n <= 2^24: index_out[j] the
 * entry, inv_p_out[j] = float(S) / float(q).  Operands are not checked beyond n; every index the search reads lies in [0, n). */
int rtpt_selftest_light_pick(rtpt_ctx* ctx, const uint64_t* cdf, size_t n, const float* u_l, size_t k, uint32_t* index_out, float* inv_p_out);
/* The weights of RTPT_FLAG_EXT_NEE_MIS (csrc/light_sample.hpp: hit_weight, mis_bounce, mis_light), one case per thread, by the
 * functions the tracing kernels call: in = n x 20 words (v0[3], v1[3], v2[3] of the hit emitter, o[3] and d[3] of the ray that hit
 * it, the hit's b1, b2, cb, inv_p as floats; word 19 is not read), out = n x 3 floats (g_hit, wb(g_hit), g_hit * m(g_hit)).  The
 * emitter's unit normal is computed as for its shade record, b0 = 1 - b1 - b2.  Operands are not checked.  Additive:
 * RTPT_ABI_VERSION stays 5. */
int rtpt_selftest_mis_weight(rtpt_ctx* ctx, const float* in, float* out, size_t n);
/* The rules of smooth shading (csrc/shading_normal.hpp: rules 1 to 7 and the three side tests), one case per thread, by the
 * functions the tracing kernels call: in = n x 36 words (n0[3], n1[3], n2[3] the corners' normals, the hit's b1, b2, the three rows
 * of the pose's cofactor matrix [9], ng[3] the faced geometric normal, d[3] the incoming direction, d'[3] a new direction, wd[3] a
 * light sample's direction, ray_offset; words 33 to 35 are not read), out = n x 8 floats (1.0f if the hit is smooth else 0.0f,
 * ns[3] — ng where it is not —, 1.0f if d' is absorbed, 1.0f if wd stays valid, the dielectric's signed offset for d', 0).
 * b0 = 1 - b1 - b2.  Operands are not checked.  Additive: RTPT_ABI_VERSION stays 5. */
int rtpt_selftest_shading_normal(rtpt_ctx* ctx, const float* in, float* out, size_t n);
/* The search of RTPT_FLAG_EXT_NEE_MIS (csrc/light_list_host.hpp: find) of k queries on the ascending list ids[0, n), n <= 2^24:
 * index_out[j] = the index of queries[j] in the list, n for an id that is not in it.  ids is not checked beyond n; every index the
 * search reads lies in [0, n). */
int rtpt_selftest_light_find(rtpt_ctx* ctx, const uint32_t* ids, size_t n, const uint32_t* queries, size_t k, uint32_t* index_out);
/* The light list of RTPT_FLAG_EXT_NEE as it stands on the device: *n = its entries (0 without the flag, without materials or
 * without an emitter), of which the first min(*n, cap) are copied to ids — id + 1 of every posed triangle inst * n_tris + t whose
 * material has Ke != 0, ascending.  ids may be NULL when cap is 0 (count only). */
int rtpt_debug_light_list(rtpt_ctx* ctx, uint32_t* ids, uint32_t cap, uint32_t* n);
/* The cumulative table of RTPT_FLAG_EXT_NEE_POWER as it stands on the device, in the manner of rtpt_debug_light_list: *n = its
 * entries (0 without both bits, without materials or without an emitter), of which the first min(*n, cap) are copied to cdf.
 * cdf may be NULL when cap is 0 (count only). */
int rtpt_debug_light_table(rtpt_ctx* ctx, uint64_t* cdf, uint32_t cap, uint32_t* n);
/* The same at an explicit level: lod[i] is the lambda a hit would have computed (any bit pattern: it is clamped to
 * [0, levels - 1], a NaN reads level 0).  A texture without RTPT_TEX_MIPMAP has one level.  rtpt_selftest_texture keeps
 * reading level 0.  Refusals as rtpt_selftest_texture (lod is not checked). */
int rtpt_selftest_texture_lod(rtpt_ctx* ctx, uint32_t texture, const float* uv, const float* lod, size_t n, float* rgba_out);
/* Level selection of the tracing kernels: traces n rays (6 floats each, as rtpt_selftest_trace) through the product's
 * traversal and returns out_id[i] = hit id + 1 (0: miss) and out_lod[i] = the lambda shade_segment would sample the hit's
 * texture at — computed by the device function the tracing kernels call.  bounce == 0: the rule of segment 0 with the
 * context's frame height and fov_slope; bounce == 1: the rule of every later segment.  Misses, untextured hits, textures
 * without RTPT_TEX_MIPMAP and scenes without textures return 0. */
int rtpt_selftest_texture_footprint(rtpt_ctx* ctx, const float* rays, size_t n, uint32_t bounce, uint32_t* out_id, float* out_lod);

/* ---- host-side helpers shared by the C++ and Python hosts -------------------------------- */
/* glm::lookAt / glm::perspective as used at main.cpp:482-484,:1470-1472 (right-handed,
 * zero-to-one depth — D6; the caller applies proj[1][1] *= -1 like the reference does). */
void rtpt_util_look_at(const float eye[3], const float center[3], const float up[3], float out[16]);
void rtpt_util_perspective(float fovy, float aspect, float z_near, float z_far, float out[16]);
/* minimal OBJ reader standing in for tinyobjloader at main.cpp:416-428: `v` and `f` records,
 * polygons fan-triangulated (0,1,2),(0,2,3) in file order (D5).  Two-call pattern: pass NULL
 * arrays to obtain counts. */
int rtpt_util_load_obj(const char* path, float* xyz, uint32_t* n_verts, uint32_t* idx, uint32_t* n_tris);
/* the material side of the same file: `mtllib` (looked up next to the OBJ), `usemtl`, and Kd / Ke of every `newmtl`.
 * tri_material lines up with rtpt_util_load_obj's triangles; material 0 is the default (Kd 0.7, Ke 0).  Two-call
 * pattern (NULL arrays: counts; *n_materials in = capacity).  A missing library is not an error — the reference's own
 * OBJ names one that does not exist (scenes/CornellBox-Original-Merged.obj:3) — *n_materials comes back 0. */
int rtpt_util_load_obj_materials(const char* path, uint32_t* tri_material, uint32_t* n_tris, rtpt_material* materials,
                                 uint32_t* n_materials);
/* The same reader, contract and numbering, plus Ks, Ns and illum of every `newmtl`.  The rule is a definition:
 *   specular[] = Ks (0 without a Ks line); roughness = min(1, sqrt(2 / (Ns + 2))) in binary32 (1 where that is no number in
 *   [0, 1]), 0 without an Ns line; flags = RTPT_MAT_SPECULAR exactly when illum >= 3, Ks != 0 and Ke == 0 (an emitter ends
 *   the path either way and stays diffuse); anything else stays diffuse.  albedo, emission and tri_material are what
 *   rtpt_util_load_obj_materials returns for the same file. */
int rtpt_util_load_obj_materials_ext(const char* path, uint32_t* tri_material, uint32_t* n_tris, rtpt_material_ext* materials,
                                     uint32_t* n_materials);
/* rtpt_util_load_obj_materials_ext plus Ni and Tf.  A material is a dielectric instead of what the rule above makes it exactly
 * when illum is 4, 6, 7 or 9, it has an `Ni` line with a finite value >= 1, Ke == 0 and its colour is not 0, the colour being Tf
 * where a complete `Tf r g b` line exists and Ks otherwise: then specular[] = colour, ior = Ni, roughness = 0 and flags =
 * RTPT_MAT_DIELECTRIC.  Every other material is what rtpt_util_load_obj_materials_ext returns for it, `_pad` 0 included. */
int rtpt_util_load_obj_materials_ni(const char* path, uint32_t* tri_material, uint32_t* n_tris, rtpt_material_ext* materials,
                                    uint32_t* n_materials);
/* the texture-coordinate side of the same file: `vt` records and the vt of `f v/vt`, `f v/vt/vn` corners (`f v`, `f v//vn`:
 * the corner gets (0, 0)); negative vt indices count back from the last `vt` read.  tri_uv: 6 floats per triangle (u0 v0 u1
 * v1 u2 v2), fanned like rtpt_util_load_obj's triangles, so the two arrays line up.  Two-call pattern (NULL: count). */
int rtpt_util_load_obj_texcoords(const char* path, float* tri_uv, uint32_t* n_tris);
/* the vertex-normal side of the same file, for rtpt_scene_set_normals: `vn` records and the vn of `f v//vn`, `f v/vt/vn` corners;
 * negative vn indices count back from the last `vn` read.  tri_normals: 9 floats per triangle (the three corners' normals),
 * tri_smooth: one word per triangle, both fanned like rtpt_util_load_obj's triangles, so the arrays line up.  A face with a
 * corner that has no vn, or whose vn index is 0 or out of range, gives triangles with tri_smooth 0 and normals (0, 0, 0); every
 * other triangle has tri_smooth 1.  Two-call pattern (tri_normals == NULL: count; tri_smooth may be NULL). */
int rtpt_util_load_obj_normals(const char* path, float* tri_normals, uint32_t* tri_smooth, uint32_t* n_tris);
/* the `map_Kd` file name of every material, in rtpt_util_load_obj_materials' numbering (entry 0, the default material, is
 * always empty; no map: empty): *n_materials NUL-terminated strings, one after the other, in `names`.  Options before the
 * name are not supported (the last word of the line is taken).  Two-call pattern: names == NULL stores the byte count in
 * *names_bytes and the count in *n_materials; with names, *names_bytes in = capacity.  *n_materials comes back 0 when the
 * OBJ names no readable library. */
int rtpt_util_load_obj_map_kd(const char* path, char* names, size_t* names_bytes, uint32_t* n_materials);
/* The mip chain of a width x height texture (RTPT_TEX_MIPMAP): *n_levels = floor(log2(max(width, height))) + 1, *n_texels =
 * the sum over the levels of max(1, width >> l) * max(1, height >> l) — what RTPT_TEX_MIPS_GIVEN expects from first_texel
 * on.  Either pointer may be NULL.  Needs no GPU.  RTPT_E_INVALID for a zero dimension or one above 65536. */
int rtpt_util_texture_chain(uint32_t width, uint32_t height, uint32_t* n_levels, uint64_t* n_texels);
/* Host-only self check of the acceleration-structure builder that stands in for the driver's BLAS/TLAS build
 * (buildAccelerationStructure, main.cpp:687-742): builds the BVH over `n_tris` world-space triangles (9 floats
 * each), packs the device nodes and verifies the invariants the traversal relies on.  Needs no GPU.
 *   stats[0] nodes, [1] leaves, [2] max depth, [3] largest leaf,
 *   [4] triangles not referenced exactly once, [5] boxes that do not contain their subtree,
 *   [6] device (16-bit grid) boxes that do not contain the binary32 box, [7] dangling child references */
int rtpt_util_bvh_check(const float* tris, uint32_t n_tris, uint64_t stats[8]);
/* rtpt_util_bvh_check with the builder's mode chosen: pairs != 0 builds over the fan pairs (2q, 2q + 1) as
 * rtpt_scene_upload does for a scene made of them (n_tris must be even) and then also counts in stats[7] every leaf
 * that is not exactly one such pair from an even slot (cnt 2, leaf_order[first] even, leaf_order[first + 1] the next id):
 * the pairs-mode traversal reads one pair record per leaf.  pairs == 0 is rtpt_util_bvh_check. */
int rtpt_util_bvh_check_pairs(const float* tris, uint32_t n_tris, int pairs, uint64_t stats[8]);
/* The structure as it stands ON THE DEVICE of a context — after rtpt_scene_upload, or after a changed ubo->model re-posed
 * the scene and refit the tree inside rtpt_gbuffer (on the device, on the context's stream, without a host
 * synchronisation: refit.hip) — read back and checked on the host (blocks).
 *   stats[0] nodes, [1] leaves, [2] deepest level, [3] largest leaf, [4] triangles not referenced exactly once,
 *   [5] decoded device boxes that do not contain every vertex below them, [6] boxes reaching beyond the padded scene,
 *   [7] dangling child references, and when the tree was built over fan pairs, leaves that are not one pair (as
 *   rtpt_util_bvh_check_pairs) */
int rtpt_debug_bvh_check(rtpt_ctx* ctx, uint64_t stats[8]);
/* The TOPOLOGY of that structure, read back (blocks): child_refs[2 i], child_refs[2 i + 1] = the left and right child
 * reference of node i in node order (bit 31 set: leaf, (first slot << 2) | (count - 1); clear: node index; 0xFFFFFFFF: absent),
 * leaf_order[slot] = triangle id.  Two calls like the loaders: with both arrays NULL it stores the counts (nodes, leaf
 * slots = triangles); with arrays, *n_nodes and *n_leaf_ids say how many entries they hold (2 x *n_nodes references) and
 * must be at least the counts.  Two trees are the same tree exactly when these arrays are equal, whatever built them.
 * RTPT_E_NO_SCENE before an upload, RTPT_E_INVALID on a NULL context or count pointer or a short array. */
int rtpt_debug_bvh_topology(rtpt_ctx* ctx, uint32_t* child_refs, uint32_t* n_nodes, uint32_t* leaf_order, uint32_t* n_leaf_ids);
/* the same invariants after a REFIT: the tree is built over `built_for` and refit to `moved` (the same n_tris
 * triangles after an animated model matrix, rtpt_gbuffer) — topology and leaf order kept, boxes recomputed */
int rtpt_util_bvh_refit_check(const float* built_for, const float* moved, uint32_t n_tris, uint64_t stats[8]);

#ifdef __cplusplus
}
static_assert(sizeof(rtpt_push_constants) == 112, "PushConstants is 112 bytes (main.cpp:35-49)");
static_assert(offsetof(rtpt_push_constants, cameraPos) == 16, "cameraPos@16");
static_assert(offsetof(rtpt_push_constants, lightPos) == 32, "lightPos@32");
static_assert(offsetof(rtpt_push_constants, lightPosPrev) == 48, "lightPosPrev@48");
static_assert(offsetof(rtpt_push_constants, currentCameraColor) == 64, "currentCameraColor@64");
static_assert(offsetof(rtpt_push_constants, previousCameraColor) == 80, "previousCameraColor@80");
static_assert(offsetof(rtpt_push_constants, waveletIteration) == 92, "waveletIteration@92");
static_assert(offsetof(rtpt_push_constants, maxWaveletIteration) == 96, "maxWaveletIteration@96");
static_assert(sizeof(rtpt_ubo) == 384, "UniformBufferObject is 384 bytes (main.cpp:82-90)");
static_assert(sizeof(rtpt_visibility_data) == 48, "VisibilityData stride 48 (std430)");
static_assert(sizeof(struct rtpt_scene_build_info) == 32, "rtpt_scene_build_info is 32 bytes");
static_assert(sizeof(rtpt_texture) == 16, "rtpt_texture is 16 bytes");
#endif

#endif /* RTPT_H */
