"""Specular materials on the device (rtpt_scene_set_materials_ext, csrc/specular.hpp), in the order of what each check can
catch: the bounce function against its numpy restatement, diffuse scenes that must not move, the closed form of a room of
mirrors, the reflected direction end to end, schedule independence where paths are absorbed at different segments, absorption
itself, demodulation / textures / lifetime / refusals, and the two hosts.

No oracle frame is involved here: every expectation is a closed form, a float64 restatement, the numpy float32 restatement of
tests/specular_scenes.py, or another schedule of the same frame.  The oracle's statement of the specular bounce
(oracle_raytrace_ext) is compared frame by frame in tests/test_shading_ext_gpu.py."""
import gc
import json
import os
import subprocess

import numpy as np
import pytest

import filter_planes as FP
import pathtrace_scenes as P
import specular_scenes as S
import test_demodulate_gpu as D
import test_pathtrace_scenes_gpu as T
import texture_scenes as TS
from conftest import bits
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
W0, H0 = P.MAIN_SHAPE
NO_COMPACTION, SINGLE_LAUNCH, NO_FUSION, FORCE_BVH, DEMODULATE = 0x8, 0x200, 0x400, 0x2, 0x8000
FORM_IDS = list(P.FORMS)


# ------------------------------------------------------------------------------------------ one frame
def upload(abi, ctx, scene, specular=None):
    ctx.scene_upload(*FP.mesh_of(scene.tris))
    ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, specular))


def frame(abi, oracle, ctx, scene, W, H, planes=()):
    out = T.frame_on_gpu(abi, oracle, ctx, scene, W, H)
    for p in planes:
        out[p] = ctx.readback(getattr(abi, "PLANE_" + p))
    return out


def context(abi, scene, W, H, segments, flags=0, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def same_frame(got, want, tag, keys=("HIT_ID", "IMAGE")):
    for k in keys:
        same_bits(got[k], want[k], tag + (k,))
    assert got["rays"] == want["rays"], tag + ("rays", got["rays"], want["rays"])


# ------------------------------------------------------------------------------------------ 1. the function
def test_bounce_equals_the_restatement(hip_lib, oracle):
    """rtpt_selftest_bounce, one case per lane, against specular_scenes.bounce32 bit for bit: d' and the absorbed flag, on the
    CPU test's hostile operands and 4 096 seeded ones"""
    abi = hip_lib
    cases = np.concatenate([S.hostile_cases(), S.seeded_cases()])
    with abi.Context(abi.config_default(64, 48)) as ctx:
        got = ctx.selftest_bounce(cases)
    want = S.bounce32(oracle, cases)
    same_bits(got[:, :3], want[:, :3], ("bounce", "d'"))
    same_bits(got[:, 3], want[:, 3], ("bounce", "absorbed"))
    assert 0 < (got[:, 3] != 0).sum() < len(got)


# ------------------------------------------------------------------------------------------ 2. nothing moves for diffuse scenes
DIFFUSE_SCENES = [(n, f) for n, f in P.MAIN_SCENES if P.scene(n, f).materials is not None]


@pytest.mark.parametrize("name,form", DIFFUSE_SCENES, ids=[f"{n}-{f}" for n, f in DIFFUSE_SCENES])
def test_diffuse_scenes_do_not_move(hip_lib, oracle, name, form):
    """the table of rtpt_scene_set_materials through rtpt_scene_set_materials_ext with flags 0; with one more material that is
    specular and assigned to no triangle (the diffuse kernels are chosen); with it assigned to two triangles no path reaches
    (the kernels that know the specular bounce compute diffuse hits): IMAGE, HIT_ID and the ray count of the six K2 variants"""
    abi = hip_lib
    scene = P.scene(name, form)
    far, far_mat = S.with_far_pair(scene)
    extra = np.concatenate([scene.materials, F32([[0.5, 0.5, 0.5, 0, 0, 0]])])
    for vid, vflags, seg in D.variants():
        tag = (name, form, vid)
        with context(abi, scene, W0, H0, seg, vflags) as ctx:
            ctx.scene_upload(*FP.mesh_of(scene.tris))
            ctx.set_materials(scene.tri_material, scene.materials)
            want = frame(abi, oracle, ctx, scene, W0, H0)
            ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials))
            same_frame(frame(abi, oracle, ctx, scene, W0, H0), want, tag + ("flags 0",))
            ctx.set_materials_ext(scene.tri_material, abi.materials_ext(extra, {len(extra) - 1: ((0.9, 0.8, 0.7), 0.3)}))
            same_frame(frame(abi, oracle, ctx, scene, W0, H0), want, tag + ("unassigned",))
        with context(abi, far, W0, H0, seg, vflags) as ctx:
            ctx.scene_upload(*FP.mesh_of(far.tris))
            ctx.set_materials(far.tri_material, far.materials)
            want_far = frame(abi, oracle, ctx, far, W0, H0)
            ctx.set_materials_ext(far.tri_material, abi.materials_ext(far.materials, {far_mat: ((0.9, 0.8, 0.7), 0.3)}))
            same_frame(frame(abi, oracle, ctx, far, W0, H0), want_far, tag + ("unreached",))
        assert not (want_far["HIT_ID"] > len(scene.tris)).any(), "no primary ray sees the far pair"
        if name.startswith("closed_room") or name in ("mask_room", "soup"):      # closed: the far pair changes no path at all
            same_bits(want_far["IMAGE"], want["IMAGE"], tag + ("the far pair is outside",))


# ------------------------------------------------------------------------------------------ 3. closed form
def _const_half_texture(n_tris):
    desc, texels = TS.atlas([TS.constant_image(3, 5, (0.5, 0.5, 0.5))])
    return TS.random_uv(n_tris, 5), np.ones(n_tris, np.uint32), desc, texels


@pytest.mark.parametrize("form", P.FORMS, ids=FORM_IDS)
def test_room_of_mirrors_closed_form(hip_lib, oracle, form):
    """every wall a mirror with Ks = (1/2, 1/4, 1/8): reflections in an axis-aligned box only flip signs of the primary
    direction, so no ray points at the far light and n . d' = -n . d > 0: nothing is absorbed, every path lives n segments and
    every pixel is exactly (2^-n, 2^-2n, 2^-3n); n W H rays.  Also with three samples per pixel, demodulated (IMAGE x ALBEDO is the
    value, ALBEDO is Ks) and with a constant texture of 1/2 (one more exact factor per hit)"""
    abi = hip_lib
    scene, spec = S.mirror_room(form)
    for n in (1, 4, 9, 17):
        value = F32([2.0 ** -n, 2.0 ** -(2 * n), 2.0 ** -(3 * n)])
        for what, flags, spp, textured in (("plain", 0, 1, False), ("spp 3", 0, 3, False), ("demodulated", DEMODULATE, 1, False),
                                           ("textured", 0, 1, True)):
            tag = ("mirrors", form, n, what)
            with context(abi, scene, W0, H0, n, flags, spp) as ctx:
                upload(abi, ctx, scene, spec)
                if textured:
                    ctx.set_textures(*_const_half_texture(len(scene.tris)))
                got = frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",) if flags else ())
            assert (got["HIT_ID"] > 0).all(), tag
            assert got["rays"] == n * W0 * H0 * spp, tag + (got["rays"],)
            rgb = got["IMAGE"][..., :3]
            if flags:
                same_bits(got["ALBEDO"][..., :3], np.broadcast_to(F32(S.MIRROR_KS), rgb.shape), tag + ("ALBEDO",))
                rgb = (rgb * got["ALBEDO"][..., :3]).astype(F32)
            want = value * F32([2.0 ** -n] * 3) if textured else value
            same_bits(rgb, np.broadcast_to(want.astype(F32), rgb.shape), tag + ("IMAGE",))


# ------------------------------------------------------------------------------------------ 4. the direction, end to end
@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
def test_mirror_quad_shows_the_sky_of_the_reflected_ray(hip_lib, oracle, vflags):
    """a mirror quad (g = 0, Ks = (1, 1/2, 1/4)) tilted back by 30 degrees under the sky, pixel_jitter 0, two segments, the light
    straight below: every pixel HIT_ID shows on the quad is Ks x sky(reflect(d)) of the float64 pixel-centre ray, within 2^-16
    absolute (the bar of test_textures_gpu's uv interpolation test for the same kind of chain).
    Measured on an MI355X, brute force and forced BVH alike: 64 x 48 (1688 pixels on the quad) max abs error 1.587e-07, 70 x 10
    (80 pixels) 1.263e-07; the bar is 1.526e-05."""
    abi = hip_lib
    scene, spec = S.mirror_quad()
    for W, H in S.SIZES:
        with context(abi, scene, W, H, 2, vflags) as ctx:
            upload(abi, ctx, scene, spec)
            got = frame(abi, oracle, ctx, scene, W, H)
        on, want = S.mirror_quad_expectation(W, H)
        hit = got["HIT_ID"] > 0
        assert np.array_equal(hit, on), "the numpy ray and K2 agree on the pixels that hit the quad"
        assert on.mean() > 0.1 and (~on).any()
        err = np.abs(got["IMAGE"][..., :3][on].astype(np.float64) - want[on])
        print(f"mirror quad {W} x {H} flags {vflags:#x}: {on.sum()} pixels on the quad, max abs error {err.max():.3e} (bar {2.0 ** -16:.3e})")
        assert err.max() <= 2.0 ** -16
        span = want[on].max(0) - want[on].min(0)
        assert span[0] > 0.02, "the frame sees a stretch of the sky's gradient"
        assert got["rays"] == W * H + on.sum()


# ------------------------------------------------------------------------------------------ 5. schedule independence
SCHEDULE_SCENES = [("mixed_room", "small"), ("mixed_room", "pairs"), ("glossy_trench", "small"), ("glossy_trench", "odd")]
SCHEDULES = (("default", 0), ("no_compaction", NO_COMPACTION), ("single_launch", SINGLE_LAUNCH), ("no_fusion", NO_FUSION), ("force_bvh", FORCE_BVH))


def _scene(name, form):
    return {"mixed_room": S.mixed_room, "glossy_trench": S.glossy_trench, "mirror_room": S.mirror_room}[name](form)


@pytest.mark.parametrize("segments", [9, 33])
@pytest.mark.parametrize("name,form", SCHEDULE_SCENES, ids=[f"{n}-{f}" for n, f in SCHEDULE_SCENES])
def test_schedules_agree(hip_lib, oracle, name, form, segments):
    """diffuse and specular surfaces side by side: paths are absorbed, and end, at different segments.  9 and 33 segments cross
    the windows 4 / 8 / 16.  Every flag, and a strip context against the full frame's rows: IMAGE and the ray count bit for bit"""
    abi = hip_lib
    scene, spec = _scene(name, form)
    out = {}
    for sid, flags in SCHEDULES:
        with context(abi, scene, W0, H0, segments, flags) as ctx:
            upload(abi, ctx, scene, spec)
            out[sid] = frame(abi, oracle, ctx, scene, W0, H0)
            if sid == "default":
                _, _, y0, y1 = P.STRIP
                ctx.set_count_rows(y0, y1)
                counted = frame(abi, oracle, ctx, scene, W0, H0)["rays"]
    for sid, _ in SCHEDULES[1:]:
        same_frame(out[sid], out["default"], (name, form, segments, sid))
    with context(abi, scene, W0, H0, segments, 0, rows=(y0, y1)) as ctx:
        upload(abi, ctx, scene, spec)
        strip = frame(abi, oracle, ctx, scene, W0, H0)
    same_bits(strip["IMAGE"], out["default"]["IMAGE"][y0:y1], (name, form, segments, "strip", "IMAGE"))
    same_bits(strip["HIT_ID"], out["default"]["HIT_ID"][y0:y1], (name, form, segments, "strip", "HIT_ID"))
    assert strip["rays"] == counted and 0 < counted < out["default"]["rays"]
    assert out["default"]["rays"] < segments * W0 * H0, "paths end early"
    if segments == 33:
        assert out["default"]["rays"] > W0 * H0 * (0.4 if name == "glossy_trench" else 4), "... and many cross the windows"


# ------------------------------------------------------------------------------------------ 6. absorption
@pytest.mark.parametrize("name,form", list(S.ABSORBED), ids=[f"{n}-{f}" for n, f in S.ABSORBED])
def test_absorbed_paths_are_black(hip_lib, oracle, name, form):
    """33 segments, one launch, demodulated: a pixel whose IMAGE is exactly 0 while its ALBEDO is not ended absorbed (every
    factor of a surviving path is positive and its product far above the smallest binary32 number; the sky and the lights are
    positive)"""
    abi = hip_lib
    scene, spec = _scene(name, form)
    with context(abi, scene, W0, H0, 33, SINGLE_LAUNCH | DEMODULATE) as ctx:
        upload(abi, ctx, scene, spec)
        got = frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",))
    rgb, alb = got["IMAGE"][..., :3], got["ALBEDO"][..., :3]
    assert (alb > 0).all()
    black = (rgb == 0).all(-1)
    partly = (rgb == 0).any(-1) & ~black
    print(f"absorbed {name} {form}: {black.sum()} of {black.size} pixels")
    assert not partly.any(), "absorption zeroes all three channels"
    assert black.sum() > 0
    assert black.sum() >= S.ABSORBED[name, form] // 2


# ------------------------------------------------------------------------------------------ 7. demodulation, textures, lifetime
@pytest.mark.parametrize("name,form", [("mixed_room", "small"), ("glossy_trench", "small"), ("glossy_trench", "pairs")])
def test_specular_trace_factorises(hip_lib, oracle, name, form):
    """test_demodulate_gpu's factorisation: IMAGE x ALBEDO of the demodulated trace against the plain trace within the
    multiply-order bound (segments + 2) 2^-23 |value|; ALBEDO of a specular first hit is Ks"""
    abi = hip_lib
    scene, spec = _scene(name, form)
    for vid, vflags, seg in D.variants():
        out = {}
        for on in (True, False):
            with context(abi, scene, W0, H0, seg, vflags | (DEMODULATE if on else 0)) as ctx:
                upload(abi, ctx, scene, spec)
                out[on] = frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",) if on else ())
        a, b = out[True], out[False]
        same_bits(a["HIT_ID"], b["HIT_ID"], (name, form, vid, "HIT_ID"))
        assert a["rays"] == b["rays"]
        alb, on_img, off_img, hit = a["ALBEDO"][..., :3], a["IMAGE"][..., :3], b["IMAGE"][..., :3], a["HIT_ID"]
        ended = (alb == 1).all(-1)
        same_bits(on_img[ended], off_img[ended], (name, form, vid, "ended at the first query"))
        went_on = ~ended
        mat = scene.tri_material[hit[went_on] - 1]
        colour = scene.materials[:, :3].copy()
        for m, (ks, _) in spec.items():
            colour[m] = ks
        same_bits(alb[went_on], colour[mat], (name, form, vid, "ALBEDO"))
        assert np.isin(mat, list(spec)).any() and (~np.isin(mat, list(spec))).any(), "first hits of both kinds"
        prod = (on_img * alb).astype(F32)
        err = np.abs(prod.astype(np.float64) - off_img.astype(np.float64))
        bound = (seg + 2) * 2.0 ** -23 * np.abs(off_img.astype(np.float64))
        assert (err[went_on] <= bound[went_on]).all(), (name, form, vid)
        assert ((prod == 0) == (off_img == 0))[went_on].all(), "an absorbed path is black on both sides"


@pytest.mark.parametrize("tflags", [0, TS.NEAREST], ids=["bilinear", "nearest"])
def test_textured_mirror_stores_ks_times_texel(hip_lib, oracle, tflags):
    abi = hip_lib
    scene, spec = S.mirror_quad()
    ks, colour = (0.9, 0.6, 0.35), (0.3, 0.55, 0.8)
    desc, texels = TS.atlas([TS.constant_image(3, 5, colour)], tflags)
    uv = TS.random_uv(len(scene.tris), 11)
    for W, H in S.SIZES:
        with context(abi, scene, W, H, 2, DEMODULATE) as ctx:
            upload(abi, ctx, scene, {0: (ks, 0.0)})
            ctx.set_textures(uv, np.ones(len(scene.tris), np.uint32), desc, texels)
            got = frame(abi, oracle, ctx, scene, W, H, ("ALBEDO",))
        on = got["HIT_ID"] > 0
        texel = TS.sample(texels, desc[0], np.full((1, 2), 0.5, F32))[0, :3]
        want = (F32(ks) * texel).astype(F32)
        same_bits(got["ALBEDO"][..., :3][on], np.broadcast_to(want, (on.sum(), 3)), ("textured mirror", W, H))
        assert on.any() and (got["ALBEDO"][..., :3][~on] == 1).all()


def test_lifetime_of_the_set(hip_lib, oracle):
    """the room of mirrors keeps its closed form through rtpt_scene_set_instances, rtpt_scene_rebuild, a changed model and
    rtpt_resize (a moved closed room is a closed room); rtpt_scene_upload drops the set, rtpt_scene_set_materials replaces it;
    the device bytes are the old call's"""
    abi = hip_lib
    gc.collect()
    scene, spec = S.mirror_room("pairs")
    n = 4
    value = F32([2.0 ** -n, 2.0 ** -(2 * n), 2.0 ** -(3 * n)])
    mesh = FP.mesh_of(scene.tris)

    def is_closed_form(ctx, W, H, model=None):
        pc = T.G.fill_push_constants(abi.PushConstants(), P.push_constants(scene), 0)
        ubo = T._ubo(abi, oracle, scene, W, H)
        if model is not None:
            ubo.model[:] = model
        ctx.reset_counters()
        ctx.gbuffer(ubo)
        ctx.temporal_gradient(pc)
        ctx.raytrace(pc)
        rgb = ctx.readback(abi.PLANE_IMAGE)[..., :3]
        ctx.end_frame()
        return np.array_equal(bits(rgb), bits(np.broadcast_to(value, rgb.shape))) and ctx.raycount() == n * W * H

    with context(abi, scene, W0, H0, n) as ctx:
        ctx.scene_upload(*mesh)
        base = abi.live_device_bytes()
        ctx.set_materials(scene.tri_material, scene.materials)
        old_bytes = abi.live_device_bytes() - base
        assert old_bytes == 32 * len(scene.tris)
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, spec))      # (before any frame allocates its buffers)
        assert abi.live_device_bytes() - base == old_bytes, "rtpt_debug_live_device_bytes reads as after rtpt_scene_set_materials"
        ctx.set_materials_ext(None, None)
        assert abi.live_device_bytes() == base
        ctx.set_materials(scene.tri_material, scene.materials)
        assert not is_closed_form(ctx, W0, H0)
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, spec))
        assert is_closed_form(ctx, W0, H0)
        ctx.scene_set_instances(F32([[1, 0, 0, 0.01, 0, 1, 0, -0.02, 0, 0, 1, 0.03]]))
        assert is_closed_form(ctx, W0, H0), "rtpt_scene_set_instances keeps the set"
        ctx.scene_rebuild()
        assert is_closed_form(ctx, W0, H0), "rtpt_scene_rebuild keeps the set"
        model = np.eye(4, dtype=F32)
        model[3, :3] = (0.02, 0.01, -0.03)      # column-major: a translation
        assert is_closed_form(ctx, W0, H0, model.ravel()), "a changed model keeps the set"
        ctx.resize(70, 10)
        assert is_closed_form(ctx, 70, 10, model.ravel()), "rtpt_resize keeps the set"
        ctx.resize(W0, H0)
        ctx.set_materials(scene.tri_material, scene.materials)
        assert not is_closed_form(ctx, W0, H0, model.ravel()), "the old call replaces the set"
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, spec))
        assert is_closed_form(ctx, W0, H0, model.ravel())
        ctx.set_materials_ext(None, None)
        assert not is_closed_form(ctx, W0, H0, model.ravel()), "NULL drops the set"
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, spec))
        ctx.scene_upload(*mesh)
        assert not is_closed_form(ctx, W0, H0), "rtpt_scene_upload drops the set"


def test_refusals_leave_the_scene_untouched(hip_lib, oracle):
    abi = hip_lib
    scene, spec = S.mixed_room("small")
    good = abi.materials_ext(scene.materials, spec)
    tri = scene.tri_material

    def bad_calls():
        yield "wrong n_tris", (tri[:-1], good)
        t = tri.copy(); t[3] = len(good)
        yield "index out of range", (t, good)
        m = good.copy(); m["flags"][0] = 2
        yield "unknown flag", (tri, m)
        for field in ("albedo", "emission", "specular"):
            for v in (np.nan, np.inf, -np.inf):
                m = good.copy(); m[field][2, 1] = v
                yield f"{field} {v}", (tri, m)
        m = good.copy(); m["roughness"][0] = np.nan
        yield "roughness nan", (tri, m)
        for g in (-0.25, 1.5):
            m = good.copy(); m["roughness"][3] = g
            yield f"roughness {g}", (tri, m)
        m = good.copy(); m["emission"][1, 2] = 0.5
        yield "specular and emissive", (tri, m)

    with abi.Context(abi.config_default(64, 48)) as ctx:
        with pytest.raises(abi.RtptError) as e:
            ctx.set_materials_ext(tri, good)
        assert e.value.code == abi.RTPT_E_NO_SCENE
    for with_set in (False, True):
        frames = []
        for refused in (False, True):
            with context(abi, scene, W0, H0, 9) as ctx:
                ctx.scene_upload(*FP.mesh_of(scene.tris))
                if with_set:
                    ctx.set_materials_ext(tri, good)
                held = abi.live_device_bytes()
                if refused:
                    for what, args in bad_calls():
                        with pytest.raises(abi.RtptError) as e:
                            ctx.set_materials_ext(*args)
                        assert e.value.code == abi.RTPT_E_INVALID, what
                    assert abi.live_device_bytes() == held
                frames.append(frame(abi, oracle, ctx, scene, W0, H0))
        same_frame(frames[1], frames[0], ("refusals", with_set))


def test_frame_reuse_goes_on_across_the_call(hip_lib, monkeypatch):
    """a resting Cornell box; two of its fan pairs become a mirror and a glossy surface between frames 4 and 5.  K0 and K1 stay
    unlaunched (rtpt_debug_reuse_info [0] keeps counting) and every frame equals the frame of a context that reuses nothing"""
    abi = hip_lib
    mesh = abi.load_obj(D.SCENE)
    tri, mats = D.material_table(len(mesh[1]))
    first = abi.materials_ext(mats)
    second = abi.materials_ext(mats, {0: ((0.9, 0.9, 0.9), 0.0), 5: ((0.8, 0.6, 0.4), 0.3)})
    for size in S.SIZES:
        frames = {}
        for reuse in (True, False):
            if reuse:
                monkeypatch.delenv("RTPT_NO_FRAME_REUSE", raising=False)
            else:
                monkeypatch.setenv("RTPT_NO_FRAME_REUSE", "1")
            app = D.make(abi, size, 0, 4, mesh)
            ctx = app.backend.ctx
            ctx.set_materials_ext(tri, first)
            out, skipped = [], []
            for f in range(8):
                if f == 5:
                    ctx.set_materials_ext(tri, second)
                app.drawScene(())
                out.append(app.backend.final_image_rows(0, size[1]).copy())
                skipped.append(ctx.reuse_info()["frames_skipped"])
            frames[reuse] = out
            if reuse:
                assert skipped[4] > 0, "frames were being reused before the change"
                assert [skipped[f] - skipped[f - 1] for f in (5, 6, 7)] == [1, 1, 1], skipped
            else:
                assert skipped[-1] == 0
            app.backend.close()
        for f in range(8):
            assert np.array_equal(bits(frames[True][f]), bits(frames[False][f])), (size, f)
        assert not np.array_equal(bits(frames[True][4]), bits(frames[True][5]))


# ------------------------------------------------------------------------------------------ 8. hosts
KEYS = ["", "E", "J", "QA", "D", "SI"]
SIZE_IDS = [f"{w}x{h}" for w, h in S.SIZES]


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    return S.write_specular_room(str(tmp_path_factory.mktemp("specular_room")))


def host_frames(room, size, in_flight=1, **kw):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    app = make_app(size[0], size[1], max_segments=5, iterations=5, scene=room, frames_in_flight=in_flight, **kw)
    frames = []
    for k in KEYS:
        app.drawScene(tuple(k))
        frames.append(app.backend.final_image_rows(0, size[1]).copy())
    rays = sum(b.ctx.raycount() for b in getattr(app.backend, "be", [app.backend]))
    app.backend.close()
    return frames, rays


@pytest.fixture(scope="module")
def serial_host(hip_lib, room):
    return {size: host_frames(room, size, specular=True) for size in S.SIZES}


@pytest.mark.parametrize("size", S.SIZES, ids=SIZE_IDS)
def test_python_host_applies_the_rule_only_when_asked(hip_lib, room, serial_host, size):
    abi = hip_lib
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    tri, m = abi.load_obj_materials_ext(room)
    assert sorted(np.flatnonzero(m["flags"]).tolist()) == [3, 4], "the mirror and the glossy strip; the satin panel (illum 2) stays diffuse"
    plain, _ = host_frames(room, size)
    assert not np.array_equal(bits(plain[-1]), bits(serial_host[size][0][-1]))
    app = make_app(*size, max_segments=5, iterations=5, scene=room)      # specular=True is what the explicit call gives
    app.backend.ctx.set_materials_ext(tri, m)
    app.drawScene(())
    assert np.array_equal(bits(app.backend.final_image_rows(0, size[1])), bits(serial_host[size][0][0]))
    app.backend.close()


@pytest.mark.parametrize("size", S.SIZES, ids=SIZE_IDS)
def test_two_frames_in_flight_equal_the_serial_host(hip_lib, room, serial_host, size):
    frames, rays = host_frames(room, size, in_flight=2, specular=True)
    for f in range(len(KEYS)):
        assert np.array_equal(bits(frames[f]), bits(serial_host[size][0][f])), f
    assert rays == serial_host[size][1]


@pytest.mark.parametrize("extra", [[], ["--ranks", "2"]], ids=["single", "ranks2"])
@pytest.mark.parametrize("size", S.SIZES, ids=SIZE_IDS)
def test_cpp_host_equals_the_python_host(hip_lib, room, serial_host, tmp_path, size, extra):
    """rtpt_app --specular dumps the Python host's last frame bit for bit, as one context and as two strip contexts"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    app_binary = os.path.join(D.PKG, "rtpt_app")
    assert os.path.exists(app_binary), "build() leaves rtpt_app next to the package"
    W, H = size
    pfm = tmp_path / "out.pfm"
    cmd = [app_binary, "--width", str(W), "--height", str(H), "--segments", "5", "--iterations", "5", "--frames", str(len(KEYS)),
           "--script", ",".join(KEYS), "--dump", str(pfm), "--scene", room, "--specular"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    stats = json.loads(out.stdout.strip().splitlines()[-1])
    frames, rays = serial_host[size]
    assert np.array_equal(bits(read_pfm(str(pfm))), bits(np.ascontiguousarray(frames[-1][..., :3])))
    assert stats["rays"] == rays
