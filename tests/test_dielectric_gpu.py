"""Dielectric materials on the device (RTPT_MAT_DIELECTRIC, csrc/dielectric.hpp), in the order of what each check can catch: the
interface function against its numpy restatement, one interface end to end in closed form from the front and from behind,
whole frames of a glass box in a room against the numpy path walker of tests/dielectric_scenes.py (held to the oracle's frames
on the CPU, tests/test_dielectric_cpu.py), the specular scenes through the new instantiations against the oracle, demodulation,
lifetime / refusals / frame reuse, and the two hosts.  Every test here fails on a library without the feature."""
import gc
import json
import os
import subprocess

import numpy as np
import pytest

import dielectric_scenes as DS
import filter_planes as FP
import path_walker as WK
import pathtrace_scenes as P
import specular_scenes as S
import test_demodulate_gpu as D
import test_pathtrace_scenes_gpu as T
from conftest import bits
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
W0, H0 = DS.SIZES[0]
NO_COMPACTION, SINGLE_LAUNCH, FORCE_BVH, DEMODULATE = 0x8, 0x200, 0x2, 0x8000
STRIP_ROWS = (5, 21)

_walked = {}


# ------------------------------------------------------------------------------------------ one frame, both sides
def upload(abi, ctx, scene, specular=None, dielectric=None):
    ctx.scene_upload(*FP.mesh_of(scene.tris))
    ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, specular, dielectric))


def context(abi, scene, W, H, segments, flags=0, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def frame(abi, oracle, ctx, scene, W, H, planes=()):
    out = T.frame_on_gpu(abi, oracle, ctx, scene, W, H)
    for p in planes:
        out[p] = ctx.readback(getattr(abi, "PLANE_" + p))
    return out


def walked(oracle, form, W, H, segments, spp=1):
    """the walker's frame of the glass room, computed once and left unchanged"""
    key = (form, W, H, segments, spp)
    if key not in _walked:
        scene, glass = DS.glass_room(form)
        r = WK.walk(oracle, scene, W, H, segments, DS.records(scene, None, glass), spp=spp)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _walked[key] = r
    return _walked[key]


def same_frame(got, want, tag, rows=None):
    y0, y1 = rows or (0, len(want["IMAGE"]))
    same_bits(got["HIT_ID"], want["HIT_ID"][y0:y1], tag + ("HIT_ID",))
    same_bits(got["IMAGE"], want["IMAGE"][y0:y1], tag + ("IMAGE",))


# ------------------------------------------------------------------------------------------ 1. the function
def test_refract_equals_the_restatement(hip_lib, oracle):
    """rtpt_selftest_refract, one case per lane, against dielectric_scenes.refract32 bit for bit: d', the transmitted flag and F, on
    the CPU test's hostile operands and 4 096 seeded ones"""
    abi = hip_lib
    cases = np.concatenate([DS.hostile_cases(oracle), DS.seeded_cases()])
    with abi.Context(abi.config_default(64, 48)) as ctx:
        got = ctx.selftest_refract(cases)
    want = DS.refract32(oracle, cases)
    same_bits(got[:, :3], want[:, :3], ("refract", "d'"))
    same_bits(got[:, 3], want[:, 3], ("refract", "transmitted"))
    same_bits(got[:, 4], want[:, 4], ("refract", "F"))
    assert 0.2 * len(got) < (got[:, 3] != 0).sum() < 0.8 * len(got)


# ------------------------------------------------------------------------------------------ 2. one interface, closed form
def _quad_expectation(oracle, scene, glass, W, H, hit):
    """colour x sky(d') of every pixel whose primary ray meets the quad (HIT_ID): d' and the choice from the pixel's own first draw
    behind the jitter's two, through refract32 on the walker's primary direction and the triangle's stored normal"""
    rng, d = DS.primary_rays(oracle, scene, W, H)
    normals = DS.stored_normals(oracle, scene.tris)
    colour, ior = glass[0]
    ys, xs = np.nonzero(hit > 0)
    u = np.array([oracle.rng_steps(int(rng[y, x]), 2)[1] for y, x in zip(ys, xs)], F32).reshape(-1, 2)
    cases = np.concatenate([d[ys, xs], normals[hit[ys, xs] - 1], u, np.full((len(ys), 1), ior, F32)], 1)
    out = DS.refract32(oracle, cases)
    want = np.asarray(colour, np.float64) * S.sky64(out[:, :3].astype(np.float64))
    return (ys, xs), out, want, DS.refract64(cases)


@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
def test_glass_quad_shows_the_sky_of_the_chosen_ray(hip_lib, oracle, vflags):
    """specular_scenes.mirror_quad's quad as glass (ior 1.5, colour (1, 1/2, 1/4)), pixel_jitter 0, two segments, the light out of
    reach: every pixel on the quad is colour x sky(d'), d' the reflected or the refracted direction by the pixel's own first draw,
    within test_mirror_quad_shows_the_sky_of_the_reflected_ray's bar of 2^-16 absolute.  Both outcomes occur: the reflected ray
    sees the sky's gradient, the refracted one goes below the horizon.
    Measured on an MI355X, brute force and forced BVH alike: 64 x 48 (1688 pixels on the quad, 54 reflect) and 70 x 10 (80 pixels, 6
    reflect) max abs error 1.490e-08; the bar is 1.526e-05."""
    abi = hip_lib
    scene, glass = DS.glass_quad()
    for W, H in DS.SIZES:
        with context(abi, scene, W, H, 2, vflags) as ctx:
            upload(abi, ctx, scene, None, glass)
            got = frame(abi, oracle, ctx, scene, W, H)
        on, _ = S.mirror_quad_expectation(W, H)
        assert np.array_equal(got["HIT_ID"] > 0, on), "the numpy ray and K2 agree on the pixels that hit the quad"
        (ys, xs), out, want, _ = _quad_expectation(oracle, scene, glass, W, H, got["HIT_ID"])
        err = np.abs(got["IMAGE"][..., :3][ys, xs].astype(np.float64) - want)
        transmitted = out[:, 3] != 0
        print(f"glass quad {W} x {H} flags {vflags:#x}: {len(ys)} pixels on the quad, {int((~transmitted).sum())} reflect, max abs error "
              f"{err.max():.3e} (bar {2.0 ** -16:.3e})")
        assert err.max() <= 2.0 ** -16
        assert transmitted.any() and (~transmitted).any(), "both outcomes occur among the pixels"
        assert (out[transmitted, 1] < 0).all() and (out[~transmitted, 1] > 0.3).all(), "refracted rays go down, reflected ones up"
        assert got["rays"] == W * H + on.sum()


@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
def test_glass_quad_from_behind_reflects_everything(hip_lib, oracle, vflags):
    """the same quad met from inside the medium beyond the critical angle (dielectric_scenes.glass_quad_from_behind): float64's k is
    below -0.05 at every pixel on the quad, so every one reflects whatever its draw — F is 1 — and shows colour x sky(reflect(d)).
    Measured on an MI355X, brute force and forced BVH alike: 52 pixels, max abs error 2.980e-08; the bar is 1.526e-05."""
    abi = hip_lib
    scene, glass = DS.glass_quad_from_behind()
    W, H = DS.BEHIND_SIZE
    with context(abi, scene, W, H, 2, vflags) as ctx:
        upload(abi, ctx, scene, None, glass)
        got = frame(abi, oracle, ctx, scene, W, H)
    (ys, xs), out, want, f64 = _quad_expectation(oracle, scene, glass, W, H, got["HIT_ID"])
    assert len(ys) >= 40 and (got["HIT_ID"] == 0).any()
    assert (f64["k"] < -0.05).all(), "beyond the critical angle, from inside"
    cases_n = DS.stored_normals(oracle, scene.tris)[got["HIT_ID"][ys, xs] - 1]
    assert ((cases_n * DS.primary_rays(oracle, scene, W, H)[1][ys, xs]).sum(1) > 0).all(), "the stored normal points away from the camera"
    assert (out[:, 3] == 0).all() and (out[:, 4] == 1).all()
    err = np.abs(got["IMAGE"][..., :3][ys, xs].astype(np.float64) - want)
    print(f"glass quad from behind flags {vflags:#x}: {len(ys)} pixels, max abs error {err.max():.3e} (bar {2.0 ** -16:.3e})")
    assert err.max() <= 2.0 ** -16
    assert (out[:, 1] > 0.3).all(), "the reflected rays see the sky's gradient"
    assert got["rays"] == W * H + len(ys)


# ------------------------------------------------------------------------------------------ 3. whole frames against the walker
FRAME_CASES = [("small", 0), ("pairs", 0), ("small", FORCE_BVH)]


@pytest.mark.parametrize("segments", [9, 33])
@pytest.mark.parametrize("form,base", FRAME_CASES, ids=["small", "pairs", "force_bvh"])
def test_glass_room_equals_the_walker(hip_lib, oracle, form, base, segments):
    """a closed glass box in a diffuse room with a lamp: IMAGE and HIT_ID of the walker bit for bit, and its ray count.  9 and 33
    segments cross the hand-over windows (4 / 8 / 16, 8 / 16 / 32).  The default schedule, RTPT_FLAG_NO_PATH_COMPACTION,
    RTPT_FLAG_SINGLE_LAUNCH_PATHS, and a strip context with row_begin > 0"""
    abi = hip_lib
    scene, glass = DS.glass_room(form)
    want = walked(oracle, form, W0, H0, segments)
    assert want["rays"] > 2 * W0 * H0
    for sid, flags in (("default", 0), ("no_compaction", NO_COMPACTION), ("single_launch", SINGLE_LAUNCH)):
        with context(abi, scene, W0, H0, segments, base | flags) as ctx:
            upload(abi, ctx, scene, None, glass)
            if form != "small":
                assert ctx.scene_build_info()["leaf_pairs"]
            got = frame(abi, oracle, ctx, scene, W0, H0)
        same_frame(got, want, (form, base, segments, sid))
        assert got["rays"] == want["rays"], (form, base, segments, sid)
    with context(abi, scene, W0, H0, segments, base, rows=STRIP_ROWS) as ctx:
        upload(abi, ctx, scene, None, glass)
        strip = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(strip, want, (form, base, segments, "strip"), STRIP_ROWS)


@pytest.mark.parametrize("form,base", FRAME_CASES, ids=["small", "pairs", "force_bvh"])
def test_glass_room_second_shape_and_samples(hip_lib, oracle, form, base):
    """70 x 10 (partial tiles in x and y), and two and three samples per pixel: every sample goes on with the pixel's stream, which
    a path that ends on its last segment still moves by its two draws"""
    abi = hip_lib
    scene, glass = DS.glass_room(form)
    W, H = DS.SIZES[1]
    for segments, spp in ((9, 1), (2, 2), (5, 3)):
        want = walked(oracle, form, W, H, segments, spp)
        with context(abi, scene, W, H, segments, base, spp) as ctx:
            upload(abi, ctx, scene, None, glass)
            got = frame(abi, oracle, ctx, scene, W, H)
        same_frame(got, want, (form, base, segments, spp))
        assert got["rays"] == want["rays"]


# ------------------------------------------------------------------------------------------ 4. no dielectric in reach
FAR_SCENES = [("mixed_room", "small"), ("mixed_room", "pairs"), ("glossy_trench", "small"), ("glossy_trench", "odd")]


@pytest.mark.parametrize("name,form", FAR_SCENES, ids=[f"{n}-{f}" for n, f in FAR_SCENES])
def test_specular_scenes_through_the_dielectric_kernels(hip_lib, oracle, name, form):
    """the specular scenes plus a far glass pair no path reaches (specular_scenes.with_far_pair): the kernels that know the
    interface are chosen, and IMAGE, HIT_ID and the ray count are oracle.raytrace_ext's of the scene, bit for bit — every K2
    variant of test_demodulate_gpu.variants(), and 33 segments"""
    abi = hip_lib
    scene, spec = {"mixed_room": S.mixed_room, "glossy_trench": S.glossy_trench}[name](form)
    far, far_mat = DS.with_far_glass_pair(scene)
    for vid, vflags, seg in D.variants() + [("default_33", 0, 33)]:
        want = DS.oracle_ext_frame(oracle, far, W0, H0, seg, spec)
        assert not (want["HIT_ID"] > len(scene.tris)).any(), "no primary ray sees the far pair"
        with context(abi, far, W0, H0, seg, vflags) as ctx:
            upload(abi, ctx, far, spec, {far_mat: (DS.GLASS_COLOUR, DS.GLASS_IOR)})
            got = frame(abi, oracle, ctx, far, W0, H0)
        same_frame(got, want, (name, form, vid))
        assert got["rays"] == want["rays"], (name, form, vid)


# ------------------------------------------------------------------------------------------ 5. demodulated
@pytest.mark.parametrize("form,base", FRAME_CASES, ids=["small", "pairs", "force_bvh"])
def test_glass_trace_factorises(hip_lib, oracle, form, base):
    """test_specular_trace_factorises on the glass room: IMAGE x ALBEDO of the demodulated trace against the plain trace within the
    multiply-order bound (segments + 2) 2^-23 |value|; ALBEDO of a first hit on glass is the glass's colour"""
    abi = hip_lib
    scene, glass = DS.glass_room(form)
    colour = scene.materials[:, :3].copy()
    for m, (c, _) in glass.items():
        colour[m] = c
    for seg, flags in ((4, 0), (8, 0), (8, SINGLE_LAUNCH), (4, NO_COMPACTION)):
        out = {}
        for on in (True, False):
            with context(abi, scene, W0, H0, seg, base | flags | (DEMODULATE if on else 0)) as ctx:
                upload(abi, ctx, scene, None, glass)
                out[on] = frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",) if on else ())
        a, b = out[True], out[False]
        same_bits(a["HIT_ID"], b["HIT_ID"], (form, seg, flags, "HIT_ID"))
        same_bits(b["IMAGE"], walked(oracle, form, W0, H0, seg)["IMAGE"], (form, seg, flags, "the plain trace is the walker's"))
        assert a["rays"] == b["rays"]
        alb, on_img, off_img, hit = a["ALBEDO"][..., :3], a["IMAGE"][..., :3], b["IMAGE"][..., :3], a["HIT_ID"]
        ended = (alb == 1).all(-1)
        same_bits(on_img[ended], off_img[ended], (form, seg, flags, "ended at the first query"))
        went_on = ~ended
        mat = scene.tri_material[hit[went_on] - 1]
        same_bits(alb[went_on], colour[mat], (form, seg, flags, "ALBEDO"))
        assert (mat == 6).sum() > 100 and (mat != 6).sum() > 100, "first hits on glass and on walls"
        prod = (on_img * alb).astype(F32)
        err = np.abs(prod.astype(np.float64) - off_img.astype(np.float64))
        bound = (seg + 2) * 2.0 ** -23 * np.abs(off_img.astype(np.float64))
        assert (err[went_on] <= bound[went_on]).all(), (form, seg, flags)


# ------------------------------------------------------------------------------------------ 6. lifetime, refusals, frame reuse
def test_lifetime_of_the_set(hip_lib, oracle):
    """the closed room with every wall glass of ior 1: nothing is totally reflected and Schlick's term is (1 - cos)^5, so most paths
    cross their first wall and leave for the sky after two rays, where every path of the diffuse room lives to the bound —
    exactly n W H rays.  The set survives
    rtpt_scene_set_instances, rtpt_scene_rebuild, a changed model and rtpt_resize; rtpt_scene_upload drops it,
    rtpt_scene_set_materials replaces it; the device bytes are the old call's"""
    abi = hip_lib
    gc.collect()
    scene = P.closed_room("pairs")
    glass = {m: (P.WALL_KD[m], 1.0) for m in range(len(scene.materials))}
    n = 4
    mesh = FP.mesh_of(scene.tris)

    def is_glass(ctx, W, H, model=None):
        pc = T.G.fill_push_constants(abi.PushConstants(), P.push_constants(scene), 0)
        ubo = T._ubo(abi, oracle, scene, W, H)
        if model is not None:
            ubo.model[:] = model
        ctx.reset_counters()
        ctx.gbuffer(ubo)
        ctx.temporal_gradient(pc)
        ctx.raytrace(pc)
        ctx.end_frame()
        if ctx.raycount() == n * W * H:
            return False
        assert 2 * W * H <= ctx.raycount() < 3 * W * H, ctx.raycount() / (W * H)
        return True

    with context(abi, scene, W0, H0, n) as ctx:
        ctx.scene_upload(*mesh)
        base = abi.live_device_bytes()
        ctx.set_materials(scene.tri_material, scene.materials)
        old_bytes = abi.live_device_bytes() - base
        assert old_bytes == 32 * len(scene.tris)
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, None, glass))
        assert abi.live_device_bytes() - base == old_bytes
        ctx.set_materials_ext(None, None)
        assert abi.live_device_bytes() == base
        ctx.set_materials(scene.tri_material, scene.materials)
        assert not is_glass(ctx, W0, H0)
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, None, glass))
        assert is_glass(ctx, W0, H0)
        ctx.scene_set_instances(F32([[1, 0, 0, 0.01, 0, 1, 0, -0.02, 0, 0, 1, 0.03]]))
        assert is_glass(ctx, W0, H0), "rtpt_scene_set_instances keeps the set"
        ctx.scene_rebuild()
        assert is_glass(ctx, W0, H0), "rtpt_scene_rebuild keeps the set"
        model = np.eye(4, dtype=F32)
        model[3, :3] = (0.02, 0.01, -0.03)
        assert is_glass(ctx, W0, H0, model.ravel()), "a changed model keeps the set"
        ctx.resize(70, 10)
        assert is_glass(ctx, 70, 10, model.ravel()), "rtpt_resize keeps the set"
        ctx.resize(W0, H0)
        ctx.set_materials(scene.tri_material, scene.materials)
        assert not is_glass(ctx, W0, H0, model.ravel()), "the old call replaces the set"
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, None, glass))
        assert is_glass(ctx, W0, H0, model.ravel())
        ctx.set_materials_ext(None, None)
        assert not is_glass(ctx, W0, H0, model.ravel()), "NULL drops the set"
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, None, glass))
        ctx.scene_upload(*mesh)
        assert not is_glass(ctx, W0, H0), "rtpt_scene_upload drops the set"


def test_refusals_leave_the_scene_untouched(hip_lib, oracle):
    abi = hip_lib
    scene, glass = DS.glass_room("small")
    good = abi.materials_ext(scene.materials, None, glass)
    tri = scene.tri_material

    def bad_calls():
        m = good.copy(); m["flags"][6] = abi.MAT_DIELECTRIC | abi.MAT_SPECULAR
        yield "both flags", m
        m = good.copy(); m["roughness"][6] = 0.25
        yield "a rough dielectric", m
        m = good.copy(); m["emission"][6, 1] = 0.5
        yield "an emissive dielectric", m
        for v in (np.nan, np.inf, -np.inf, 0.0, 0.5, np.nextafter(F32(1), F32(0)), -1.5):
            m = good.copy(); m["ior"][6] = v
            yield f"ior {v}", m
        m = good.copy(); m["flags"][0] = abi.MAT_DIELECTRIC      # a wall's word is 0: no ior
        yield "the flag without an ior", m
        m = good.copy(); m["flags"][6] = 4
        yield "unknown flag", m

    ignored = good.copy()
    ignored["_pad"][:6] = 0x7fc00000      # without the flag the word is ignored
    for with_set in (False, True):
        frames = []
        for refused in (False, True):
            with context(abi, scene, W0, H0, 9) as ctx:
                ctx.scene_upload(*FP.mesh_of(scene.tris))
                if with_set:
                    ctx.set_materials_ext(tri, ignored if refused else good)
                held = abi.live_device_bytes()
                if refused:
                    for what, m in bad_calls():
                        with pytest.raises(abi.RtptError) as e:
                            ctx.set_materials_ext(tri, m)
                        assert e.value.code == abi.RTPT_E_INVALID, what
                    assert abi.live_device_bytes() == held
                frames.append(frame(abi, oracle, ctx, scene, W0, H0))
        same_frame(frames[1], frames[0], ("refusals", with_set))
        assert frames[1]["rays"] == frames[0]["rays"]
        if with_set:
            same_frame(frames[0], walked(oracle, "small", W0, H0, 9), ("the accepted set is the walker's",))


def test_frame_reuse_goes_on_across_the_call(hip_lib, monkeypatch):
    """a resting Cornell box; two of its fan pairs become glass between frames 4 and 5.  K0 and K1 stay unlaunched
    (rtpt_debug_reuse_info keeps counting) and every frame equals the frame of a context that reuses nothing"""
    abi = hip_lib
    mesh = abi.load_obj(D.SCENE)
    tri, mats = D.material_table(len(mesh[1]))
    first = abi.materials_ext(mats)
    second = abi.materials_ext(mats, None, {0: ((0.9, 0.9, 0.9), 1.5), 5: ((0.8, 0.6, 0.4), 1.33)})
    size = DS.SIZES[0]
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
        assert np.array_equal(bits(frames[True][f]), bits(frames[False][f])), f
    assert not np.array_equal(bits(frames[True][4]), bits(frames[True][5]))


# ------------------------------------------------------------------------------------------ 7. hosts
KEYS = ["", "E", "J", "QA", "D", "SI"]
SIZE_IDS = [f"{w}x{h}" for w, h in DS.SIZES]


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    return DS.write_glass_room(str(tmp_path_factory.mktemp("glass_room")))


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
    return {size: host_frames(room, size, dielectric=True) for size in DS.SIZES}


@pytest.mark.parametrize("size", DS.SIZES, ids=SIZE_IDS)
def test_python_host_applies_the_rule_only_when_asked(hip_lib, room, serial_host, size, tmp_path):
    """dielectric=True is the explicit call with the new loader's table; on the glass room it differs from specular=True, on
    specular_scenes' room (no Ni anywhere) it is specular=True bit for bit"""
    abi = hip_lib
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    tri, m = abi.load_obj_materials_ni(room)
    assert np.flatnonzero(m["flags"] == abi.MAT_DIELECTRIC).tolist() == [5] and np.flatnonzero(m["flags"] == abi.MAT_SPECULAR).tolist() == [3, 4]
    assert np.array_equal(m["specular"][5], F32([0.9, 0.95, 1.0])), "Tf is the pane's colour"
    with_specular, _ = host_frames(room, size, specular=True)
    assert not np.array_equal(bits(with_specular[-1]), bits(serial_host[size][0][-1]))
    app = make_app(*size, max_segments=5, iterations=5, scene=room)
    app.backend.ctx.set_materials_ext(tri, m)
    app.drawScene(())
    assert np.array_equal(bits(app.backend.final_image_rows(0, size[1])), bits(serial_host[size][0][0]))
    app.backend.close()
    plain_room = S.write_specular_room(str(tmp_path))
    a, ra = host_frames(plain_room, size, dielectric=True)
    b, rb = host_frames(plain_room, size, specular=True)
    assert ra == rb and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("size", DS.SIZES, ids=SIZE_IDS)
def test_two_frames_in_flight_equal_the_serial_host(hip_lib, room, serial_host, size):
    frames, rays = host_frames(room, size, in_flight=2, dielectric=True)
    for f in range(len(KEYS)):
        assert np.array_equal(bits(frames[f]), bits(serial_host[size][0][f])), f
    assert rays == serial_host[size][1]


@pytest.mark.parametrize("extra", [[], ["--ranks", "2"]], ids=["single", "ranks2"])
@pytest.mark.parametrize("size", DS.SIZES, ids=SIZE_IDS)
def test_cpp_host_equals_the_python_host(hip_lib, room, serial_host, tmp_path, size, extra):
    """rtpt_app --dielectric dumps the Python host's last frame bit for bit, as one context and as two strip contexts"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    app_binary = os.path.join(D.PKG, "rtpt_app")
    assert os.path.exists(app_binary), "build() leaves rtpt_app next to the package"
    W, H = size
    pfm = tmp_path / "out.pfm"
    cmd = [app_binary, "--width", str(W), "--height", str(H), "--segments", "5", "--iterations", "5", "--frames", str(len(KEYS)),
           "--script", ",".join(KEYS), "--dump", str(pfm), "--scene", room, "--dielectric"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    stats = json.loads(out.stdout.strip().splitlines()[-1])
    frames, rays = serial_host[size]
    assert np.array_equal(bits(read_pfm(str(pfm))), bits(np.ascontiguousarray(frames[-1][..., :3])))
    assert stats["rays"] == rays
