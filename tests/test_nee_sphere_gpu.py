"""The sphere sample of next-event estimation in the tile kernels (RTPT_FLAG_EXT_NEE_SPHERE; csrc/light_sample.hpp states the
rules): the device function against its numpy restatement bit for bit, whole frames against the walker of tests/nee_sphere.py
(held on the CPU by tests/test_nee_sphere_cpu.py) — IMAGE, HIT_ID and the ray count bit for bit — alone and together with
RTPT_FLAG_EXT_NEE, demodulation, the identities, the launches a sampling frame does not take, and the hosts.  Every test but
test_flag_off_is_the_existing_walker fails on a library without the feature."""
import gc
import json
import os
import subprocess

import numpy as np
import pytest

import dielectric_scenes as DS
import filter_planes as FP
import nee_paths as NP
import nee_scenes as N
import nee_sphere as NS
import path_walker as WK
import test_demodulate_gpu as D
import test_pathtrace_scenes_gpu as T
from conftest import bits
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
W0, H0 = N.SIZES[0]
W1, H1 = N.SIZES[1]
FORCE_BVH, NO_COMPACTION, SINGLE_LAUNCH, UNFUSED, DEMODULATE, NEE, SPHERE = 0x2, 0x8, 0x200, 0x400, 0x8000, 0x10000, 0x20000
STRIP_ROWS = (5, 21)
NONE = np.zeros(0, U32)

_walked = {}


# ------------------------------------------------------------------------------------------ one frame, both sides
def context(abi, scene, W, H, segments, flags=SPHERE, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def upload(abi, ctx, scene, glass=None):
    ctx.scene_upload(*FP.mesh_of(scene.tris))
    if scene.materials is None:
        return
    if glass:
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, None, glass))
    else:
        ctx.set_materials(scene.tri_material, scene.materials)


def frame(abi, oracle, ctx, scene, W, H, planes=(), frame_no=0):
    out = T.frame_on_gpu(abi, oracle, ctx, scene, W, H, frame_no)
    for p in planes:
        out[p] = ctx.readback(getattr(abi, "PLANE_" + p))
    return out


def walked(oracle, scene, W, H, segments, rec, lights, sphere=True, spp=1, frame_no=0):
    """the walker's frame, computed once and left unchanged"""
    key = (scene.name, scene.form, W, H, segments, spp, len(lights), sphere, frame_no)
    if key not in _walked:
        r = WK.walk(oracle, scene, W, H, segments, rec, lights, sphere, frame=frame_no, spp=spp)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _walked[key] = r
    return _walked[key]


def same_frame(got, want, tag, rows=None):
    y0, y1 = rows or (0, len(want["IMAGE"]))
    same_bits(got["HIT_ID"], want["HIT_ID"][y0:y1], tag + ("HIT_ID",))
    same_bits(got["IMAGE"], want["IMAGE"][y0:y1], tag + ("IMAGE",))


def lit_room(form="small"):
    scene, glass = NS.glass_room_lit(form)
    return scene, glass, DS.records(scene, None, glass)


# ------------------------------------------------------------------------------------------ 1. the device function
def test_sphere_sample_equals_the_restatement(hip_lib, oracle):
    """rtpt_selftest_sphere_sample, one case per lane, against nee_sphere.sphere32 bit for bit — wd, g, taken and valid — on 4,096
    seeded cases and on the hostile ones: x at the centre, d2 == r2 and one ulp to either side, x inside, w = (0, 0, +-1) and
    w.z = -0, u_c at 0 and 1 - 2^-24, u_p at 0 and next to 1, nf perpendicular to w, LIGHT_FAR, the radii of
    pathtrace_scenes.PLACEMENTS, q subnormal"""
    abi = hip_lib
    cases = np.concatenate([NS.hostile_cases(), NS.seeded_cases()])
    with abi.Context(T._config(abi, N.receiver(), 64, 12, 1, 1, 0)) as ctx:
        got = ctx.selftest_sphere_sample(cases)
    want = NS.sphere32(oracle, cases)
    same_bits(got[:, 4].view(F32), want[:, 4].view(F32), ("sphere_sample", "taken"))
    same_bits(got[:, 5].view(F32), want[:, 5].view(F32), ("sphere_sample", "valid"))
    same_bits(got[:, 0:3].view(F32), want[:, 0:3].view(F32), ("sphere_sample", "wd"))
    same_bits(got[:, 3].view(F32), want[:, 3].view(F32), ("sphere_sample", "g"))
    assert (want[:, 4].view(F32) == 0).sum() == 4 and (want[:, 5].view(F32) != 0).mean() > 0.9


# ------------------------------------------------------------------------------------------ 2. whole frames against the walker
@pytest.mark.parametrize("flags", [SPHERE, SPHERE | NEE], ids=["sphere", "both"])
@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
@pytest.mark.parametrize("segments", [2, 5])
def test_receiver_equals_the_walker(hip_lib, oracle, segments, vflags, flags):
    """the receiver under the near sphere, pixel_jitter 0, at 64 x 48 and 70 x 10: every pixel that meets the receiver samples the
    sphere at its first hit.  With both flags the trapezoid lamp is sampled at the same hits: both bits are live, and the sphere's
    gain goes into R before the triangle's"""
    abi = hip_lib
    scene = NS.receiver_near()
    rec = DS.records(scene)
    lights = NP.light_list(scene) if flags & NEE else NONE
    for W, H in (N.SIZES[0], N.SIZES[1]):
        want = walked(oracle, scene, W, H, segments, rec, lights)
        assert want["sphere_valid"] > 0.9 * want["sphere_samples"] > 0 and (want["samples"] > 0) == bool(flags & NEE)
        if segments > 2:
            assert want["sphere_dropped"] > 0, "paths meet the sphere they sampled"
        with context(abi, scene, W, H, segments, flags | vflags) as ctx:
            upload(abi, ctx, scene)
            got = frame(abi, oracle, ctx, scene, W, H)
        same_frame(got, want, ("receiver_near", W, H, segments, vflags, flags))
        assert got["rays"] == want["rays"], ("receiver_near", W, H, segments, vflags, flags)


@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
def test_sphere_through_the_floor(hip_lib, oracle, vflags):
    """the light's centre 0.1 above the receiver's plane, radius 0.2: every cone from the plane is cut by the horizon, so valid and
    invalid samples both occur, from points down to the sphere's rim.  (A path never lands inside the sphere — the ray that would
    take it there meets the light first — so a sample that is not taken is the device function's test, not a frame's.)"""
    abi = hip_lib
    scene = NS.receiver_low()
    rec = DS.records(scene)
    for segments in (2, 5):
        want = walked(oracle, scene, W0, H0, segments, rec, NONE)
        assert want["sphere_samples"] == want["sphere_taken"] > want["sphere_valid"] > 0.25 * want["sphere_samples"], want
        with context(abi, scene, W0, H0, segments, SPHERE | vflags) as ctx:
            upload(abi, ctx, scene)
            got = frame(abi, oracle, ctx, scene, W0, H0)
        same_frame(got, want, ("receiver_low", segments, vflags))
        assert got["rays"] == want["rays"], ("receiver_low", segments, vflags)


@pytest.mark.parametrize("form,base", [("small", 0), ("pairs", 0), ("small", FORCE_BVH)], ids=["small", "pairs", "force_bvh"])
def test_glass_room_equals_the_walker(hip_lib, oracle, form, base):
    """the glass room with the light inside it, 9 segments: diffuse, dielectric and emissive hits, so the sphere bit is set and
    cleared along a path, and a sphere seen through the glass behind a diffuse hit counts.  The default schedule,
    RTPT_FLAG_NO_PATH_COMPACTION, the unfused launch, RTPT_FLAG_SINGLE_LAUNCH_PATHS, both flags together, and a strip context with
    row_begin 5"""
    abi = hip_lib
    scene, glass, rec = lit_room(form)
    want = walked(oracle, scene, W0, H0, 9, rec, NONE)
    assert want["sphere_valid"] > 0 and want["sphere_dropped"] > 0 and want["sphere_kept"] > 0, want
    for sid, flags in (("default", 0), ("no_compaction", NO_COMPACTION), ("unfused", UNFUSED), ("single_launch", SINGLE_LAUNCH)):
        with context(abi, scene, W0, H0, 9, SPHERE | base | flags) as ctx:
            upload(abi, ctx, scene, glass)
            got = frame(abi, oracle, ctx, scene, W0, H0)
        same_frame(got, want, (form, base, sid))
        assert got["rays"] == want["rays"], (form, base, sid)
    with context(abi, scene, W0, H0, 9, SPHERE | base, rows=STRIP_ROWS) as ctx:
        upload(abi, ctx, scene, glass)
        strip = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(strip, want, (form, base, "strip"), STRIP_ROWS)
    lights = NP.light_list(scene, 1, rec)
    both = walked(oracle, scene, W0, H0, 9, rec, lights)
    assert both["lit"] > 0 and both["sphere_valid"] > 0
    with context(abi, scene, W0, H0, 9, SPHERE | NEE | base) as ctx:
        upload(abi, ctx, scene, glass)
        got = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(got, both, (form, base, "both flags"))
    assert got["rays"] == both["rays"], (form, base, "both flags")


@pytest.mark.parametrize("form,base", [("small", 0), ("small", FORCE_BVH)], ids=["small", "force_bvh"])
def test_glass_room_second_shape_and_samples(hip_lib, oracle, form, base):
    """70 x 10 (partial tiles in x and y) with one, two and three samples per pixel: R restarts with every sample, both bits are
    clear on every primary ray, and a path's last segment moves the stream by its two draws only"""
    abi = hip_lib
    scene, glass, rec = lit_room(form)
    for segments, spp in ((9, 1), (2, 2), (5, 3)):
        want = walked(oracle, scene, W1, H1, segments, rec, NONE, spp=spp)
        with context(abi, scene, W1, H1, segments, SPHERE | base, spp) as ctx:
            upload(abi, ctx, scene, glass)
            got = frame(abi, oracle, ctx, scene, W1, H1)
        same_frame(got, want, (form, base, segments, spp))
        assert got["rays"] == want["rays"], (form, base, segments, spp)


@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
def test_three_ends_without_materials(hip_lib, oracle, vflags):
    """pathtrace_scenes.three_ends, which has a near light, without a material table: the sampling kernels run without a list and
    without records, on the reference's normal-keyed colours"""
    abi = hip_lib
    scene = NS.three_ends_plain()
    rec = NS.normal_keyed_records(oracle, scene)
    want = walked(oracle, scene, W0, H0, 5, rec, NONE)
    assert want["sphere_valid"] > 0 and want["sphere_dropped"] > 0
    with context(abi, scene, W0, H0, 5, SPHERE | vflags) as ctx:
        upload(abi, ctx, scene)
        got = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(got, want, ("three_ends_plain", vflags))
    assert got["rays"] == want["rays"]


def test_light_far(hip_lib, oracle):
    """the glass room with its light left at pathtrace_scenes.LIGHT_FAR, outside the room (the reference's light is never
    occluded): q = 1.6e-9, k = q / 2 without cancellation; the floor and two walls face it, the others do not"""
    abi = hip_lib
    scene, glass = DS.glass_room("small")
    rec = DS.records(scene, None, glass)
    want = walked(oracle, scene, W0, H0, 5, rec, NONE)
    assert want["sphere_taken"] == want["sphere_samples"] > want["sphere_valid"] > 0.1 * want["sphere_samples"], want
    off = WK.walk(oracle, scene, W0, H0, 5, rec)
    assert not np.array_equal(bits(off["IMAGE"]), bits(want["IMAGE"]))
    with context(abi, scene, W0, H0, 5) as ctx:
        upload(abi, ctx, scene, glass)
        got = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(got, want, ("light_far",))
    assert got["rays"] == want["rays"]


def test_two_frames_with_a_moving_light(hip_lib, oracle):
    """one context, two frames, lightPos moved between them: the sample reads the frame's own light"""
    abi = hip_lib
    first, second = NS.receiver_near(), NS.receiver_moved()
    rec = DS.records(first)
    with context(abi, first, W0, H0, 3) as ctx:
        upload(abi, ctx, first)
        for no, scene in enumerate((first, second)):
            want = walked(oracle, scene, W0, H0, 3, rec, NONE, frame_no=no)
            got = frame(abi, oracle, ctx, scene, W0, H0, frame_no=no)
            same_frame(got, want, ("moving light", no))
            assert got["rays"] == want["rays"], no
    a, b = walked(oracle, first, W0, H0, 3, rec, NONE), walked(oracle, second, W0, H0, 3, rec, NONE, frame_no=1)
    assert not np.array_equal(bits(a["IMAGE"]), bits(b["IMAGE"]))


# ------------------------------------------------------------------------------------------ 3. demodulated
def test_sphere_trace_factorises(hip_lib, oracle):
    """RTPT_FLAG_EXT_DEMODULATE with the sphere sample on the lit glass room, 4 segments: same HIT_ID and ray count, and IMAGE x
    ALBEDO against the undemodulated frame within test_demodulate_gpu's bar (segments + 2) 2^-23 |value| — the gain of segment 0
    is illumination"""
    abi = hip_lib
    scene, glass, rec = lit_room("small")
    seg = 4
    out = {}
    for on in (True, False):
        with context(abi, scene, W0, H0, seg, SPHERE | (DEMODULATE if on else 0)) as ctx:
            upload(abi, ctx, scene, glass)
            out[on] = frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",) if on else ())
    a, b = out[True], out[False]
    same_bits(a["HIT_ID"], b["HIT_ID"], ("HIT_ID",))
    same_bits(b["IMAGE"], walked(oracle, scene, W0, H0, seg, rec, NONE)["IMAGE"], ("the plain trace is the walker's",))
    assert a["rays"] == b["rays"]
    alb, on_img, off_img = a["ALBEDO"][..., :3], a["IMAGE"][..., :3], b["IMAGE"][..., :3]
    ended = (alb == 1).all(-1)
    same_bits(on_img[ended], off_img[ended], ("ended at the first query",))
    went_on = ~ended
    prod = (on_img * alb).astype(F32)
    err = np.abs(prod.astype(np.float64) - off_img.astype(np.float64))
    bound = (seg + 2) * 2.0 ** -23 * np.abs(off_img.astype(np.float64))
    print(f"sphere NEE demodulated: max err / bound = {np.max(err[went_on] / np.maximum(bound[went_on], 1e-300)):.3f}")
    assert went_on.sum() > 1000 and (err[went_on] <= bound[went_on]).all()


# ------------------------------------------------------------------------------------------ 4. identities
def test_one_segment_with_the_flag_is_flag_off(hip_lib, oracle):
    """max_segments = 1: the only segment is the last, no sample is taken — frames and ray counts of a context without the flag,
    with one and with two samples per pixel"""
    abi = hip_lib
    scene, glass, rec = lit_room("small")
    for spp in (1, 2):
        frames = []
        for flags in (0, SPHERE, SPHERE | NEE):
            with context(abi, scene, W0, H0, 1, flags, spp) as ctx:
                upload(abi, ctx, scene, glass)
                frames.append(frame(abi, oracle, ctx, scene, W0, H0))
        for f in frames[1:]:
            same_frame(f, frames[0], ("one segment", spp))
            assert f["rays"] == frames[0]["rays"]


def test_flag_off_is_the_existing_walker(hip_lib, oracle):
    """without the flag the lit glass room is the walker's frame without lights (this one passes without the feature too)"""
    abi = hip_lib
    scene, glass, rec = lit_room("small")
    want = WK.walk(oracle, scene, W0, H0, 9, rec)
    with context(abi, scene, W0, H0, 9, flags=0) as ctx:
        upload(abi, ctx, scene, glass)
        got = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(got, want, ("flag off",))
    assert got["rays"] == want["rays"]


# ------------------------------------------------------------------------------------------ 5. launches not taken
def test_a_sphere_sampling_launch_takes_neither_queues_nor_the_final_pass(hip_lib, oracle):
    """9 segments on the lit glass room: a context without the flag allocates the hand-over queues of the split launch, one with it
    does not (rtpt_debug_live_device_bytes); and a host loop with the flag never takes a deferred final pass into its tracing
    launch (rtpt_debug_defer_info), where the same loop without the flag does"""
    abi = hip_lib
    gc.collect()
    scene, glass, rec = lit_room("small")
    held = {}
    for flags in (0, SPHERE):
        before = abi.live_device_bytes()
        with context(abi, scene, W0, H0, 9, flags) as ctx:
            upload(abi, ctx, scene, glass)
            frame(abi, oracle, ctx, scene, W0, H0)
            held[flags] = abi.live_device_bytes() - before
    queue_bytes = ((W0 + 63) // 64) * ((H0 + 3) // 4) * 256 * 48
    assert held[0] - held[SPHERE] >= queue_bytes, held
    mesh = abi.load_obj(D.SCENE)                     # test_final_defer_gpu's resting frames: the Cornell box, no materials
    taken = {}
    for flags in (0, SPHERE):
        app = D.make(abi, (200, 83), flags, 4, mesh, None)
        for _ in range(8):
            app.drawScene(())
        info = app.backend.ctx.defer_info()
        taken[flags] = info["launched_in_trace"]
        assert info["recorded"] >= 4 and info["recorded"] - info["launched_in_trace"] - info["launched_alone"] <= 1, info
        app.backend.close()
    assert taken[SPHERE] == 0 and taken[0] >= 2, taken


# ------------------------------------------------------------------------------------------ 6. hosts
KEYS = ["", "E", "J"]


def host_frames(size, in_flight=1, **kw):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    app = make_app(size[0], size[1], max_segments=5, iterations=5, frames_in_flight=in_flight, **kw)
    frames = []
    for k in KEYS:
        app.drawScene(tuple(k))
        frames.append(app.backend.final_image_rows(0, size[1]).copy())
    backends = getattr(app.backend, "be", [app.backend])
    rays = sum(b.ctx.raycount() for b in backends)
    app.backend.close()
    return frames, rays


def test_hosts_sample_the_sphere(hip_lib, tmp_path):
    """make_app(nee_sphere=True) on the default scene (the Cornell box, no materials): the frames differ from the flag-off host's,
    two frames in flight render the same frames, flags=FLAG_EXT_NEE_SPHERE is the same switch, and rtpt_app --nee-sphere dumps the
    last frame bit for bit with the same ray count, as one context and as two strips"""
    abi = hip_lib
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    size = N.SIZES[0]
    on, rays_on = host_frames(size, nee_sphere=True)
    off, rays_off = host_frames(size)
    assert rays_on > 0 and rays_off > 0 and not np.array_equal(bits(on[-1]), bits(off[-1]))
    two, rays_two = host_frames(size, in_flight=2, nee_sphere=True)
    assert rays_two == rays_on
    for f in range(len(KEYS)):
        assert np.array_equal(bits(two[f]), bits(on[f])), f
    flag, rays_flag = host_frames(size, flags=abi.FLAG_EXT_NEE_SPHERE)
    assert rays_flag == rays_on and np.array_equal(bits(flag[-1]), bits(on[-1]))
    app_binary = os.path.join(D.PKG, "rtpt_app")
    assert os.path.exists(app_binary), "build() leaves rtpt_app next to the package"
    for extra in ([], ["--ranks", "2"]):
        pfm = tmp_path / "out.pfm"
        cmd = [app_binary, "--width", str(size[0]), "--height", str(size[1]), "--segments", "5", "--iterations", "5", "--frames", str(len(KEYS)),
               "--script", ",".join(KEYS), "--dump", str(pfm), "--nee-sphere"] + extra
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        stats = json.loads(out.stdout.strip().splitlines()[-1])
        assert np.array_equal(bits(read_pfm(str(pfm))), bits(np.ascontiguousarray(on[-1][..., :3]))), extra
        assert stats["rays"] == rays_on, extra
    help_text = subprocess.run([app_binary, "--help"], capture_output=True, text=True)
    assert "--nee-sphere" in help_text.stdout + help_text.stderr
