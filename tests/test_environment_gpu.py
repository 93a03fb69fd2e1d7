"""The environment map (rtpt_set_environment) on the device against tests/environment_maps.py: the lookup operand by operand, a closed
form, whole frames bit for bit against the walker with its sky seam replaced (IMAGE, HIT_ID, the ray count and, with
RTPT_FLAG_EXT_DEMODULATE, ALBEDO), what must not move, and the hosts.  No tolerance appears anywhere.  tests/test_environment_cpu.py
holds the restatement to the double-precision decode first.

Frames are normal_paths' 70 x 10 (one full tile column, a partial one, partial tile rows) on its scenes, which are open towards the
sky: the 40-triangle sphere with its floor and lamp alone (brute force; the camera moved closer so that enough paths leave the scene
behind a bounce), and the three-instance scenes over triangles (uv_sphere, scene mode 1) and over fan pairs (half_cylinder, mode 2).
Maps are at most 64 x 64."""
import json
import os
import subprocess

import numpy as np
import pytest

import dielectric_scenes as DS
import environment_maps as EM
import filter_planes as FP
import gbuffer_scenes as G
import normal_paths as NP
import path_walker as WK
import pathtrace_scenes as P
import shading_scenes as SS
import test_pathtrace_scenes_gpu as T
from conftest import bits
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = NP.SHAPE
NO_PATH_COMPACTION = 0x8
SMALL_CAM = (0.05, 0.0, 1.2)


def env_a():
    return EM.make_env(EM.distinct_map(8), 0, EM.rotation(), EM.SCALE)


def env_b():
    return EM.make_env(EM.distinct_map(64), EM.NEAREST)


def set_env(ctx, env):
    ctx.set_environment(env.texels, env.flags, env.rotation, env.scale)


# ------------------------------------------------------------------------------------------ 1. the lookup on the device
def test_lookup_on_the_device(hip_lib, oracle):
    """rtpt_selftest_environment over every generated direction x every generated map, bilinear and nearest, with and without a
    rotation and a scale: the restatement's bits, no case left out"""
    abi = hip_lib
    d = EM.hostile_directions()
    with abi.Context(abi.config_default(64, 16)) as ctx:
        with pytest.raises(abi.RtptError):
            ctx.selftest_environment(d[:4])                                   # no environment yet
        for tag, env in EM.envs():
            set_env(ctx, env)
            got, want = ctx.selftest_environment(d), EM.color32(oracle, env, d)
            same_bits(got, want, ("rtpt_selftest_environment",) + tag)
            assert (want != 0).any(1).sum() > 1500 and (want == 0).all(1).sum() >= 15, tag


# ------------------------------------------------------------------------------------------ scenes, references, frames
def case_of(oracle, name):
    """(Case, Normals) of a scene name: normal_paths' two, or "small": its base mesh alone with the camera moved closer"""
    if name != "small":
        return NP.case(oracle, name)
    c, nrm = NP.small_case(oracle)
    return c._replace(sh=c.sh._replace(scene=c.sh.scene._replace(cam=SMALL_CAM))), nrm


_ref = {}


def reference(oracle, env, name, spec, tex, demod, normals, spp, segments, rows=None, frame=0, hits=False):
    key = (None if env is None else (env.texels.shape[0], env.flags), name, spec, tex, demod, normals, spp, segments, rows, frame)
    if key not in _ref:
        c, nrm = case_of(oracle, name)
        table = [] if hits else None
        with EM.environment(oracle, env) as samples:
            r = WK.walk(oracle, c.sh.scene, W, H, segments, normals=nrm if normals else None, n_base=len(nrm.tri_smooth), spp=spp,
                        tex=WK.textures(c.sh, tex), demod=demod, rows=rows, frame=frame, hits=table, **NP.setup(oracle, c, spec))
        r["env_shares"] = EM.shares(samples, W * ((rows[1] - rows[0]) if rows else H))
        if hits:
            r["env_behind"] = EM.ended_behind(samples, WK.hit_table(table))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ref[key] = r
    return _ref[key]


def upload(abi, ctx, c, name, spec, tex, normals):
    sh = c.sh
    if name == "small":
        ctx.scene_upload(sh.mesh[0], sh.mesh[1])
    else:
        ctx.scene_upload(sh.mesh[0], sh.mesh[1], NP.xforms())
    ctx.set_materials_ext(sh.scene.tri_material, abi.materials_ext(sh.scene.materials, sh.spec if spec >= 1 else None, c.glass if spec >= 2 else None))
    if tex:
        ctx.set_textures(sh.tri_uv, sh.tri_texture, *SS.atlas(sh, tex))
    if normals:
        ctx.set_normals(c.tri_normals, c.tri_smooth)


def context(abi, c, segments, flags=0, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, c.sh.scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def frame(abi, oracle, ctx, c, demod, frame_no=0):
    """K0, K1, K2 in the reference's order; IMAGE, HIT_ID, the ray count, ALBEDO"""
    sc = c.sh.scene
    pc = G.fill_push_constants(abi.PushConstants(), P.push_constants(sc), frame_no)
    ctx.reset_counters()
    ctx.gbuffer(T._ubo(abi, oracle, sc, W, H))
    ctx.temporal_gradient(pc)
    ctx.raytrace(pc)
    got = dict(IMAGE=ctx.readback(abi.PLANE_IMAGE), HIT_ID=ctx.readback(abi.PLANE_HIT_ID), rays=ctx.raycount())
    if demod:
        got["ALBEDO"] = ctx.readback(abi.PLANE_ALBEDO)
    return got


def compare(got, ref, tag, rows=None):
    T.compare(got, ref, rows, tag)
    if "ALBEDO" in got:
        y0, y1 = rows or (0, H)
        same_bits(got["ALBEDO"], ref["ALBEDO"][y0:y1], tag + ("ALBEDO",))


def flags_of(spec, demod, bvh=False):
    return NP.SPEC_FLAGS[spec] | (NP.DEMODULATE if demod else 0) | (NP.FORCE_BVH if bvh else 0)


def _launch_form(monkeypatch, form):
    monkeypatch.delenv("RTPT_PT_WINDOW", raising=False)
    monkeypatch.setenv("RTPT_HOST_REFIT", "0")
    if form == "unfused":
        monkeypatch.setenv("RTPT_NO_TRACE_FUSION", "1")
    else:
        monkeypatch.delenv("RTPT_NO_TRACE_FUSION", raising=False)


# ------------------------------------------------------------------------------------------ 2. the closed form
def test_closed_form_with_nothing_in_front_of_the_camera(hip_lib, oracle):
    """every triangle behind the camera: a pixel is the restatement's colour of its own primary ray, or light_col_first on the light"""
    abi = hip_lib
    c, _ = case_of(oracle, "small")
    sc = c.sh.scene._replace(cam=(0.0, 0.0, -3.0), light=(0.1, 0.15, -6.0), light_radius=0.5)
    c = c._replace(sh=c.sh._replace(scene=sc))
    env = env_a()
    cfg = P.configure(oracle.config_default(W, H), sc, 4, 1)
    _, d = DS.primary_rays(oracle, sc, W, H)
    d = d.reshape(-1, 3)
    o = np.broadcast_to(F32(sc.cam), d.shape)
    lit = DS._contract(oracle, "ray_hits_light", o, d, np.broadcast_to(F32(sc.light), d.shape), np.full((len(d), 1), sc.light_radius, F32)).view(np.uint32)[:, 0] != 0
    light_first = ((F32(P.LIGHT_COLOR) * F32(cfg.light_intensity)).astype(F32) / F32(cfg.first_hit_light_divisor)).astype(F32)
    want = np.where(lit[:, None], light_first[None, :], EM.color32(oracle, env, d)).astype(F32).reshape(H, W, 3)
    assert 0 < lit.sum() < len(lit) // 2
    for bvh in (False, True):
        with context(abi, c, 4, flags_of(0, False, bvh)) as ctx:
            upload(abi, ctx, c, "small", 0, 0, False)
            set_env(ctx, env)
            got = frame(abi, oracle, ctx, c, False)
        assert not got["HIT_ID"].any() and got["rays"] == W * H
        same_bits(got["IMAGE"][..., :3], want, ("closed form", bvh))


# ------------------------------------------------------------------------------------------ 3. frames against the patched walker
# (what the cell is for, scene, SPEC, TEX, DEMOD, normals, forced BVH, launch form, samples per pixel, segments, environment)
CELLS = (
    ("diffuse, brute force", "small", 0, 0, False, False, False, "fused", 1, 4, env_a),
    ("diffuse, forced BVH", "small", 0, 0, False, False, True, "fused", 1, 4, env_a),
    ("mirror, glossy, glass", "uv_sphere", 2, 0, False, False, False, "fused", 1, 5, env_b),
    ("mips and demodulation", "half_cylinder", 1, 2, True, False, False, "unfused", 1, 4, env_a),
    ("NEE, power, MIS, sphere", "uv_sphere", 10, 0, False, False, False, "unfused", 1, 4, env_a),
    ("vertex normals", "half_cylinder", 2, 0, False, True, False, "fused", 1, 6, env_b),
    ("three samples", "small", 0, 0, False, False, False, "fused", 3, 4, env_b),
)


@pytest.mark.parametrize("cell", CELLS, ids=[c[0] for c in CELLS])
def test_frames(hip_lib, oracle, monkeypatch, cell):
    what, name, spec, tex, demod, normals, bvh, form, spp, segments, make = cell
    abi = hip_lib
    _launch_form(monkeypatch, form)
    env = make()
    c, _ = case_of(oracle, name)
    ref = reference(oracle, env, name, spec, tex, demod, normals, spp, segments, hits=spec == 2)
    first, later = ref["env_shares"]
    print(f"{what}: {first:.3f} of the paths end in the environment at segment 0, {later:.3f} at later segments")
    assert first >= 0.1 and later >= 0.1, (what, first, later)          # the frame reads the map, at both kinds of segment
    if spec == 2:
        assert ref["env_behind"] > 0, (what, "no path ends in the environment behind a mirror or through glass")
    with context(abi, c, segments, flags_of(spec, demod, bvh), spp) as ctx:
        upload(abi, ctx, c, name, spec, tex, normals)
        set_env(ctx, env)
        info = ctx.scene_build_info()
        if name != "small":
            assert bool(info["leaf_pairs"]) == (name == "half_cylinder"), cell
        got = frame(abi, oracle, ctx, c, demod)
    compare(got, ref, (what,))
    sky = reference(oracle, None, name, spec, tex, demod, normals, spp, segments)
    assert not WK.same_image(got, sky) and np.array_equal(ref["HIT_ID"], sky["HIT_ID"]) and ref["rays"] == sky["rays"]
    assert np.array_equal(ref["seq_n"], sky["seq_n"])


# ------------------------------------------------------------------------------------------ 4. nothing else moves
def test_nothing_else_moves(hip_lib, oracle, monkeypatch):
    """HIT_ID and RAYCOUNT with the environment are those without; after rtpt_set_environment(NULL) the frames are a never-set
    context's; the map is 16 n^2 bytes of device memory, gone after the drop and after rtpt_destroy; it survives an upload, the
    scene setters, a rebuild and a resize; refusals leave the previous map in place"""
    abi = hip_lib
    _launch_form(monkeypatch, "fused")
    name, spec, tex, demod, seg = "uv_sphere", 2, 1, True, 4
    c, _ = case_of(oracle, name)
    env = env_a()
    ref = reference(oracle, env, name, spec, tex, demod, False, 1, seg)
    before_all = abi.live_device_bytes()
    with context(abi, c, seg, flags_of(spec, demod)) as never, context(abi, c, seg, flags_of(spec, demod)) as ctx:
        upload(abi, never, c, name, spec, tex, False)
        base = abi.live_device_bytes()
        set_env(ctx, env)                                                     # before any scene: the call needs none
        assert abi.live_device_bytes() - base == 16 * 8 * 8
        set_env(ctx, env_b())
        assert abi.live_device_bytes() - base == 16 * 64 * 64, "the replaced map is released"
        set_env(ctx, env)
        upload(abi, ctx, c, name, spec, tex, False)                          # the upload and every setter keep it
        plain = frame(abi, oracle, never, c, demod)
        got = frame(abi, oracle, ctx, c, demod)
        held = abi.live_device_bytes()
        compare(got, ref, ("kept through the upload",))
        assert np.array_equal(got["HIT_ID"], plain["HIT_ID"]) and got["rays"] == plain["rays"]
        assert not np.array_equal(bits(got["IMAGE"]), bits(plain["IMAGE"]))
        # refusals: the previous environment stays
        big = np.zeros((1, 1, 4), F32)
        for bad in (dict(texels=F32(np.full((2, 2, 4), np.nan))), dict(texels=F32(np.full((2, 2, 4), np.inf))),
                    dict(texels=big, flags=0x2), dict(texels=big, flags=0x10), dict(texels=big, rotation=F32([[np.nan, 0, 0], [0, 1, 0], [0, 0, 1]])),
                    dict(texels=big, scale=F32([1, np.inf, 1]))):
            with pytest.raises(abi.RtptError) as e:
                ctx.set_environment(**bad)
            assert e.value.code == abi.RTPT_E_INVALID, bad
        one = np.zeros(4, F32)
        assert ctx._lib.rtpt_set_environment(ctx._h, abi._ptr(one), 4097, 0, None, None) == abi.RTPT_E_INVALID   # refused before a texel is read
        assert abi.live_device_bytes() == held
        ctx.end_frame()
        never.end_frame()
        ctx.scene_rebuild()
        ctx.resize(W, H)
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        compare(frame(abi, oracle, ctx, c, demod, 1), reference(oracle, env, name, spec, tex, demod, False, 1, seg, frame=1), ("rebuilt and resized",))
        ctx.end_frame()
        ctx.set_environment(None)                                             # the drop
        frame(abi, oracle, never, c, demod, 1)                                # (the never-set context goes through the same calls)
        never.end_frame()
        never.scene_rebuild()
        never.resize(W, H)
        never.enable_debug(abi.DEBUG_HIT_ID)
        after = frame(abi, oracle, ctx, c, demod, 2)
        want = frame(abi, oracle, never, c, demod, 2)
        for k in ("IMAGE", "ALBEDO", "HIT_ID"):
            assert np.array_equal(bits(after[k]), bits(want[k])), ("dropped", k)
        assert after["rays"] == want["rays"]
        with pytest.raises(abi.RtptError):
            ctx.selftest_environment(F32([[0, 1, 0]]))
        set_env(ctx, env_b())
        inside = abi.live_device_bytes()
    assert abi.live_device_bytes() == before_all, "rtpt_destroy releases the map"
    assert inside > before_all
    with context(abi, c, seg, flags_of(spec, demod) | NO_PATH_COMPACTION) as ctx:
        with pytest.raises(abi.RtptError) as e:
            set_env(ctx, env)                                                 # that A/B flag has no environment kernels
        assert e.value.code == abi.RTPT_E_INVALID
        ctx.set_environment(None)                                             # dropping nothing is fine
        upload(abi, ctx, c, name, spec, tex, False)
        compare(frame(abi, oracle, ctx, c, demod), reference(oracle, None, name, spec, tex, demod, False, 1, seg), ("no compaction",))


def _script(hip_lib, when, env, **kw):
    """five resting frames of the Python host; the environment set in front of frame `when` (None: never): per-frame final images,
    frames served from the planes, the ray count"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    app = make_app(96, 64, max_segments=3, iterations=3, **kw)
    frames, served = [], []
    for f in range(5):
        if f == when:
            app.backend.set_environment(env.texels, env.flags, env.rotation, env.scale)
        ctxs = [b.ctx for b in getattr(app.backend, "be", [app.backend])]
        before = sum(x.reuse_info()["frames_skipped"] for x in ctxs)
        app.drawScene(())
        served.append(sum(x.reuse_info()["frames_skipped"] for x in ctxs) - before)
        frames.append(app.backend.final_image_rows(0, 64).copy())
    rays = sum(x.raycount() for x in ctxs)
    app.backend.close()
    return frames, served, rays


def test_setting_an_environment_keeps_frame_reuse(hip_lib, monkeypatch):
    """K0, K1 and the filter read nothing of the map: a resting scene goes on being served from its planes across the call"""
    monkeypatch.setenv("RTPT_NO_FRAME_REUSE", "0")
    monkeypatch.delenv("RTPT_NO_TRACE_FUSION", raising=False)
    _, never, _ = _script(hip_lib, None, None)
    frames, served, _ = _script(hip_lib, 3, env_a())
    assert never == [0, 0, 1, 1, 1] and served == never, (never, served)
    assert not np.array_equal(bits(frames[3]), bits(frames[2]))


# ------------------------------------------------------------------------------------------ 5. the hosts
def test_two_strips_equal_the_whole_frame(hip_lib, oracle, monkeypatch):
    """rows [0, 6) and [6, 10) in two contexts, the second with row_begin > 0, against the walker's full frame"""
    abi = hip_lib
    _launch_form(monkeypatch, "fused")
    name, spec, tex, demod, seg = "uv_sphere", 4, 2, True, 3
    c, _ = case_of(oracle, name)
    env = env_a()
    full = reference(oracle, env, name, spec, tex, demod, False, 1, seg)
    total = 0
    for rows in ((0, 6), (6, 10)):
        counted = reference(oracle, env, name, spec, tex, demod, False, 1, seg, rows=rows)["rays"]
        with context(abi, c, seg, flags_of(spec, demod), rows=rows) as ctx:
            upload(abi, ctx, c, name, spec, tex, False)
            set_env(ctx, env)
            got = frame(abi, oracle, ctx, c, demod)
        compare(got, dict(full, rays=counted), (name, "strip", rows), rows)
        total += counted
    assert total == full["rays"]


def _write_latlong(path, h=16, w=32):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import write_pfm
    rng = np.random.default_rng(17)
    im = (rng.random((h, w, 3)) * 2.0).astype(F32)
    im[3, 5] = 1e4
    write_pfm(str(path), im)


def test_hosts(hip_lib, tmp_path):
    """the project's Cornell asset under a lat-long PFM the test writes: two frames in flight equal the serial Python host, and
    rtpt_app --environment equals it too, through --dump; with and without the environment the frames differ"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import DEFAULT_SCENE, make_app
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    abi = hip_lib
    sky = tmp_path / "sky.pfm"
    _write_latlong(sky)
    Wh, Hh, seg, n_it = 96, 64, 3, 5
    keys = ["", "J", "D"]
    opts = dict(environment=str(sky), environment_size=8, environment_yaw=30.0, environment_scale=1.5)
    out = {}
    for how, kw in (("serial", opts), ("in flight", dict(opts, frames_in_flight=2)), ("sky", {})):
        app = make_app(Wh, Hh, max_segments=seg, iterations=n_it, **kw)
        for k in keys:
            app.drawScene(tuple(k))
        be = app.backend
        out[how] = (be.final_image_rows(0, Hh).copy(), sum(b.ctx.raycount() for b in getattr(be, "be", [be])))
        be.close()
    assert np.array_equal(bits(out["serial"][0]), bits(out["in flight"][0])) and out["serial"][1] == out["in flight"][1]
    assert not np.array_equal(bits(out["serial"][0]), bits(out["sky"][0])) and out["serial"][1] == out["sky"][1]
    binary = os.path.join(os.path.dirname(abi.LIB_PATH), "rtpt_app")
    assert os.path.exists(binary), "the C++ host is not built"
    pfm = tmp_path / "out.pfm"
    run = subprocess.run([binary, "--scene", DEFAULT_SCENE, "--environment", str(sky), "--environment-size", "8", "--environment-yaw", "30",
                          "--environment-scale", "1.5", "--width", str(Wh), "--height", str(Hh), "--segments", str(seg), "--iterations", str(n_it),
                          "--frames", str(len(keys)), "--script", ",".join(keys), "--dump", str(pfm)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    stats = json.loads(run.stdout.strip().splitlines()[-1])
    got = np.ascontiguousarray(read_pfm(str(pfm)), F32)
    assert np.array_equal(bits(got), bits(np.ascontiguousarray(out["serial"][0][..., :3])))
    assert stats["rays"] == out["serial"][1]
