"""Multiple importance sampling of next-event estimation on the device (RTPT_FLAG_EXT_NEE_MIS; csrc/light_sample.hpp states the
rules): the weights and the search against their numpy restatement bit for bit, whole frames against the walker of
tests/nee_mis.py (held on the CPU by tests/test_nee_mis_cpu.py) — IMAGE, HIT_ID and the ray count bit for bit — the other
schedules, the identities, the lifetime of the hit emitter's entry on the posed scene, and the hosts.  Every test but the
identities fails on a library without the feature: the symbols and the flag's kernels do not exist there."""
import gc
import json
import os
import subprocess

import numpy as np
import pytest

import dielectric_scenes as DS
import filter_planes as FP
import gbuffer_scenes as G
import nee_mis as M
import nee_paths as NP
import nee_power as PW
import nee_scenes as N
import path_walker as WK
import pathtrace_scenes as P
import refit_moves as RM
import test_demodulate_gpu as D
import test_nee_paths_gpu as TN
import test_pathtrace_scenes_gpu as T
from conftest import bits
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
W0, H0 = N.SIZES[0]
W1, H1 = N.SIZES[1]
FORCE_BVH, NO_COMPACTION, UNFUSED, DEMODULATE = 0x2, 0x8, 0x400, 0x8000
NEE, SPHERE, POWER, MIS = 0x10000, 0x20000, 0x40000, 0x80000
STRIP_ROWS = (5, 21)

_walked = {}


# ------------------------------------------------------------------------------------------ one frame, both sides
def context(abi, scene, W, H, segments, flags=NEE | MIS, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def frame(abi, oracle, ctx, scene, W, H, planes=(), frame_no=0):
    out = T.frame_on_gpu(abi, oracle, ctx, scene, W, H, frame_no)
    for p in planes:
        out[p] = ctx.readback(getattr(abi, "PLANE_" + p))
    return out


def walked(oracle, key, scene, W, H, segments, rec, lights, flags=NEE | MIS, spp=1, texture=None):
    """the walker's frame under `flags`, computed once and left unchanged"""
    mis, power, sphere = bool(flags & MIS), bool(flags & POWER), bool(flags & SPHERE)
    key = (key, W, H, segments, spp, len(lights), mis, power, sphere, texture is not None)
    if key not in _walked:
        r = WK.walk(oracle, scene, W, H, segments, rec, lights, mis=mis, power=power, sphere=sphere, spp=spp,
                    tex=None if texture is None else WK.Tex(*texture, None))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _walked[key] = r
    return _walked[key]


def same_frame(got, want, tag, rows=None):
    y0, y1 = rows or (0, len(want["IMAGE"]))
    same_bits(got["HIT_ID"], want["HIT_ID"][y0:y1], tag + ("HIT_ID",))
    same_bits(got["IMAGE"], want["IMAGE"][y0:y1], tag + ("IMAGE",))


def scenes():
    """name -> (scene, glass, records, light list)"""
    out = {}
    for sc in (M.wall_lamp(), NP.two_lamps(), NP.occluder(), PW.unequal_lamps()):
        out[sc.name] = (sc, None, DS.records(sc), NP.light_list(sc))
    room, glass, rec = PW.glass_room_two_lamps()
    out[room.name] = (room, glass, rec, NP.light_list(room, 1, rec))
    return out


# ------------------------------------------------------------------------------------------ 1. the self tests
def test_mis_weight_equals_the_restatement(hip_lib, oracle):
    """rtpt_selftest_mis_weight against nee_mis.mis_weight32 bit for bit — g_hit, wb(g_hit), g_hit * m(g_hit) — on the hostile rows
    (cl = 0, cb = 0, q_i = 0 as inv_p = inf, NaN, r2 = 0 and subnormal, a degenerate emitter, squares that overflow) and on 4,096
    seeded hits; and on given g through a unit emitter: the hostile weights 0, subnormal, 1, 2^63, 2^64 and above, +inf, NaN"""
    abi = hip_lib
    unit = (F32([0, 0, 0]), F32([1, 0, 0]), F32([0, 0, 1]))
    g = np.concatenate([M.G_HOSTILE, M.seeded_g(256)])
    # cb = g, cl = 1, a2 = 1, inv_p = 2 pi, r2 = 1: g_hit = ((g * 1) * (1 * 2 pi)) / (2 pi * 1), g to a rounding
    by_g = M.cases_of(*unit, np.broadcast_to(F32([0.25, 1, 0.25]), (len(g), 3)), F32([0, -1, 0]), 0.25, 0.25, g, N.K2PI)
    with abi.Context(T._config(abi, N.receiver(), 64, 12, 1, 1, 0)) as ctx:
        for name, cases in (("hostile", M.hostile_cases()), ("seeded", M.seeded_cases()), ("by_g", by_g)):
            got = ctx.selftest_mis_weight(cases)
            want = M.mis_weight32(oracle, cases)
            assert got.shape == want.shape == (len(cases), 3)
            same_bits(got, want, (name,))
    with np.errstate(all="ignore"):
        assert ((want[:, 1] >= 0) & (want[:, 1] <= 1)).all() and not (want[:, 2] > 0.5).any()
    assert want[13, 1] == 1 and want[14, 1] == 1, "wb(inf) = wb(NaN) = 1"


@pytest.mark.parametrize("n", M.FIND_SIZES)
def test_light_find_equals_the_restatement(hip_lib, n):
    """rtpt_selftest_light_find against nee_mis.find on lists of 1, 2, 3, 1,000 and 2^20 + 1,025 ids: both ends, every entry, every
    gap, ids below, above and between; n for an id that is not in the list"""
    abi = hip_lib
    ids, q = M.find_case(n)
    with abi.Context(T._config(abi, N.receiver(), 64, 12, 1, 1, 0)) as ctx:
        got = ctx.selftest_light_find(ids, q)
        empty = ctx.selftest_light_find(np.zeros(0, U32), q[:7])
    want = M.find(ids, q)
    assert got.dtype == U32 and np.array_equal(got, want), np.flatnonzero(got != want)[:4]
    assert (want == n).sum() >= 7 and (want < n).sum() >= min(n, 1000)
    assert (empty == 0).all()


# ------------------------------------------------------------------------------------------ 2. whole frames against the walker
@pytest.mark.parametrize("flags", [NEE | MIS, NEE | MIS | POWER, NEE | MIS | SPHERE, NEE | MIS | POWER | SPHERE],
                         ids=["0x90000", "0xD0000", "0xB0000", "0xF0000"])
@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
@pytest.mark.parametrize("name", ["nee_wall_lamp", "nee_two_lamps", "nee_occluder", "nee_unequal_lamps", "glass_room_two_lamps"])
def test_frames_equal_the_walker(hip_lib, oracle, name, vflags, flags):
    """IMAGE, HIT_ID and the ray count against path_walker.walk, at 2 segments and at 5 (the glass room: 9), by brute force and with
    RTPT_FLAG_FORCE_BVH, with flags 0x90000, 0xD0000, 0xB0000 and 0xF0000; weighted terminals occur, and the frame is not the one
    without the MIS bit"""
    abi = hip_lib
    scene, glass, rec, lights = scenes()[name]
    for segments in (2, 9 if glass else 5):
        want = walked(oracle, name, scene, W0, H0, segments, rec, lights, flags)
        plain = walked(oracle, name, scene, W0, H0, segments, rec, lights, flags & ~MIS)
        assert want["weighted"] > 0 and want["lit"] > 0 and not np.array_equal(bits(want["IMAGE"]), bits(plain["IMAGE"]))
        if glass and segments == 9:
            assert want["kept"] > 0, "behind a mirror or glass hit the bit is clear"
        with context(abi, scene, W0, H0, segments, flags | vflags) as ctx:
            TN.upload(abi, ctx, scene, glass)
            got = frame(abi, oracle, ctx, scene, W0, H0)
        same_frame(got, want, (name, segments, vflags, hex(flags)))
        assert got["rays"] == want["rays"] == plain["rays"], (name, segments, vflags, hex(flags))
        assert not np.array_equal(bits(got["IMAGE"]), bits(plain["IMAGE"]))


def test_other_schedules_shapes_and_samples(hip_lib, oracle):
    """the glass room with its second lamp: RTPT_FLAG_NO_PATH_COMPACTION (cb stays in its register), the unfused launch, the
    unfused launch on the BVH, a strip context with row_begin 5, and one, two and three samples per pixel at 70 x 10 (partial
    tiles in x and y; R restarts with every sample and the primary ray starts with the bit clear)"""
    abi = hip_lib
    scene, glass, rec, lights = scenes()["glass_room_two_lamps"]
    flags = NEE | MIS | POWER
    want = walked(oracle, scene.name, scene, W0, H0, 9, rec, lights, flags)
    for sid, extra in (("no_compaction", NO_COMPACTION), ("no_compaction_bvh", NO_COMPACTION | FORCE_BVH), ("unfused", UNFUSED),
                       ("unfused_bvh", UNFUSED | FORCE_BVH)):
        with context(abi, scene, W0, H0, 9, flags | extra) as ctx:
            TN.upload(abi, ctx, scene, glass)
            got = frame(abi, oracle, ctx, scene, W0, H0)
        same_frame(got, want, (sid,))
        assert got["rays"] == want["rays"], sid
    with context(abi, scene, W0, H0, 9, flags, rows=STRIP_ROWS) as ctx:
        TN.upload(abi, ctx, scene, glass)
        strip = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(strip, want, ("strip",), STRIP_ROWS)
    for segments, spp, f in ((9, 1, NEE | MIS), (2, 2, NEE | MIS | POWER | SPHERE), (5, 3, NEE | MIS | POWER | FORCE_BVH)):
        want = walked(oracle, scene.name, scene, W1, H1, segments, rec, lights, f, spp=spp)
        assert want["weighted"] > 0
        with context(abi, scene, W1, H1, segments, f, spp) as ctx:
            TN.upload(abi, ctx, scene, glass)
            got = frame(abi, oracle, ctx, scene, W1, H1)
        same_frame(got, want, (segments, spp, hex(f)))
        assert got["rays"] == want["rays"], (segments, spp, hex(f))


def test_demodulated_and_textured(hip_lib, oracle):
    """RTPT_FLAG_EXT_DEMODULATE with MIS on the glass room, 4 segments: same HIT_ID and ray count, and IMAGE x ALBEDO against the
    undemodulated frame within test_demodulate_gpu's bar (segments + 2) 2^-23 |value| (wb and gm are factors like any other: one
    more rounding where a path ends on an emitter, within the bar's two spare ones); and the room with albedo textures without
    mips (TEX = 1) against the walker that samples them.
    Measured on an MI355X: max err / bound 0.187."""
    abi = hip_lib
    scene, glass, rec, lights = scenes()["glass_room_two_lamps"]
    seg = 4
    flags = NEE | MIS | POWER
    out = {}
    for on in (True, False):
        with context(abi, scene, W0, H0, seg, flags | (DEMODULATE if on else 0)) as ctx:
            TN.upload(abi, ctx, scene, glass)
            out[on] = frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",) if on else ())
    a, b = out[True], out[False]
    same_bits(a["HIT_ID"], b["HIT_ID"], ("HIT_ID",))
    same_frame(b, walked(oracle, scene.name, scene, W0, H0, seg, rec, lights, flags), ("the plain trace is the walker's",))
    assert a["rays"] == b["rays"]
    alb, on_img, off_img = a["ALBEDO"][..., :3], a["IMAGE"][..., :3], b["IMAGE"][..., :3]
    ended = (alb == 1).all(-1)
    same_bits(on_img[ended], off_img[ended], ("ended at the first query",))
    went_on = ~ended
    err = np.abs((on_img * alb).astype(F32).astype(np.float64) - off_img.astype(np.float64))
    bound = (seg + 2) * 2.0 ** -23 * np.abs(off_img.astype(np.float64))
    print(f"MIS demodulated: max err / bound = {np.max(err[went_on] / np.maximum(bound[went_on], 1e-300)):.3f}")
    assert went_on.sum() > 1000 and (err[went_on] <= bound[went_on]).all()
    tex = TN.texture_setup(len(scene.tris), False)
    for f in (NEE | MIS, NEE | MIS | POWER | FORCE_BVH):
        want = walked(oracle, "textured", scene, W0, H0, 5, rec, lights, f, texture=tex)
        assert not np.array_equal(bits(want["IMAGE"]), bits(walked(oracle, scene.name, scene, W0, H0, 5, rec, lights, f)["IMAGE"]))
        with context(abi, scene, W0, H0, 5, f) as ctx:
            TN.upload(abi, ctx, scene, glass)
            ctx.set_textures(*tex)
            got = frame(abi, oracle, ctx, scene, W0, H0)
        same_frame(got, want, ("textured", hex(f)))
        assert got["rays"] == want["rays"], ("textured", hex(f))


# ------------------------------------------------------------------------------------------ 3. identities
def test_the_bit_alone_is_ignored(hip_lib, oracle):
    """0x80000 is 0 and 0xA0000 is 0x20000 bit for bit, rays included, by brute force and on the BVH; 0x90000 on a scene without an
    emitter, or without materials, is flag off, 0xB0000 there is 0x20000; 0xC0000 (no NEE bit) is flag off; max_segments = 1 with
    the flag is flag off"""
    abi = hip_lib
    scene, glass, rec, lights = scenes()["glass_room_two_lamps"]
    dark = scene.materials.copy()
    dark[:, 3:] = 0

    def render(flags, materials, seg=9):
        with context(abi, scene, W0, H0, seg, flags) as ctx:
            ctx.scene_upload(*FP.mesh_of(scene.tris))
            if materials is not None:
                ctx.set_materials_ext(scene.tri_material, abi.materials_ext(materials, None, glass))
            return frame(abi, oracle, ctx, scene, W0, H0)

    for base in (0, FORCE_BVH):
        for a, b, materials in ((MIS, 0, scene.materials), (MIS | SPHERE, SPHERE, scene.materials), (MIS | POWER, 0, scene.materials),
                                (NEE | MIS, 0, dark), (NEE | MIS, 0, None), (NEE | MIS | SPHERE, SPHERE, dark),
                                (NEE | MIS | SPHERE, SPHERE, None), (NEE | MIS | POWER, 0, dark)):
            got, want = render(a | base, materials), render(b | base, materials)
            same_frame(got, want, (hex(a), hex(b), base))
            assert got["rays"] == want["rays"], (hex(a), hex(b), base)
        got, want = render(NEE | MIS | POWER | base, scene.materials, 1), render(base, scene.materials, 1)
        same_frame(got, want, ("one segment", base))
        assert got["rays"] == want["rays"]


def test_a_mis_launch_takes_neither_queues_nor_the_final_pass(hip_lib, oracle):
    """9 segments on the glass room: a context without the flags allocates the hand-over queues of the split launch, one with 0x90000
    does not (rtpt_debug_live_device_bytes), and 0x80000 alone allocates what flag off allocates; a host loop with 0x90000 never
    takes a deferred final pass into its tracing launch (rtpt_debug_defer_info), where the same loop without the flags does"""
    abi = hip_lib
    gc.collect()
    scene, glass, rec, lights = scenes()["glass_room_two_lamps"]
    held = {}
    for flags in (0, MIS, NEE | MIS):
        before = abi.live_device_bytes()
        with context(abi, scene, W0, H0, 9, flags) as ctx:
            TN.upload(abi, ctx, scene, glass)
            frame(abi, oracle, ctx, scene, W0, H0)
            held[flags] = abi.live_device_bytes() - before
    queue_bytes = ((W0 + 63) // 64) * ((H0 + 3) // 4) * 256 * 48
    assert held[MIS] == held[0], "the bit alone: every allocation is flag off's"
    assert held[0] - held[NEE | MIS] >= queue_bytes - 4 * len(lights), held
    mesh = abi.load_obj(D.SCENE)                     # test_final_defer_gpu's resting frames: the Cornell box, one fan pair a lamp
    table = D.material_table(len(mesh[1]))
    taken = {}
    for flags in (0, NEE | MIS):
        app = D.make(abi, (200, 83), flags, 4, mesh, table)
        for _ in range(8):
            app.drawScene(())
        info = app.backend.ctx.defer_info()
        taken[flags] = info["launched_in_trace"]
        assert info["recorded"] >= 4 and info["recorded"] - info["launched_in_trace"] - info["launched_alone"] <= 1, info
        app.backend.close()
    assert taken[NEE | MIS] == 0 and taken[0] >= 2, taken


# ------------------------------------------------------------------------------------------ 4. lifetime
@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["host_repose", "device_refit"])
def test_frames_follow_the_posed_scene(hip_lib, oracle, vflags):
    """0xD0000 on three instances of the unequal-lamps mesh: the frame is the walker's on the posed scene after
    rtpt_scene_set_instances (one instance scaled by powers of two, so its emitters' weights and q_i change), after
    rtpt_scene_rebuild, after a sheared ubo.model (re-posed on the host, or refit on the device with RTPT_FLAG_FORCE_BVH), after
    rtpt_resize, and after other materials — the hit emitter's entry and its q_i come from the re-posed table each time"""
    abi = hip_lib
    flags = NEE | MIS | POWER
    base = PW.unequal_lamps()
    rec = DS.records(base)
    lights = NP.light_list(base, 3)
    xf, posed = NP.translated(base, TN.OFFSETS3)
    seg = 5

    def check(ctx, sc, r, tag, model=None):
        want = walked(oracle, tag, sc, W0, H0, seg, r, lights, flags)
        assert want["weighted"] > 0, tag
        if model is None:
            got = frame(abi, oracle, ctx, sc, W0, H0)
        else:                                      # T.frame_on_gpu with the model in the UBO: the walker's scene is the posed one
            pc = G.fill_push_constants(abi.PushConstants(), P.push_constants(sc), 0)
            ubo = T._ubo(abi, oracle, sc, W0, H0)
            ubo.model[:] = model
            ctx.reset_counters()
            ctx.gbuffer(ubo)
            ctx.temporal_gradient(pc)
            ctx.raytrace(pc)
            got = dict(IMAGE=ctx.readback(abi.PLANE_IMAGE), HIT_ID=ctx.readback(abi.PLANE_HIT_ID), rays=ctx.raycount())
        same_frame(got, want, (tag, vflags))
        assert got["rays"] == want["rays"], tag
        return want

    with context(abi, base, W0, H0, seg, flags | vflags) as ctx:
        ctx.scene_upload(*FP.mesh_of(base.tris), instance_xforms=xf)
        ctx.set_materials(base.tri_material, base.materials)
        first = check(ctx, posed, rec, "posed3")
        scale = F32([[1, 1, 1], [2, 0.5, 1], [1, 1, 1]])
        move = F32(TN.MOVED3)
        xf2 = np.zeros((3, 3, 4), F32)
        for i in range(3):
            xf2[i, :, :3] = np.diag(scale[i])
            xf2[i, :, 3] = move[i]
        b = np.asarray(base.tris, F32).reshape(-1, 3, 3)
        moved_tris = np.concatenate([((b * scale[i][None, None, :]).astype(F32) + move[i][None, None, :]).astype(F32) for i in range(3)]).reshape(-1, 9)
        moved = base._replace(name="unequal_scaled3", tris=P._frozen(moved_tris))
        ctx.scene_set_instances(xf2.reshape(-1, 12))
        second = check(ctx, moved, rec, "moved3")
        assert not np.array_equal(bits(second["IMAGE"]), bits(first["IMAGE"]))
        ctx.scene_rebuild()
        check(ctx, moved, rec, "moved3")
        sheared = moved._replace(name="unequal_sheared3", tris=P._frozen(RM.posed(oracle, np.ascontiguousarray(moved.tris, F32), "general")))
        check(ctx, sheared, rec, "sheared3", RM.model("general"))
        check(ctx, moved, rec, "moved3")             # the identity again
        ctx.resize(W1, H1)
        ctx.resize(W0, H0)
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        check(ctx, moved, rec, "moved3")
        brighter = base.materials.copy()
        brighter[1, 3:] *= 16
        ctx.set_materials(base.tri_material, brighter)
        third = check(ctx, moved, DS.records(base._replace(materials=P._frozen(brighter))), "brighter3")
        assert not np.array_equal(bits(third["IMAGE"]), bits(second["IMAGE"]))


# ------------------------------------------------------------------------------------------ 5. hosts
KEYS = ["", "E", "J"]


@pytest.fixture(scope="module")
def wall_file(tmp_path_factory):
    """nee_paths.two_lamps() with nee_mis.wall_lamp()'s wall standing on its receiver, as wall.obj + wall.mtl: one `f` per triangle,
    one newmtl per material row"""
    two, wall = NP.two_lamps(), M.wall_lamp()
    n_mat = len(two.materials)
    scene = two._replace(tris=np.concatenate([np.asarray(two.tris, F32).reshape(-1, 9), np.asarray(wall.tris, F32).reshape(-1, 9)[2:]]),
                         tri_material=np.concatenate([np.asarray(two.tri_material), [n_mat, n_mat]]),
                         materials=np.concatenate([np.asarray(two.materials, F32), np.asarray(wall.materials, F32)[1:2]]))
    d = str(tmp_path_factory.mktemp("nee_mis_wall"))
    with open(os.path.join(d, "wall.mtl"), "w") as f:
        for i, m in enumerate(np.asarray(scene.materials, np.float64)):
            f.write("newmtl m%d\nKd %r %r %r\nKe %r %r %r\n" % ((i,) + tuple(float(x) for x in m)))
    with open(os.path.join(d, "wall.obj"), "w") as f:
        f.write("mtllib wall.mtl\n")
        for v in np.asarray(scene.tris, np.float64).reshape(-1, 3):
            f.write("v %r %r %r\n" % tuple(float(x) for x in v))
        for t, m in enumerate(np.asarray(scene.tri_material)):
            f.write("usemtl m%d\nf %d %d %d\n" % (m, 3 * t + 1, 3 * t + 2, 3 * t + 3))
    return os.path.join(d, "wall.obj")


def host_frames(path, size, in_flight=1, **kw):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    app = make_app(size[0], size[1], max_segments=5, iterations=5, scene=path, frames_in_flight=in_flight, specular=True, **kw)
    frames = []
    for k in KEYS:
        app.drawScene(tuple(k))
        frames.append(app.backend.final_image_rows(0, size[1]).copy())
    backends = getattr(app.backend, "be", [app.backend])
    rays = sum(b.ctx.raycount() for b in backends)
    app.backend.close()
    return frames, rays


def test_hosts_weigh_their_samples(hip_lib, oracle, wall_file, tmp_path):
    """make_app(nee_mis=True) on two_lamps with the wall lamp as an OBJ file: the frames differ from make_app(nee=True)'s with the same ray
    count, two frames in flight render the same frames, flags=0x90000 is the same switch, nee_mis beside nee_power and nee_sphere
    is 0xF0000, and rtpt_app --nee-mis (which implies --nee) dumps the last frame bit for bit with the same ray count, as one
    context and as two strips"""
    abi = hip_lib
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    size = N.SIZES[0]
    on, rays_on = host_frames(wall_file, size, nee_mis=True)
    plain, rays_plain = host_frames(wall_file, size, nee=True)
    assert rays_on == rays_plain > 0 and not np.array_equal(bits(on[-1]), bits(plain[-1]))
    two, rays_two = host_frames(wall_file, size, in_flight=2, nee_mis=True)
    assert rays_two == rays_on
    for f in range(len(KEYS)):
        assert np.array_equal(bits(two[f]), bits(on[f])), f
    flag, rays_flag = host_frames(wall_file, size, flags=NEE | MIS)
    assert rays_flag == rays_on and np.array_equal(bits(flag[-1]), bits(on[-1]))
    every, _ = host_frames(wall_file, size, nee_mis=True, nee_power=True, nee_sphere=True)
    every_flag, _ = host_frames(wall_file, size, flags=NEE | MIS | POWER | SPHERE)
    assert np.array_equal(bits(every[-1]), bits(every_flag[-1])) and not np.array_equal(bits(every[-1]), bits(on[-1]))
    app_binary = os.path.join(D.PKG, "rtpt_app")
    assert os.path.exists(app_binary), "build() leaves rtpt_app next to the package"
    dumps = {}
    for extra in (["--nee-mis"], ["--nee-mis", "--ranks", "2"], ["--nee"], ["--nee-mis", "--nee-power", "--nee-sphere"]):
        pfm = tmp_path / "out.pfm"
        cmd = [app_binary, "--width", str(size[0]), "--height", str(size[1]), "--segments", "5", "--iterations", "5", "--frames", str(len(KEYS)),
               "--script", ",".join(KEYS), "--dump", str(pfm), "--scene", wall_file, "--specular"] + extra
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        dumps[tuple(extra)] = (read_pfm(str(pfm)), json.loads(out.stdout.strip().splitlines()[-1])["rays"])
    for extra in (("--nee-mis",), ("--nee-mis", "--ranks", "2")):
        assert np.array_equal(bits(dumps[extra][0]), bits(np.ascontiguousarray(on[-1][..., :3]))), extra
        assert dumps[extra][1] == rays_on, extra
    assert np.array_equal(bits(dumps[("--nee",)][0]), bits(np.ascontiguousarray(plain[-1][..., :3])))
    assert not np.array_equal(bits(dumps[("--nee",)][0]), bits(dumps[("--nee-mis",)][0]))
    assert np.array_equal(bits(dumps[("--nee-mis", "--nee-power", "--nee-sphere")][0]), bits(np.ascontiguousarray(every[-1][..., :3])))
    help_text = subprocess.run([app_binary, "--help"], capture_output=True, text=True)
    assert "--nee-mis" in help_text.stdout + help_text.stderr
