"""Next-event estimation in the tile kernels (RTPT_FLAG_EXT_NEE; csrc/light_sample.hpp states the rules), in the order of what each
check can catch: the light list as it stands on the device against tests/nee_paths.light_list — the narrowest test of the upload,
able to run alone — then whole frames against the numpy walker path_walker.walk (held on the CPU by
tests/test_nee_paths_cpu.py), IMAGE, HIT_ID and the ray count bit for bit; demodulation; the identities of a context whose list is
empty; lifetime and the launches a sampling frame does not take; and the two hosts.  Every test but
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
import path_walker as WK
import pathtrace_scenes as P
import test_demodulate_gpu as D
import test_pathtrace_scenes_gpu as T
import texture_scenes as TS
from conftest import ROOT, bits
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
W0, H0 = N.SIZES[0]
W1, H1 = N.SIZES[1]
FORCE_BVH, NO_COMPACTION, SINGLE_LAUNCH, UNFUSED, DEMODULATE, NEE = 0x2, 0x8, 0x200, 0x400, 0x8000, 0x10000
STRIP_ROWS = (5, 21)
OFFSETS3 = ((0.0, 0.0, 0.0), (0.25, -0.5, -1.0), (-0.5, 0.25, -2.0))
MOVED3 = ((0.0, 0.0, 0.0), (0.5, -0.25, -1.5), (-0.25, 0.5, -2.5))

_walked = {}


# ------------------------------------------------------------------------------------------ one frame, both sides
def context(abi, scene, W, H, segments, flags=NEE, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def upload(abi, ctx, scene, glass=None, xf=None, base=None):
    """scene.tris, or the mesh of `base` under the instance transforms xf; the extended call where some material is glass, the plain
    one elsewhere, so that both build the list"""
    ctx.scene_upload(*FP.mesh_of((base or scene).tris), instance_xforms=xf)
    if glass:
        ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, None, glass))
    else:
        ctx.set_materials(scene.tri_material, scene.materials)


def frame(abi, oracle, ctx, scene, W, H, planes=(), frame_no=0):
    out = T.frame_on_gpu(abi, oracle, ctx, scene, W, H, frame_no)
    for p in planes:
        out[p] = ctx.readback(getattr(abi, "PLANE_" + p))
    return out


def walked(oracle, key, scene, W, H, segments, rec, lights, spp=1, rows=None, texture=None):
    """the walker's frame, computed once and left unchanged"""
    key = (key, W, H, segments, spp, len(lights))
    if key not in _walked:
        r = WK.walk(oracle, scene, W, H, segments, rec, lights, spp=spp, tex=None if texture is None else WK.Tex(*texture, None))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _walked[key] = r
    return _walked[key]


def glass_room(form):
    scene, glass = DS.glass_room(form)
    rec = DS.records(scene, None, glass)
    return scene, glass, rec, NP.light_list(scene, 1, rec)


def same_frame(got, want, tag, rows=None):
    y0, y1 = rows or (0, len(want["IMAGE"]))
    same_bits(got["HIT_ID"], want["HIT_ID"][y0:y1], tag + ("HIT_ID",))
    same_bits(got["IMAGE"], want["IMAGE"][y0:y1], tag + ("IMAGE",))


# ------------------------------------------------------------------------------------------ 1. the light list on the device
def test_light_list_readback(hip_lib, oracle):
    """rtpt_debug_light_list against nee_paths.light_list: the receiver (rtpt_scene_set_materials), the glass room small and as fan
    pairs (rtpt_scene_set_materials_ext), three instances of the receiver's mesh, the same after rtpt_scene_set_instances and after
    rtpt_scene_rebuild; dropped materials leave n = 0, a second table with other emitters leaves the new list, a context without the
    flag has none, and the list costs 4 bytes an entry of device memory and nothing when it is empty"""
    abi = hip_lib
    gc.collect()
    rcv = N.receiver()
    with context(abi, rcv, W0, H0, 2) as ctx:
        assert len(ctx.debug_light_list()) == 0, "no scene, no list"
        ctx.scene_upload(*FP.mesh_of(rcv.tris))
        held = abi.live_device_bytes()
        ctx.set_materials(rcv.tri_material, rcv.materials)
        got = ctx.debug_light_list()
        assert got.dtype == U32 and got.tolist() == NP.light_list(rcv).tolist() == [3, 4]
        assert abi.live_device_bytes() - held == 32 * len(rcv.tris) + 4 * 2
        ctx.set_materials(None, None)
        assert len(ctx.debug_light_list()) == 0 and abi.live_device_bytes() == held, "dropping the materials drops the list"
        swapped = rcv.materials.copy()
        swapped[:, 3:] = swapped[::-1, 3:]                      # the receiver emits, the lamp does not
        ctx.set_materials_ext(rcv.tri_material, abi.materials_ext(swapped))
        assert ctx.debug_light_list().tolist() == [1, 2]
        ctx.set_materials_ext(rcv.tri_material, abi.materials_ext(rcv.materials))
        assert ctx.debug_light_list().tolist() == [3, 4], "a second table leaves the new list"
        dark = rcv.materials.copy()
        dark[:, 3:] = 0
        ctx.set_materials(rcv.tri_material, dark)
        assert len(ctx.debug_light_list()) == 0 and abi.live_device_bytes() - held == 32 * len(rcv.tris), "no emitter: no allocation"
        ctx.set_materials(rcv.tri_material, rcv.materials)
        ctx.scene_upload(*FP.mesh_of(rcv.tris))
        assert len(ctx.debug_light_list()) == 0, "rtpt_scene_upload drops the list with the scene"
    with context(abi, rcv, W0, H0, 2, flags=0) as ctx:
        upload(abi, ctx, rcv)
        assert len(ctx.debug_light_list()) == 0, "without the flag no list is built"
    for form in ("small", "pairs"):
        scene, glass, rec, lights = glass_room(form)
        with context(abi, scene, W0, H0, 9) as ctx:
            upload(abi, ctx, scene, glass)
            assert ctx.debug_light_list().tolist() == lights.tolist() and len(lights) == (2 if form == "small" else 18)
    xf, _ = NP.translated(rcv, OFFSETS3)
    want3 = NP.light_list(rcv, 3)
    assert want3.tolist() == [3, 4, 7, 8, 11, 12]
    with context(abi, rcv, W0, H0, 2) as ctx:
        upload(abi, ctx, rcv, xf=xf)
        assert ctx.debug_light_list().tolist() == want3.tolist()
        ctx.scene_set_instances(NP.translated(rcv, MOVED3)[0])
        assert ctx.debug_light_list().tolist() == want3.tolist(), "rtpt_scene_set_instances keeps the list"
        ctx.scene_rebuild()
        assert ctx.debug_light_list().tolist() == want3.tolist(), "rtpt_scene_rebuild keeps the list"


# ------------------------------------------------------------------------------------------ 2. whole frames against the walker
@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
@pytest.mark.parametrize("segments", [2, 5])
def test_receiver_equals_the_walker(hip_lib, oracle, segments, vflags):
    """the receiver under its trapezoid lamp, pixel_jitter 0, at 64 x 48 and 70 x 10: every pixel samples the lamp at its first hit,
    and nothing stands between"""
    abi = hip_lib
    scene = N.receiver()
    rec, lights = DS.records(scene), NP.light_list(scene)
    for W, H in (N.SIZES[0], N.SIZES[1]):
        want = walked(oracle, "receiver", scene, W, H, segments, rec, lights)
        assert want["samples"] > 0 and want["queries"] == want["samples"] and want["lit"] > 0.99 * want["queries"]
        with context(abi, scene, W, H, segments, NEE | vflags) as ctx:
            upload(abi, ctx, scene)
            got = frame(abi, oracle, ctx, scene, W, H)
        same_frame(got, want, ("receiver", W, H, segments, vflags))
        assert got["rays"] == want["rays"], ("receiver", W, H, segments, vflags)


@pytest.mark.parametrize("segments", [9, 33])
@pytest.mark.parametrize("form,base", [("small", 0), ("pairs", 0), ("small", FORCE_BVH)], ids=["small", "pairs", "force_bvh"])
def test_glass_room_equals_the_walker(hip_lib, oracle, form, base, segments):
    """the glass room with its lamp (26 triangles, 234 as fan pairs): diffuse, dielectric and emissive hits, so the sampled bit is
    set and cleared along a path.  The default schedule, RTPT_FLAG_NO_PATH_COMPACTION, the unfused launch
    (RTPT_FLAG_NO_FILTER_FUSION), RTPT_FLAG_SINGLE_LAUNCH_PATHS (which a sampling launch is anyway), and a strip context with
    row_begin 5"""
    abi = hip_lib
    scene, glass, rec, lights = glass_room(form)
    want = walked(oracle, "glass_room_" + form, scene, W0, H0, segments, rec, lights)
    off = WK.walk(oracle, scene, W0, H0, segments, rec) if segments == 9 and form == "small" and not base else None
    assert want["lit"] > 0 and want["queries"] > want["lit"], "the box shadows some samples"
    if off is not None:
        assert not np.array_equal(bits(off["IMAGE"]), bits(want["IMAGE"])) and want["rays"] > off["rays"]
    for sid, flags in (("default", 0), ("no_compaction", NO_COMPACTION), ("unfused", UNFUSED), ("single_launch", SINGLE_LAUNCH)):
        with context(abi, scene, W0, H0, segments, NEE | base | flags) as ctx:
            upload(abi, ctx, scene, glass)
            if form != "small":
                assert ctx.scene_build_info()["leaf_pairs"]
            got = frame(abi, oracle, ctx, scene, W0, H0)
        same_frame(got, want, (form, base, segments, sid))
        assert got["rays"] == want["rays"], (form, base, segments, sid)
    with context(abi, scene, W0, H0, segments, NEE | base, rows=STRIP_ROWS) as ctx:
        upload(abi, ctx, scene, glass)
        strip = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(strip, want, (form, base, segments, "strip"), STRIP_ROWS)


@pytest.mark.parametrize("form,base", [("small", 0), ("pairs", 0), ("small", FORCE_BVH)], ids=["small", "pairs", "force_bvh"])
def test_glass_room_second_shape_and_samples(hip_lib, oracle, form, base):
    """70 x 10 (partial tiles in x and y) with one, two and three samples per pixel: R restarts with every sample, the stored pixel
    is the mean of R + terminal, and a path's last segment moves the stream by its two draws only"""
    abi = hip_lib
    scene, glass, rec, lights = glass_room(form)
    for segments, spp in ((9, 1), (2, 2), (5, 3)):
        want = walked(oracle, "glass_room_" + form, scene, W1, H1, segments, rec, lights, spp)
        with context(abi, scene, W1, H1, segments, NEE | base, spp) as ctx:
            upload(abi, ctx, scene, glass)
            got = frame(abi, oracle, ctx, scene, W1, H1)
        same_frame(got, want, (form, base, segments, spp))
        assert got["rays"] == want["rays"], (form, base, segments, spp)


@pytest.mark.parametrize("vflags", [0, FORCE_BVH], ids=["brute", "bvh"])
def test_occluder_and_two_lamps(hip_lib, oracle, vflags):
    """an opaque quad between part of the receiver and the lamp: shadowed samples add nothing, and both shadowed and lit samples
    occur; and two lamps of unequal area and colour with a degenerate emissive triangle in the list, whose samples are never valid"""
    abi = hip_lib
    for scene in (NP.occluder(), NP.two_lamps()):
        rec, lights = DS.records(scene), NP.light_list(scene)
        for segments in (2, 5):
            want = walked(oracle, scene.name, scene, W0, H0, segments, rec, lights)
            if scene.name == "nee_occluder":
                assert want["lit"] > 100 and want["queries"] - want["lit"] > 100, "both shadowed and lit samples occur"
            else:
                assert lights.tolist() == [3, 4, 5, 6, 7] and want["samples"] - want["queries"] > 0.1 * want["samples"], "the degenerate light"
            with context(abi, scene, W0, H0, segments, NEE | vflags) as ctx:
                upload(abi, ctx, scene)
                assert ctx.debug_light_list().tolist() == lights.tolist()
                got = frame(abi, oracle, ctx, scene, W0, H0)
            same_frame(got, want, (scene.name, segments, vflags))
            assert got["rays"] == want["rays"], (scene.name, segments, vflags)


MIRROR_KS, GLOSS_KS = (0.875, 0.75, 0.625), (0.5, 0.75, 0.25)


@pytest.mark.parametrize("segments", [5, 9])
@pytest.mark.parametrize("form,base", [("small", 0), ("pairs", 0), ("small", FORCE_BVH)], ids=["small", "pairs", "force_bvh"])
def test_mirror_room_equals_the_walker(hip_lib, oracle, form, base, segments):
    """the glass room with its box a MIRROR (roughness 0) and its floor glossy (roughness 0.25): a specular hit takes no light draw
    and clears the sampled bit, so a lamp seen in the mirror behind a diffuse hit returns T Ke, where a lamp met straight from a
    diffuse hit returns 0 — both occur, and the frame, its ids and its ray count are the walker's"""
    abi = hip_lib
    scene, _ = DS.glass_room(form)
    spec = {6: (MIRROR_KS, 0.0), 2: (GLOSS_KS, 0.25)}
    rec = DS.records(scene, spec)
    lights = NP.light_list(scene, 1, rec)
    want = walked(oracle, "mirror_room_" + form, scene, W0, H0, segments, rec, lights)
    assert want["kept"] > 0 and want["dropped"] > 0 and want["lit"] > 0, want
    for sid, flags in (("default", 0), ("no_compaction", NO_COMPACTION)):
        with context(abi, scene, W0, H0, segments, NEE | base | flags) as ctx:
            ctx.scene_upload(*FP.mesh_of(scene.tris))
            ctx.set_materials_ext(scene.tri_material, abi.materials_ext(scene.materials, spec))
            assert ctx.debug_light_list().tolist() == lights.tolist()
            got = frame(abi, oracle, ctx, scene, W0, H0)
        same_frame(got, want, ("mirror", form, base, segments, sid))
        assert got["rays"] == want["rays"], ("mirror", form, base, segments, sid)


def texture_setup(n_tris, mips):
    """(tri_uv, tri_texture, textures, texels) for n_tris base triangles, every fifth untextured.  Without mips: four bilinear
    textures of distinct texels (TEX = 1).  With: four constant images with RTPT_TEX_MIPMAP (TEX = 2) — every level of a generated
    chain of a constant dyadic colour holds that colour, so the walker's level-0 read is the read of any level"""
    if mips:
        desc, texels = TS.constants_atlas([(0.5, 0.75, 0.25), (0.75, 0.5, 1.0), (0.25, 0.25, 0.5), (1.0, 0.75, 0.75)], flags=0x10)
    else:
        desc, texels = TS.four_sizes()
    tri_texture = (np.arange(n_tris) % (len(desc) + 1)).astype(np.uint32)
    return TS.random_uv(n_tris, 11), tri_texture, desc, texels


@pytest.mark.parametrize("mips", [False, True], ids=["tex1", "tex2_mips"])
@pytest.mark.parametrize("form,base", [("small", 0), ("pairs", 0), ("small", FORCE_BVH)], ids=["small", "pairs", "force_bvh"])
def test_textured_room_equals_the_walker(hip_lib, oracle, form, base, mips):
    """the glass room with albedo textures on four of every five triangles, sampled at every hit: the TEX = 1 and TEX = 2
    instantiations of the sampling kernels against the walker, which multiplies a hit's albedo by texture_scenes.sample's texel;
    plain and demodulated (ALBEDO then holds colour x texel, and IMAGE x ALBEDO is the plain frame within test_demodulate_gpu's bar)"""
    abi = hip_lib
    scene, glass, rec, lights = glass_room(form)
    tex = texture_setup(len(scene.tris), mips)
    seg = 5
    want = walked(oracle, f"textured_{form}_{mips}", scene, W0, H0, seg, rec, lights, texture=tex)
    plain = walked(oracle, "glass_room_" + form, scene, W0, H0, seg, rec, lights)
    assert not np.array_equal(bits(want["IMAGE"]), bits(plain["IMAGE"])) and want["lit"] > 0
    out = {}
    for flags in (0, NO_COMPACTION, DEMODULATE):
        with context(abi, scene, W0, H0, seg, NEE | base | flags) as ctx:
            upload(abi, ctx, scene, glass)
            ctx.set_textures(*tex)
            out[flags] = frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",) if flags & DEMODULATE else ())
        if not flags & DEMODULATE:
            same_frame(out[flags], want, ("textured", form, base, mips, flags))
        assert out[flags]["rays"] == want["rays"], ("textured", form, base, mips, flags)
    a, b = out[DEMODULATE], out[0]
    same_bits(a["HIT_ID"], b["HIT_ID"], ("textured demod", "HIT_ID"))
    alb, on_img, off_img = a["ALBEDO"][..., :3], a["IMAGE"][..., :3], b["IMAGE"][..., :3]
    went_on = ~(alb == 1).all(-1)
    err = np.abs((on_img * alb).astype(F32).astype(np.float64) - off_img.astype(np.float64))
    bound = (seg + 2) * 2.0 ** -23 * np.abs(off_img.astype(np.float64))
    assert (err[went_on] <= bound[went_on]).all(), (form, base, mips)


# ------------------------------------------------------------------------------------------ 3. demodulated
@pytest.mark.parametrize("form,base", [("small", 0), ("pairs", 0)], ids=["small", "pairs"])
def test_nee_trace_factorises(hip_lib, oracle, form, base):
    """RTPT_FLAG_EXT_DEMODULATE with NEE on the glass room, 4 segments: same HIT_ID and ray count, ALBEDO the first hit's colour, and
    IMAGE x ALBEDO against the undemodulated NEE frame within test_demodulate_gpu's bar (segments + 2) 2^-23 |value| — the gain of
    segment 0 is illumination.
    Measured on an MI355X: max err / bound 0.181 (small), 0.190 (pairs)."""
    abi = hip_lib
    scene, glass, rec, lights = glass_room(form)
    seg = 4
    out = {}
    for on in (True, False):
        with context(abi, scene, W0, H0, seg, NEE | base | (DEMODULATE if on else 0)) as ctx:
            upload(abi, ctx, scene, glass)
            out[on] = frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",) if on else ())
    a, b = out[True], out[False]
    same_bits(a["HIT_ID"], b["HIT_ID"], (form, "HIT_ID"))
    same_bits(b["IMAGE"], walked(oracle, "glass_room_" + form, scene, W0, H0, seg, rec, lights)["IMAGE"], (form, "the plain trace is the walker's"))
    assert a["rays"] == b["rays"]
    alb, on_img, off_img = a["ALBEDO"][..., :3], a["IMAGE"][..., :3], b["IMAGE"][..., :3]
    ended = (alb == 1).all(-1)
    same_bits(on_img[ended], off_img[ended], (form, "ended at the first query"))
    went_on = ~ended
    prod = (on_img * alb).astype(F32)
    err = np.abs(prod.astype(np.float64) - off_img.astype(np.float64))
    bound = (seg + 2) * 2.0 ** -23 * np.abs(off_img.astype(np.float64))
    print(f"NEE demodulated {form}: max err / bound = {np.max(err[went_on] / np.maximum(bound[went_on], 1e-300)):.3f}")
    assert (err[went_on] <= bound[went_on]).all()


# ------------------------------------------------------------------------------------------ 4. identities
def test_flag_on_without_an_emitter_is_flag_off(hip_lib, oracle):
    """no emitter in the table, and no table at all: a context with the flag renders the frames of one without, bit for bit, ray
    count included — also textured (without and with mip chains), demodulated and with three samples"""
    abi = hip_lib
    scene, glass = DS.glass_room("small")
    dark = scene.materials.copy()
    dark[:, 3:] = 0
    cases = (("dark", dark, 0, 1, None), ("dark_demod", dark, DEMODULATE, 1, None), ("none", None, 0, 3, None), ("dark_bvh", dark, FORCE_BVH, 1, None),
             ("dark_tex1", dark, 0, 1, False), ("dark_tex2", dark, FORCE_BVH, 1, True), ("none_tex1_demod", None, DEMODULATE, 1, False))
    for tag, materials, flags, spp, mips in cases:
        frames = []
        for nee in (0, NEE):
            with context(abi, scene, W0, H0, 9, nee | flags, spp) as ctx:
                ctx.scene_upload(*FP.mesh_of(scene.tris))
                if materials is not None:
                    ctx.set_materials_ext(scene.tri_material, abi.materials_ext(materials, None, glass))
                if mips is not None:
                    ctx.set_textures(*texture_setup(len(scene.tris), mips))
                assert len(ctx.debug_light_list()) == 0
                frames.append(frame(abi, oracle, ctx, scene, W0, H0, ("ALBEDO",) if flags & DEMODULATE else ()))
        same_frame(frames[1], frames[0], (tag,))
        assert frames[1]["rays"] == frames[0]["rays"], tag
        if flags & DEMODULATE:
            same_bits(frames[1]["ALBEDO"], frames[0]["ALBEDO"], (tag, "ALBEDO"))


def test_flag_off_is_the_existing_walker(hip_lib, oracle):
    """without the flag the glass room with its lamp is the walker's frame without lights (this one passes without the feature too)"""
    abi = hip_lib
    scene, glass = DS.glass_room("small")
    want = WK.walk(oracle, scene, W0, H0, 9, DS.records(scene, None, glass))
    with context(abi, scene, W0, H0, 9, flags=0) as ctx:
        upload(abi, ctx, scene, glass)
        got = frame(abi, oracle, ctx, scene, W0, H0)
    same_frame(got, want, ("flag off",))
    assert got["rays"] == want["rays"]


def test_bench_scene_with_the_flag_is_without(hip_lib, tmp_path):
    """bench.py's scene has no material table, so no emissive triangle: --flags 0x10000 changes neither the frame it dumps nor its
    ray count (the 1080p workload: the same scene, a quarter of the pixels)"""
    import sys
    out = {}
    for flags in ("0", "0x10000"):
        d = tmp_path / flags
        d.mkdir()
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "1080p",
                            "--prewarm-seconds", "0", "--flags", flags, "--dump-outputs", str(d)], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        out[flags] = (json.loads(r.stdout.strip().splitlines()[-1]), np.load(str(d / "frame.npy")))
    assert out["0"][0]["rays_per_frame"] == out["0x10000"][0]["rays_per_frame"] > 0
    assert np.array_equal(bits(out["0"][1]), bits(out["0x10000"][1]))


# ------------------------------------------------------------------------------------------ 5. lifetime, refusals, launches not taken
def test_lifetime_of_the_list(hip_lib, oracle):
    """three instances of the occluder scene's mesh: frames equal the walker on the posed scene after the upload, after
    rtpt_scene_set_instances moved two of them, after rtpt_scene_rebuild, after rtpt_resize to 70 x 10 and back, and under a
    changed ubo.model (the refit rewrites the shade records a sample reads its light's vertices from; the list is as it was);
    then rtpt_scene_upload drops the list"""
    abi = hip_lib
    base = NP.occluder()
    rec = DS.records(base)
    lights = NP.light_list(base, 3)
    xf, posed = NP.translated(base, OFFSETS3)
    xf2, moved = NP.translated(base, MOVED3)
    with context(abi, base, W0, H0, 5) as ctx:
        upload(abi, ctx, base, xf=xf)
        same_frame(frame(abi, oracle, ctx, posed, W0, H0), walked(oracle, "posed3", posed, W0, H0, 5, rec, lights), ("uploaded",))
        ctx.scene_set_instances(xf2)
        want = walked(oracle, "moved3", moved, W0, H0, 5, rec, lights)
        got = frame(abi, oracle, ctx, moved, W0, H0)
        same_frame(got, want, ("moved",))
        assert got["rays"] == want["rays"]
        ctx.scene_rebuild()
        same_frame(frame(abi, oracle, ctx, moved, W0, H0), want, ("rebuilt",))
        ctx.resize(W1, H1)
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        same_frame(frame(abi, oracle, ctx, moved, W1, H1), walked(oracle, "moved3", moved, W1, H1, 5, rec, lights), ("resized",))
        ctx.resize(W0, H0)
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        same_frame(frame(abi, oracle, ctx, moved, W0, H0), want, ("resized back",))
        shift = F32([0.125, -0.25, -0.5])                       # a translation poses a vertex as v + t, one rounding
        model = np.eye(4, dtype=F32)
        model[3, :3] = shift
        posed_m = moved._replace(name="moved3_model", tris=P._frozen((np.asarray(moved.tris, F32).reshape(-1, 3) + shift).astype(F32).reshape(-1, 9)))
        want_m = walked(oracle, "moved3_model", posed_m, W0, H0, 5, rec, lights)
        assert not np.array_equal(bits(want_m["IMAGE"]), bits(want["IMAGE"])) and want_m["lit"] > 0
        pc = T.G.fill_push_constants(abi.PushConstants(), P.push_constants(moved), 0)
        ubo = T._ubo(abi, oracle, moved, W0, H0)
        ubo.model[:] = model.ravel()
        ctx.reset_counters()
        ctx.gbuffer(ubo)
        ctx.temporal_gradient(pc)
        ctx.raytrace(pc)
        got_m = dict(IMAGE=ctx.readback(abi.PLANE_IMAGE), HIT_ID=ctx.readback(abi.PLANE_HIT_ID), rays=ctx.raycount())
        same_frame(got_m, want_m, ("changed model",))
        assert got_m["rays"] == want_m["rays"] and ctx.debug_light_list().tolist() == lights.tolist(), "a changed model keeps the list"
        same_frame(frame(abi, oracle, ctx, moved, W0, H0), want, ("the identity again",))
        ctx.scene_upload(*FP.mesh_of(moved.tris))
        ctx.set_materials(np.tile(base.tri_material, 3), base.materials)
        assert ctx.debug_light_list().tolist() == lights.tolist(), "the flattened scene as one instance has the same list"
        same_frame(frame(abi, oracle, ctx, moved, W0, H0), want, ("flattened",))
        ctx.scene_upload(*FP.mesh_of(moved.tris))
        assert len(ctx.debug_light_list()) == 0


def test_a_sampling_launch_takes_neither_queues_nor_the_final_pass(hip_lib, oracle):
    """9 segments on the glass room: a context without the flag allocates the hand-over queues of the split launch, one that samples
    lights does not (rtpt_debug_live_device_bytes); and a host loop with the flag never takes a deferred final pass into its
    tracing launch (rtpt_debug_defer_info), where the same loop without the flag does"""
    abi = hip_lib
    gc.collect()
    scene, glass, rec, lights = glass_room("small")
    held = {}
    for nee in (0, NEE):
        before = abi.live_device_bytes()
        with context(abi, scene, W0, H0, 9, nee) as ctx:
            upload(abi, ctx, scene, glass)
            frame(abi, oracle, ctx, scene, W0, H0)
            held[nee] = abi.live_device_bytes() - before
    queue_bytes = ((W0 + 63) // 64) * ((H0 + 3) // 4) * 256 * 48
    assert held[0] - held[NEE] >= queue_bytes - 4 * len(lights), held
    mesh = abi.load_obj(D.SCENE)                     # test_final_defer_gpu's resting frames: the Cornell box, one fan pair a lamp
    table = D.material_table(len(mesh[1]))
    taken = {}
    for nee in (0, NEE):
        app = D.make(abi, (200, 83), nee, 4, mesh, table)
        for _ in range(8):
            app.drawScene(())
        info = app.backend.ctx.defer_info()
        taken[nee] = info["launched_in_trace"]
        assert info["recorded"] >= 4 and info["recorded"] - info["launched_in_trace"] - info["launched_alone"] <= 1, info
        assert len(app.backend.ctx.debug_light_list()) == (2 if nee else 0)
        app.backend.close()
    assert taken[NEE] == 0 and taken[0] >= 2, taken


# ------------------------------------------------------------------------------------------ 6. hosts
KEYS = ["", "E", "J"]


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    return DS.write_glass_room(str(tmp_path_factory.mktemp("nee_room")))


def host_frames(room, size, in_flight=1, **kw):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    app = make_app(size[0], size[1], max_segments=5, iterations=5, scene=room, frames_in_flight=in_flight, **kw)
    frames = []
    for k in KEYS:
        app.drawScene(tuple(k))
        frames.append(app.backend.final_image_rows(0, size[1]).copy())
    backends = getattr(app.backend, "be", [app.backend])
    rays = sum(b.ctx.raycount() for b in backends)
    lists = [b.ctx.debug_light_list().tolist() for b in backends]
    app.backend.close()
    return frames, rays, lists


def test_hosts_sample_the_lamp(hip_lib, room, tmp_path):
    """make_app(nee=True) on dielectric_scenes' room file (a lamp quad from the .mtl's Ke): every context has the lamp's two
    triangles in its list, the frames differ from the flag-off host's and cost more rays, two frames in flight render the same
    frames, and rtpt_app --nee dumps the last one bit for bit with the same ray count, as one context and as two strips"""
    abi = hip_lib
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    size = N.SIZES[0]
    tri, mats = abi.load_obj_materials(room)
    lamp = (np.flatnonzero((mats[tri][:, 3:] != 0).any(1)) + 1).tolist()
    assert len(lamp) == 2
    on, rays_on, lists = host_frames(room, size, dielectric=True, nee=True)
    off, rays_off, no_lists = host_frames(room, size, dielectric=True)
    assert lists == [lamp] and no_lists == [[]]
    assert rays_on > rays_off and not np.array_equal(bits(on[-1]), bits(off[-1]))
    two, rays_two, lists_two = host_frames(room, size, in_flight=2, dielectric=True, nee=True)
    assert lists_two == [lamp, lamp] and rays_two == rays_on
    for f in range(len(KEYS)):
        assert np.array_equal(bits(two[f]), bits(on[f])), f
    flag, rays_flag, flag_lists = host_frames(room, size, dielectric=True, flags=NEE)      # the flag by its other name
    assert flag_lists == [lamp] and rays_flag == rays_on and np.array_equal(bits(flag[-1]), bits(on[-1]))
    app_binary = os.path.join(D.PKG, "rtpt_app")
    assert os.path.exists(app_binary), "build() leaves rtpt_app next to the package"
    for extra in ([], ["--ranks", "2"]):
        pfm = tmp_path / "out.pfm"
        cmd = [app_binary, "--width", str(size[0]), "--height", str(size[1]), "--segments", "5", "--iterations", "5", "--frames", str(len(KEYS)),
               "--script", ",".join(KEYS), "--dump", str(pfm), "--scene", room, "--dielectric", "--nee"] + extra
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        stats = json.loads(out.stdout.strip().splitlines()[-1])
        assert np.array_equal(bits(read_pfm(str(pfm))), bits(np.ascontiguousarray(on[-1][..., :3]))), extra
        assert stats["rays"] == rays_on, extra
