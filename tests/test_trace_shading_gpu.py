"""What K2's shading leaves out (csrc/shade_segment.hpp: shade_segment, ray_hits_light; csrc/pathtrace_tile.hpp: the primary ray of pathtrace_tile)
must not show in any stored value: the last segment of a path returns before its bounce, the light test takes the sign of its
quotient from exact::quotient_positive, the primary ray's two divisions share a reciprocal.

  * exact::quotient_positive on the device against a / b > 0.0f over 2^33 pairs of arbitrary bits (rtpt_selftest_div mode 2);
  * frames of the small rooms of tests/pathtrace_scenes.py at 96 x 12 (a partial tile column: 96 = 64 + 32, 12 = 3 tile rows,
    and 97 x 13 for a partial tile row and a 1-pixel column) against the oracle, bit for bit: IMAGE, HIT_ID and the ray count,
    with max_segments 1, 2 and 4, a budget one beyond the first window, three samples per pixel, textures, demodulation and an
    emitter at the last segment, over brute force, RTPT_FLAG_FORCE_BVH and RTPT_FLAG_SINGLE_LAUNCH_PATHS;
  * the light sphere around the camera, through the camera (c == 0 in the quadratic: the numerator of t2 is exactly 0 or 2 |b|),
    across the frame (its silhouette: discriminants near 0) and behind the camera.

The oracle's plain path loop (oracle_raytrace_seq_mat, the reference of this file) samples no texture; its statement of the
textured path, oracle_raytrace_ext, is compared frame by frame in tests/test_shading_ext_gpu.py.  Here a textured frame is compared
with the plain loop through an atlas of constants (texture p = the colour Kd_p over white materials is the material table,
test_textures_gpu.py), and the barycentrics of the last hit — which only a texture reads there — through distinct texels: the image of a 1-segment frame is the first hit's albedo, which a 2-segment demodulated
frame stores in ALBEDO from a hit that is NOT its last."""
import numpy as np
import pytest

import pathtrace_scenes as P
import texture_mip_scenes as MS
import texture_scenes as TS
from conftest import bits
from filter_planes import same_bits
from test_pathtrace_scenes_gpu import _config, compare, frame_on_gpu, reference, upload

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = ((96, 12), (97, 13))
W0, H0 = SHAPES[0]
# name -> (flags, environment read by rtpt_create)
ROUTES = {"brute": (0, {}), "force_bvh": (0x2, {}), "single_launch": (0x200, {}), "force_bvh_single_launch": (0x202, {}),
          "no_path_compaction": (0x8, {})}


def run(abi, oracle, route, scene, W, H, segments, spp=1, tag=(), textures=None, materials=None, flags=0):
    """one frame on the GPU against the oracle's; textures / materials replace what upload() sets.  Returns (oracle's, GPU's)"""
    tag = (route, scene.name, W, H, segments, spp) + tag
    ref = reference(oracle, scene, W, H, segments, spp)
    with abi.Context(_config(abi, scene, W, H, segments, spp, ROUTES[route][0] | flags)) as ctx:
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        upload(ctx, scene)
        if materials is not None:
            ctx.set_materials(*materials)
        if textures is not None:
            ctx.set_textures(*textures)
        got = frame_on_gpu(abi, oracle, ctx, scene, W, H)
        if flags & abi.FLAG_EXT_DEMODULATE:
            got["ALBEDO"] = ctx.readback(abi.PLANE_ALBEDO)
            ctx.modulate()
            got["SHADED"] = ctx.readback(abi.PLANE_SHADED)
    if not flags & abi.FLAG_EXT_DEMODULATE:
        compare(got, ref, None, tag)
    return ref, got


def ends(oracle, ref, segments):
    """paths (1 spp) by (the way they end, at the last segment or before)"""
    last = ref["seq_n"] == segments
    return {(k, at): int(((ref["seq_end"] == v) & (last if at == "last" else ~last)).sum())
            for k, v in (("light", oracle.END_LIGHT), ("sky", oracle.END_SKY), ("bound", oracle.END_BOUND), ("emissive", oracle.END_EMISSIVE))
            for at in ("last", "before")}


# ------------------------------------------------------------------------------------------ 1. the sign of a quotient
def test_quotient_positive_on_the_device(hip_lib):
    """one pass of mode 1's generator: 2^33 pairs of arbitrary bits, every other one with equal exponents"""
    with hip_lib.Context(hip_lib.config_default(64, 48)) as ctx:
        bad, first = ctx.selftest_div(2, 0, 1)
    assert bad == 0, f"exact::quotient_positive differs from a / b > 0.0f on {bad} pairs, e.g. {[hex(v) for v in first]}"


# ------------------------------------------------------------------------------------------ 2. the last segment
@pytest.mark.parametrize("segments", [1, 2, 4])
@pytest.mark.parametrize("route", ["brute", "force_bvh", "single_launch", "force_bvh_single_launch"])
def test_last_segment_of_every_budget(hip_lib, oracle, monkeypatch, route, segments):
    """three_ends: light, sky, an emitter and the bound end paths of one tile; mask_room: emitters end the paths of chosen pixels
    at segment 0 (with max_segments 1: on the last segment); closed_room: every path lives to the bound"""
    _env_of(monkeypatch, route)
    seen = {}
    for W, H in SHAPES:
        for name in ("three_ends", "mask_room", "closed_room"):
            ref, _ = run(hip_lib, oracle, route, P.scene(name, "small", W, H), W, H, segments)
            for k, v in ends(oracle, ref, segments).items():
                seen[k] = seen.get(k, 0) + v
    for k in ("light", "sky", "bound", "emissive"):
        assert seen[k, "last"] > 0, (k, "no path ends this way on its last segment", seen)
    if segments > 1:
        for k in ("light", "sky", "emissive"):
            assert seen[k, "before"] > 0, (k, seen)


def _env_of(monkeypatch, route, window=None):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)
    if window:
        monkeypatch.setenv("RTPT_PT_WINDOW", str(window))
    else:
        monkeypatch.delenv("RTPT_PT_WINDOW", raising=False)


@pytest.mark.parametrize("route,window", [("brute", None), ("brute", 1), ("brute", 2), ("force_bvh", None), ("force_bvh", 1)])
def test_budget_one_beyond_the_first_window(hip_lib, oracle, monkeypatch, route, window):
    """max_segments = window + 1: the tile kernel's last segment is not the path's (it must bounce and hand o, d and the RNG state
    over), the queue kernel's only segment is"""
    w = window or (4 if route == "brute" else 8)
    _env_of(monkeypatch, route, window)
    for name in ("closed_room", "three_ends", "mask_room"):
        ref, _ = run(hip_lib, oracle, route, P.scene(name, "small", W0, H0), W0, H0, w + 1, tag=("window", w))
        assert P.alive_after(ref["seq_n"], [w])[0] > 0, (name, "nothing is handed over")
        if name == "closed_room":
            assert (ref["seq_n"] == w + 1).all()


@pytest.mark.parametrize("segments", [1, 2])
@pytest.mark.parametrize("route", ["brute", "force_bvh", "no_path_compaction"])
def test_three_samples_continue_the_stream(hip_lib, oracle, monkeypatch, route, segments):
    """samples_per_pixel = 3: the next sample of a pixel starts from the RNG state behind the two draws of the bounce the last
    segment no longer evaluates"""
    _env_of(monkeypatch, route)
    for W, H in SHAPES:
        for name in ("closed_room", "three_ends", "mask_room"):
            ref, _ = run(hip_lib, oracle, route, P.scene(name, "small", W, H), W, H, segments, spp=3)
            if name == "closed_room":
                assert (ref["seq_n"] == 3 * segments).all(), "every sample of every pixel ends at the bound"


# ------------------------------------------------------------------------------------------ 3. textures at the last hit
def _white(scene):
    m = np.array(scene.materials, F32)
    m[:, :3] = 1.0
    return scene.tri_material, m


def _constants(scene, flags):
    """texture p = the constant colour Kd_p; every triangle reads its material's texture at random uv"""
    desc, texels = TS.constants_atlas(np.asarray(scene.materials)[:, :3], flags)
    return TS.random_uv(len(scene.tris), 7), (np.asarray(scene.tri_material) + 1).astype(np.uint32), desc, texels


def _distinct(scene, flags):
    """distinct values in every texel; every fifth triangle untextured; uv within a few repeats"""
    desc, texels = TS.four_sizes(flags)
    tri_texture = (np.arange(len(scene.tris)) % (len(desc) + 1)).astype(np.uint32)
    return TS.random_uv(len(scene.tris), 11), tri_texture, desc, texels


TEX_FLAGS = (("bilinear", 0), ("nearest", TS.NEAREST), ("mipmap", MS.MIPMAP))


@pytest.mark.parametrize("tex", TEX_FLAGS, ids=[t[0] for t in TEX_FLAGS])
@pytest.mark.parametrize("route", ["brute", "force_bvh"])
def test_textured_last_hit_equals_the_oracle(hip_lib, oracle, monkeypatch, route, tex):
    """white materials under an atlas of constants Kd_p (a generated chain of equal texels is that texel at every level): the
    frame of the material table, which the oracle computes; max_segments 1 (the textured hit is the last) and 2"""
    _env_of(monkeypatch, route)
    for segments in (1, 2):
        for name in ("mask_room", "three_ends"):
            scene = P.scene(name, "small", W0, H0)
            run(hip_lib, oracle, route, scene, W0, H0, segments, tag=("constants", tex[0]), textures=_constants(scene, tex[1]),
                materials=_white(scene))


@pytest.mark.parametrize("tex", TEX_FLAGS, ids=[t[0] for t in TEX_FLAGS])
@pytest.mark.parametrize("route", ["brute", "force_bvh"])
def test_last_hit_reads_the_texel_of_its_own_barycentrics(hip_lib, oracle, monkeypatch, route, tex):
    """distinct texels: IMAGE of a 1-segment frame (1 x albedo of the first hit, which is the last) and ALBEDO of a 1-segment
    demodulated frame equal ALBEDO of a 2-segment demodulated frame, whose first hit goes on to bounce"""
    abi = hip_lib
    _env_of(monkeypatch, route)
    for name in ("closed_room", "three_ends"):
        scene = P.scene(name, "small", W0, H0)
        out = {}
        for segments, demod in ((1, 0), (1, abi.FLAG_EXT_DEMODULATE), (2, abi.FLAG_EXT_DEMODULATE)):
            with abi.Context(_config(abi, scene, W0, H0, segments, 1, ROUTES[route][0] | demod)) as ctx:
                ctx.enable_debug(abi.DEBUG_HIT_ID)
                upload(ctx, scene)
                ctx.set_textures(*_distinct(scene, tex[1]))
                got = frame_on_gpu(abi, oracle, ctx, scene, W0, H0)
                if demod:
                    got["ALBEDO"] = ctx.readback(abi.PLANE_ALBEDO)
            out[segments, bool(demod)] = got
        want = out[2, True]["ALBEDO"]
        went_on = ~(want[..., :3] == 1).all(-1)      # neither light nor sky nor an emitter at segment 0
        assert went_on.mean() > 0.2, (name, went_on.mean())
        assert len(np.unique(bits(want[went_on][:, 0]))) > 20, "more albedos than materials: texels were read"
        for k in ((1, False), (1, True)):
            assert np.array_equal(out[k]["HIT_ID"], out[2, True]["HIT_ID"]), (name, k)
        same_bits(out[1, True]["ALBEDO"], want, (route, name, tex[0], "ALBEDO of 1 segment"))
        same_bits(out[1, False]["IMAGE"][went_on][:, :3], want[went_on][:, :3], (route, name, tex[0], "IMAGE of 1 segment"))


# ------------------------------------------------------------------------------------------ 4. demodulation, one segment
@pytest.mark.parametrize("route", ["brute", "force_bvh", "single_launch"])
def test_demodulation_with_one_segment(hip_lib, oracle, monkeypatch, route):
    """the mask room, max_segments 1: ALBEDO is Kd of the only hit and 1 on emitters; every Kd component is a power of two, so
    rtpt_modulate gives the oracle's image back bit for bit"""
    abi = hip_lib
    _env_of(monkeypatch, route)
    for W, H in SHAPES:
        scene = P.mask_room("small", W, H)
        ref, got = run(abi, oracle, route, scene, W, H, 1, flags=abi.FLAG_EXT_DEMODULATE)
        same_bits(got["HIT_ID"], ref["HIT_ID"], (route, W, H, "HIT_ID"))
        assert got["rays"] == ref["rays"]
        mat = scene.materials[scene.tri_material[ref["HIT_ID"] - 1]]
        emits = (mat[..., 3:] != 0).any(-1)
        assert np.array_equal(emits, P.mask(W, H)) and (ref["HIT_ID"] > 0).all() and emits.any() and not emits.all()
        want = np.zeros((H, W, 4), F32)
        want[..., :3] = np.where(emits[..., None], F32(1), mat[..., :3])
        same_bits(got["ALBEDO"], want, (route, W, H, "ALBEDO"))
        same_bits(got["SHADED"], ref["IMAGE"], (route, W, H, "SHADED"))
        same_bits(got["IMAGE"][emits], ref["IMAGE"][emits], (route, W, H, "emitters"))
        bound = ref["seq_end"] == oracle.END_BOUND
        assert np.array_equal(bound, ~emits) and (got["IMAGE"][bound][:, :3] == 1).all(), "a path that ends at its bound keeps its throughput of 1"


# ------------------------------------------------------------------------------------------ 5. the light test's edges
ROOM_CAM = np.array(P.ROOM_CAM, np.float64)
# (light position, radius): the camera inside the sphere; ON the sphere with the centre in front (oc . oc - r^2 is exactly 0 in
# binary32: oc = (0, 0, 0.25), r = 0.25; the numerator of t2 is 2 |b|) and behind (the numerator is exactly 0: t2 = 0 is no hit);
# the sphere inside the frame (its silhouette crosses pixels: discriminants on both sides of 0); behind the camera (t2 < 0)
LIGHTS = {
    "inside": (tuple(ROOM_CAM + (0.05, 0.0, -0.1)), 0.5),
    "on_sphere_front": (tuple(ROOM_CAM + (0.0, 0.0, -0.25)), 0.25),
    "on_sphere_behind": (tuple(ROOM_CAM + (0.0, 0.0, 0.25)), 0.25),
    "silhouette": (tuple(ROOM_CAM + (0.2, 0.02, -1.5)), 0.25),
    "behind": (tuple(ROOM_CAM + (0.0, 0.0, 0.4)), 0.125),
}


@pytest.mark.parametrize("where", list(LIGHTS))
@pytest.mark.parametrize("route", ["brute", "force_bvh"])
def test_light_sphere_at_the_edges_of_its_test(hip_lib, oracle, monkeypatch, route, where):
    _env_of(monkeypatch, route)
    pos, radius = LIGHTS[where]
    for jitter in (0.0, 0.375):
        scene = P.closed_room("small")._replace(name=f"closed_room_light_{where}_{jitter}", light=tuple(float(F32(v)) for v in pos),
                                                light_radius=radius, jitter=jitter)
        for segments in (1, 3):
            ref, _ = run(hip_lib, oracle, route, scene, W0, H0, segments, tag=(where,))
            first = (ref["seq_end"] == oracle.END_LIGHT) & (ref["seq_n"] == 1)
            if where in ("inside", "on_sphere_front"):
                assert first.all(), "every primary ray starts inside the sphere (or on it, towards its centre)"
            elif where == "silhouette":
                assert 0.005 < first.mean() < 0.5, first.mean()
            else:
                assert not first.any(), "the sphere is behind every primary ray"
                if segments == 3 and where == "behind":
                    assert (ref["seq_end"] == oracle.END_LIGHT).any(), "bounced rays do see it"
