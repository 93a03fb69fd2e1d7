"""Everything the path-trace kernels (K2) do after the first hit — shade_segment, the per-segment compaction through LDS, the
hand-over queue between the tile kernel and k_pathtrace_queue, the accumulators of samples_per_pixel > 1, the ray counter — on
the generated scenes of tests/pathtrace_scenes.py against the oracle, bit for bit (what the scenes exercise is checked on the
oracle in tests/test_pathtrace_scenes_cpu.py).  Every other GPU test runs these paths on the Cornell box seen from outside, or
with two segments.

Compared: the traced IMAGE (readback clears its alpha, as the oracle's is 0), HIT_ID and the ray count; NaNs as positions,
everything else as bits (same_bits of filter_planes.py).  The timing table names the kernel a route launched; it does not tell
the queue launches apart, so the window cases run RTPT_FLAG_SINGLE_LAUNCH_PATHS beside the queue.  What a case relies on (a
full queue, an empty tile, paths alive behind a window boundary) is asserted on the oracle's path dump of the same frame."""
import numpy as np
import pytest

import filter_planes as FP
import gbuffer_scenes as G
import pathtrace_scenes as P
from filter_planes import same_bits
from test_gbuffer_scenes_gpu import K012
from test_gbuffer_scenes_gpu import ROUTES as GBUFFER_ROUTES

pytestmark = pytest.mark.gpu

W0, H0 = P.MAIN_SHAPE
# name -> (flags, environment read by rtpt_create, launches of K012)
ROUTES = {k: GBUFFER_ROUTES[k] for k in ("default", "no_trace_fusion", "no_path_compaction", "force_bvh")}
ROUTES["single_launch"] = (0x200, {}, (0, 0, 0, 0, 1))

_ref_cache = {}


# ------------------------------------------------------------------------------------------ one frame, both sides
def reference(oracle, scene, W, H, segments=P.SEGMENTS, spp=1, frame=0, rows=None):
    key = (scene.name, scene.form, W, H, rows, segments, spp, frame)
    if key not in _ref_cache:
        r = P.oracle_frame(oracle, scene, W, H, segments, spp, frame, rows)
        FP.check_ids(r["HIT_ID"], len(scene.tris))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ref_cache[key] = r
    return _ref_cache[key]


def _ubo(abi, oracle, scene, W, H):
    """K0 looks where K2 does (down -z from the K2 camera); what it stores is not compared here"""
    u = abi.Ubo()
    eye = np.asarray(scene.cam, np.float32)
    extent = float(np.abs(np.asarray(scene.tris, np.float64).reshape(-1, 3) - np.asarray(scene.cam, np.float64)).max())
    proj = oracle.perspective(np.float32(G.FOVY), np.float32(W) / np.float32(H), 1e-3 * extent, 4.0 * extent)
    proj[5] *= -1
    u.model[:] = np.eye(4, dtype=np.float32).ravel()
    u.view[:], u.proj[:] = oracle.look_at(eye, (eye + np.float32([0, 0, -1])).astype(np.float32), (0.0, 1.0, 0.0)), proj
    u.modelPrev[:], u.viewPrev[:], u.projPrev[:] = u.model[:], u.view[:], u.proj[:]
    return u


def _config(abi, scene, W, H, segments, spp, flags, rows=None):
    cfg = P.configure(abi.config_default(W, H), scene, segments, spp)
    cfg.flags = flags
    if rows:
        cfg.row_begin, cfg.row_end = rows
    return cfg


def upload(ctx, scene):
    ctx.scene_upload(*FP.mesh_of(scene.tris))
    if scene.materials is not None:
        ctx.set_materials(scene.tri_material, scene.materials)
    else:
        ctx.set_materials(None, None)


def frame_on_gpu(abi, oracle, ctx, scene, W, H, frame=0):
    """K0, K1, K2 in the reference's order, then IMAGE, HIT_ID and the ray count"""
    pc = G.fill_push_constants(abi.PushConstants(), P.push_constants(scene), frame)
    ctx.reset_counters()
    ctx.gbuffer(_ubo(abi, oracle, scene, W, H))
    ctx.temporal_gradient(pc)
    ctx.raytrace(pc)
    return dict(IMAGE=ctx.readback(abi.PLANE_IMAGE), HIT_ID=ctx.readback(abi.PLANE_HIT_ID), rays=ctx.raycount())


def compare(got, ref, rows, tag):
    y0, y1 = rows or (0, len(ref["IMAGE"]))
    same_bits(got["HIT_ID"], ref["HIT_ID"][y0:y1], tag + ("HIT_ID",))
    same_bits(got["IMAGE"], ref["IMAGE"][y0:y1], tag + ("IMAGE",))
    assert got["rays"] == ref["rays"], tag + ("rays", got["rays"], ref["rays"])


def run_case(abi, oracle, route, scene, W, H, segments=P.SEGMENTS, spp=1, rows=None, tag=()):
    flags, _, launches = ROUTES[route]
    tag = (route, scene.name, scene.form, W, H, rows, segments, spp) + tag
    ref = reference(oracle, scene, W, H, segments, spp, 0, rows)
    with abi.Context(_config(abi, scene, W, H, segments, spp, flags, rows)) as ctx:
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        upload(ctx, scene)
        if scene.form != "small":      # (more than 64 triangles: the BVH kernels, over pairs or over triangles)
            assert bool(ctx.scene_build_info()["leaf_pairs"]) == (scene.form == "pairs"), tag
        ctx.timing_enable(1)
        got = frame_on_gpu(abi, oracle, ctx, scene, W, H)
        tm = ctx.timing_collect()
    compare(got, ref, rows, tag)
    assert tuple(tm[k][1] for k in K012) == launches, (tag, {k: v[1] for k, v in tm.items()})
    return ref


def _env(monkeypatch, route, window=None):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)
    if window:
        monkeypatch.setenv("RTPT_PT_WINDOW", str(window))


# ------------------------------------------------------------------------------------------ 1. routes x scenes
def _route_cases():
    out = []
    for route in ROUTES:
        for name, form in P.MAIN_SCENES:
            if route == "force_bvh" and form != "small":
                continue      # already a BVH form: the flag changes nothing
            out.append((route, name, form))
    return out


@pytest.mark.parametrize("route,name,form", _route_cases())
def test_routes_equal_the_oracle(hip_lib, oracle, monkeypatch, route, name, form):
    """9 segments: the brute-force forms hand over after 4 and compact at every segment, the BVH forms hand over after 8.  The
    mask room and three_ends also at the edge shapes (a 1-pixel-wide tile column, a 3-row last tile row, one pixel)"""
    _env(monkeypatch, route)
    shapes = ((W0, H0),) + (P.EDGE_SHAPES if name in ("mask_room", "three_ends") else ())
    for W, H in shapes:
        ref = run_case(hip_lib, oracle, route, P.scene(name, form, W, H), W, H)
        if name == "closed_room" and form == "small":
            assert ref["rays"] == W * H * P.SEGMENTS, "every queue is full"


# ------------------------------------------------------------------------------------------ 2. window boundaries
@pytest.mark.parametrize("name,form", P.WINDOW_SCENES)
@pytest.mark.parametrize("window", P.WINDOWS)
def test_window_boundaries(hip_lib, oracle, monkeypatch, window, name, form):
    """RTPT_PT_WINDOW = w: the tile kernel runs w segments, the queue launches w, 2w, 4w, ... more, writing queue 0, 1, 0, ...
    max_segments on, one past and far past every boundary (w = 1 and 17 segments: five queue launches); the same frames
    without the queue"""
    w = P.window_of(window, form)
    _env(monkeypatch, "default", window)
    scene = P.scene(name, form)
    handed = 0
    for segments in P.segment_values(w):
        for route in ("default", "single_launch"):
            ref = run_case(hip_lib, oracle, route, scene, W0, H0, segments, tag=("window", w))
        alive = P.alive_after(ref["seq_n"], P.window_boundaries(w, segments))
        if name == "closed_room" and form == "small":
            assert all(a == W0 * H0 for a in alive), "every record of every queue is written"
        assert all(a > 0 for a in alive), (name, form, w, segments, alive, "a queue that hands nothing over")
        handed += len(alive)
    assert handed >= 4, "boundaries were crossed"
    if name == "mask_room":
        assert "empty" in P.tile_patterns(W0, H0).values(), "a workgroup that appends nothing"


# ------------------------------------------------------------------------------------------ 3. frames and a resize in one context
@pytest.mark.parametrize("window", [1, None])
def test_two_frames_and_a_resize_in_one_context(hip_lib, oracle, monkeypatch, window):
    """closed room (every queue record written), the mask room after another upload (fewer records: the rest are stale), a
    larger frame (rtpt_resize frees the queues; the next trace sizes them anew), the closed room again"""
    abi = hip_lib
    _env(monkeypatch, "default", window)
    W1, H1 = P.RESIZED_SHAPE
    first = P.scene("closed_room_unjittered")      # one context, one pixel_jitter: the mask room's 0
    with abi.Context(_config(abi, first, W0, H0, P.SEGMENTS, 1, 0)) as ctx:
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        script = [(first, W0, H0, 0), (P.mask_room("small"), W0, H0, 1), (first, W1, H1, 2), (P.mask_room("small", W1, H1), W1, H1, 3)]
        size = (W0, H0)
        for scene, W, H, frame in script:
            if (W, H) != size:
                ctx.resize(W, H)
                size = (W, H)
            upload(ctx, scene)
            ref = reference(oracle, scene, W, H, frame=frame)
            got = frame_on_gpu(abi, oracle, ctx, scene, W, H, frame)
            compare(got, ref, None, ("one context", window, scene.name, W, H, frame))
            ctx.end_frame()
            if scene is first:
                assert ref["rays"] == W * H * P.SEGMENTS, "every queue record is written"


# ------------------------------------------------------------------------------------------ 4. strip
@pytest.mark.parametrize("name", ["closed_room", "mask_room"])
def test_strip_through_the_queue(hip_lib, oracle, monkeypatch, name):
    """rows [5, 21) of 130 x 33 stored, rows [8, 15) counted, window 1: the queue kernel's pixel index is relative to the first
    stored row, its ray counter tests the frame's row"""
    abi = hip_lib
    _env(monkeypatch, "default", 1)
    W, H, y0, y1 = P.STRIP
    c0, c1 = 8, 15
    scene = P.scene(name, "small", W, H, (y0, y1))
    ref = reference(oracle, scene, W, H, rows=(y0, y1))
    counted = reference(oracle, scene, W, H, rows=(c0, c1))
    assert 0 < counted["rays"] < ref["rays"]
    with abi.Context(_config(abi, scene, W, H, P.SEGMENTS, 1, 0, (y0, y1))) as ctx:
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        upload(ctx, scene)
        got = frame_on_gpu(abi, oracle, ctx, scene, W, H)
        compare(got, ref, (y0, y1), ("strip", name))
        ctx.set_count_rows(c0, c1)
        got = frame_on_gpu(abi, oracle, ctx, scene, W, H)
        compare(got, dict(ref, rays=counted["rays"]), (y0, y1), ("strip, counted rows", name))


# ------------------------------------------------------------------------------------------ 5. the queue kernel's second grid step
def test_queue_kernel_takes_a_second_grid_step(hip_lib, oracle):
    """k_pathtrace_queue runs 8 workgroups per CU, each 256 records per step: the closed room on the smallest frame whose full
    queue holds more records than that, by a few chunks and a partial one"""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    per_step = 8 * n_cu * 256
    W = 1021
    H = -(-per_step // W) + 1
    assert per_step < W * H < per_step + 2 * W and (W * H) % 256
    scene = P.closed_room("small")
    ref = run_case(hip_lib, oracle, "default", scene, W, H)
    assert (ref["seq_n"] == P.SEGMENTS).all(), "the queue is full: the grid's first step does not reach its end"


# ------------------------------------------------------------------------------------------ 6. three samples per pixel
@pytest.mark.parametrize("name,form", [("mask_room", "small"), ("three_ends", "small"), ("three_ends", "pairs"), ("three_ends", "odd")])
@pytest.mark.parametrize("route", ["default", "no_path_compaction", "force_bvh"])
def test_three_samples_per_pixel(hip_lib, oracle, monkeypatch, route, name, form):
    """paths of different length in one tile: after a compaction a thread finishes the path of another pixel than the one it
    started on, and writes that pixel's sum_* and rng_pix"""
    _env(monkeypatch, route)
    ref = run_case(hip_lib, oracle, route, P.scene(name, form), W0, H0, spp=3)
    assert P.tiles_with_end_segments(ref["seq_n"]) >= 6


# ------------------------------------------------------------------------------------------ 7. demodulation rides along
def test_demodulation_through_the_queue(hip_lib, oracle, monkeypatch):
    """the mask room with RTPT_FLAG_EXT_DEMODULATE, window 1: ALBEDO is Kd of the first hit, 1 on emitters; every Kd component is
    a power of two, so the products are exact in any order and rtpt_modulate gives the flag-off image back bit for bit"""
    abi = hip_lib
    _env(monkeypatch, "default", 1)
    scene = P.mask_room("small")
    ref = reference(oracle, scene, W0, H0)
    with abi.Context(_config(abi, scene, W0, H0, P.SEGMENTS, 1, abi.FLAG_EXT_DEMODULATE)) as ctx:
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        upload(ctx, scene)
        got = frame_on_gpu(abi, oracle, ctx, scene, W0, H0)
        albedo = ctx.readback(abi.PLANE_ALBEDO)
        ctx.modulate()
        shaded = ctx.readback(abi.PLANE_SHADED)
    same_bits(got["HIT_ID"], ref["HIT_ID"], ("demodulate", "HIT_ID"))
    assert got["rays"] == ref["rays"]
    mat = scene.materials[scene.tri_material[ref["HIT_ID"] - 1]]
    emits = (mat[..., 3:] != 0).any(-1)
    assert np.array_equal(emits, P.mask(W0, H0)) and (ref["HIT_ID"] > 0).all()
    want = np.zeros((H0, W0, 4), np.float32)
    want[..., :3] = np.where(emits[..., None], np.float32(1), mat[..., :3])
    same_bits(albedo, want, ("demodulate", "ALBEDO"))
    same_bits(shaded, ref["IMAGE"], ("demodulate", "SHADED"))
    went_on = ~emits
    assert not np.array_equal(got["IMAGE"][went_on], ref["IMAGE"][went_on]), "the image is demodulated"
    same_bits(got["IMAGE"][emits], ref["IMAGE"][emits], ("demodulate", "emitters"))
