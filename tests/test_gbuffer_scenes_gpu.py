"""K0 (G-buffer), K1 (temporal gradient) and the primary rays of K2 on generated adversarial input against the oracle, bit for
bit (tests/gbuffer_scenes.py; its claims are checked in tests/test_gbuffer_scenes_cpu.py).  Every other GPU test feeds these
passes the Cornell box, one heightfield and one soup from cameras that look at them from outside along -z.

  cull scenes    at most 64 triangles: the primary rays of K0 and K2 test only the triangles whose padded 16-bit screen rectangle
                 (screen_bounds, csrc/api_context.hip) meets the 16 x 4 pixel block of their wave (span_candidates,
                 closest_hit_brute_set, csrc/closest_hit.hpp).  rtpt_selftest_trace never takes that path.  A rectangle one pixel too
                 tight changes an id (the backdrop is behind every pixel), RTPT_FLAG_FORCE_BVH runs the same frames without it.
  K1             alone on injected ids / world positions / previous LUTs (k_gradient), as the first pass after an upload, a
                 re-upload or moved instances (it has to build the per-id tables it reads), and inside the K0 + K1 and the
                 K0 + K1 + K2 launch with every class of push constants and previous LUT.

Planes compared: VIS_ID, WORLDPOS, DEPTH, GRADIENT, HIT_ID, the traced IMAGE, the ray count.  NaNs are compared as positions,
everything else as bits (same_bits of filter_planes.py).  The timing table names the kernel a route launched."""
import numpy as np
import pytest

import filter_planes as FP
import gbuffer_scenes as G
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32).ravel()
SEGMENTS = 2
K012 = ("k_gbuffer", "k_gradient", "k_pathtrace", "k_gbuffer_gradient", "k_gbuffer_pathtrace")
# name -> (flags, environment read by rtpt_create, launches of K012)
ROUTES = {
    "default": (0, {}, (0, 0, 0, 0, 1)),
    "no_trace_fusion": (0, {"RTPT_NO_TRACE_FUSION": "1"}, (0, 0, 1, 1, 0)),
    "no_filter_fusion": (0x400, {}, (1, 1, 1, 0, 0)),
    "no_path_compaction": (0x8, {}, (0, 0, 1, 1, 0)),
    "force_bvh": (0x2, {}, (0, 0, 0, 0, 1)),          # no screen bounds: the cross-check that a difference comes from them
}
PLANES = ("VIS_ID", "WORLDPOS", "DEPTH", "GRADIENT", "HIT_ID", "IMAGE")

_ref_cache = {}


# ------------------------------------------------------------------------------------------ one frame, both sides
def _rot(angle, axis, shift):
    """column-major float32[16]: a rotation about `axis` followed by a translation"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    m[:3, 3] = shift
    return np.ascontiguousarray(m.astype(np.float32).T).ravel()


MODEL_TURNED = _rot(1.0, (0.3, 1.0, 0.2), (0.2, -0.1, 0.3))


def _ubo(cls, oracle, cam, W, H, model=EYE):
    u = cls()
    u.model[:] = model
    u.view[:], u.proj[:] = G.k0_camera(oracle, cam, W, H)
    u.modelPrev[:], u.viewPrev[:], u.projPrev[:] = u.model[:], u.view[:], u.proj[:]
    return u


def _config(mod, W, H, k2, rows=None, flags=None):
    cfg = mod.config_default(W, H)
    cfg.max_segments = SEGMENTS
    cfg.fov_slope, cfg.pixel_jitter = k2[1], k2[2]
    if flags is not None:
        cfg.flags = flags
        if rows:
            cfg.row_begin, cfg.row_end = rows
    return cfg


def _push_constants(cls, values, frame):
    return G.fill_push_constants(cls(), values, frame)


def reference(oracle, tris, cam, W, H, rows, k2, pcls, lut_prev, frame=0, model=EYE, key=None):
    """the oracle's frame: dict of PLANES (the stored rows), rays, lut and the push-constant values.  lut_prev: a class name of
    gbuffer_scenes.k1_lut_prev, an array, or None (D3: the LUT itself)"""
    if key is not None and key in _ref_cache:
        return _ref_cache[key]
    y0, y1 = rows or (0, H)
    posed = np.asarray(tris, np.float32)
    if not np.array_equal(model, EYE):   # world triangle = model * uploaded triangle: exactly the LUT's vertices
        posed = np.ascontiguousarray(oracle.lut(posed, model)[1:].reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9))
    lut = oracle.lut(posed, EYE)
    if lut_prev is None:
        lut_prev = lut
    elif isinstance(lut_prev, str):
        lut_prev = G.k1_lut_prev(lut_prev, posed)
    cfg = _config(oracle, W, H, k2)
    vis, wp, depth = oracle.gbuffer(cfg, posed, _ubo(oracle.Ubo, oracle, cam, W, H), y0, y1)
    values = G.k1_push_constants(pcls, vis[y0:y1], wp[y0:y1])
    if pcls != "camera_on_pixel":
        values["cameraPos"] = G.K2_POSITIONS[k2[0]]
    pc = _push_constants(oracle.PushConstants, values, frame)
    grad = oracle.temporal_gradient(cfg, pc, vis, wp, lut, lut_prev, y0, y1)
    image, rays, hit = oracle.raytrace(cfg, pc, posed, y0, y1)
    out = dict(VIS_ID=vis, WORLDPOS=wp, DEPTH=depth, GRADIENT=grad, HIT_ID=hit, IMAGE=image)
    out = {k: v[y0:y1] for k, v in out.items()}
    out.update(rays=rays, lut=lut, lut_prev=lut_prev, values=values, n_ids=len(np.unique(vis[y0:y1])))
    if key is not None:
        _ref_cache[key] = out
    return out


def frame_on_gpu(abi, ctx, ubo, values, frame):
    """K0, K1, K2 in the reference's order, then everything read back"""
    pc = _push_constants(abi.PushConstants, values, frame)
    ctx.reset_counters()
    ctx.gbuffer(ubo)
    ctx.temporal_gradient(pc)
    ctx.raytrace(pc)
    got = {p: ctx.readback(getattr(abi, "PLANE_" + p)) for p in PLANES}
    got["rays"] = ctx.raycount()
    return got


def compare(got, ref, tag):
    for p in PLANES:
        same_bits(got[p], ref[p], tag + (p,))
    assert got["rays"] == ref["rays"], tag + ("rays", got["rays"], ref["rays"])


def run_case(abi, oracle, route, tris, cam, W, H, rows, k2, pcls, lcls, tag, key=None):
    flags, _, launches = ROUTES[route]
    ref = reference(oracle, tris, cam, W, H, rows, k2, pcls, lcls, key=key)
    with abi.Context(_config(abi, W, H, k2, rows, flags)) as ctx:
        ctx.enable_debug(abi.DEBUG_HIT_ID)
        ctx.scene_upload(*FP.mesh_of(tris))
        if lcls is not None:
            ctx.set_plane(abi.PLANE_LUT_PREV, ref["lut_prev"])
        ctx.timing_enable(1)
        got = frame_on_gpu(abi, ctx, _ubo(abi.Ubo, oracle, cam, W, H), ref["values"], 0)
        tm = ctx.timing_collect()
    compare(got, ref, tag)
    assert tuple(tm[k][1] for k in K012) == launches and tm["k_lut"][1] == 1, (tag, {k: v[1] for k, v in tm.items()})
    return ref


def _env(monkeypatch, route):
    for k, v in ROUTES[route][1].items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------ K0 and K2 on the cull scenes
def k0k2_cases(ci):
    """(scene kind, W, H, stored rows, K2 camera, push-constant class, previous-LUT class) of camera number ci: every shape, the
    main shape with every scene of 40 triangles and more, the strip; scenes, K2 cameras and K1 classes rotate with the camera
    and the shape, so that over the cameras every scene meets every shape and every K2 camera"""
    out = []
    n = 0
    for si, (W, H) in enumerate(G.SHAPES):
        kinds = [G.SCENES[(ci + si) % len(G.SCENES)]]
        if (W, H) == G.MAIN_SHAPE:
            kinds = [("cull", 40), ("cull", 63), ("cull", 64), (("fan", 20), ("fan_odd", 20), ("fan", 32))[ci % 3]]
        for kind in kinds:
            out.append((kind, W, H, None, n))
            n += 1
    W, H, y0, y1 = G.STRIP
    out.append((G.SCENES[2 + ci % 6], W, H, (y0, y1), n))
    luts = (None,) + G.LUT_PREV_CLASSES      # None: nothing injected, LUT_PREV is the LUT (D3)
    return [(kind, W, H, rows, G.K2_CAMERAS[(ci + n) % len(G.K2_CAMERAS)], G.PC_CLASSES[(ci + n) % len(G.PC_CLASSES)], luts[(ci + 2 * n) % len(luts)])
            for (kind, W, H, rows, n) in out]


@pytest.mark.parametrize("cam", list(G.K0_CAMERAS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_cull_scenes_equal_the_oracle(hip_lib, oracle, monkeypatch, route, cam):
    _env(monkeypatch, route)
    ids_seen = 0
    for (kind, W, H, rows, k2, pcls, lcls) in k0k2_cases(list(G.K0_CAMERAS).index(cam)):
        tag = (route, cam, kind, W, H, rows, k2, pcls, lcls)
        ref = run_case(hip_lib, oracle, route, G.scene(kind), cam, W, H, rows, k2, pcls, lcls, tag, key=tag[1:])
        ids_seen = max(ids_seen, ref["n_ids"])
    assert ids_seen >= 12, "the camera sees the scene"


# ------------------------------------------------------------------------------------------ bounds follow the pose
@pytest.mark.parametrize("route", ["default", "no_filter_fusion", "force_bvh"])
def test_bounds_follow_the_pose(hip_lib, oracle, monkeypatch, route):
    """one context per scene, consecutive frames: ubo.model turned by a radian, then (two instances of 32 triangles) the
    instances moved, then the model back — every frame the oracle's with the same pose, LUT_PREV the frame before's LUT"""
    _env(monkeypatch, route)
    flags, _, launches = ROUTES[route]
    W, H = G.MAIN_SHAPE
    cam, k2 = "outside", G.K2_CAMERAS[0]
    base = np.ascontiguousarray(G.cull_scene(40)[:32])
    xyz, idx = FP.mesh_of(base)
    x0 = np.stack([_rot(0.0, (0, 1, 0), (0, 0, 0)).reshape(4, 4).T[:3], _rot(0.4, (0, 0, 1), (0.6, 0.2, -0.5)).reshape(4, 4).T[:3]])
    x1 = np.stack([_rot(0.9, (1, 1, 0), (-0.4, 0.1, 0.2)).reshape(4, 4).T[:3], _rot(-0.7, (0, 1, 1), (0.3, -0.2, 0.4)).reshape(4, 4).T[:3]])
    x0, x1 = (np.ascontiguousarray(x, np.float32).reshape(2, 12) for x in (x0, x1))
    single = [(G.cull_scene(64), None, EYE), (None, None, MODEL_TURNED), (None, None, EYE)]
    moving = [(None, x0, EYE), (None, x0, MODEL_TURNED), (None, x1, MODEL_TURNED), (None, x1, EYE)]
    for name, script in (("single", single), ("instances", moving)):
        with hip_lib.Context(_config(hip_lib, W, H, k2, None, flags)) as ctx:
            ctx.enable_debug(hip_lib.DEBUG_HIT_ID)
            if name == "single":
                ctx.scene_upload(*FP.mesh_of(script[0][0]))
                tris = script[0][0]
            else:
                ctx.scene_upload(xyz, idx, x0)
            ctx.timing_enable(1)
            lut_prev, current, seen = None, x0, []
            for f, (_, xf, model) in enumerate(script):
                if xf is not None:
                    if xf is not current:
                        ctx.scene_set_instances(xf)
                        current = xf
                    tris = oracle.flatten(xyz, idx, xf)
                    assert len(tris) == 64
                pcls = G.PC_CLASSES[f % 2]      # rest, moved
                ref = reference(oracle, tris, cam, W, H, None, k2, pcls, lut_prev, frame=f, model=model)
                got = frame_on_gpu(hip_lib, ctx, _ubo(hip_lib.Ubo, oracle, cam, W, H, model), ref["values"], f)
                compare(got, ref, (route, name, f))
                same_bits(ctx.readback(hip_lib.PLANE_LUT), ref["lut"], (route, name, f, "LUT"))
                ctx.end_frame()
                lut_prev = ref["lut"]
                seen.append(ref["VIS_ID"])
                assert ref["n_ids"] >= 12, (name, f)
            tm = ctx.timing_collect()
            assert tuple(tm[k][1] for k in K012) == tuple(len(script) * n for n in launches), (route, name, tm)
            assert all(not np.array_equal(seen[i], seen[i + 1]) for i in range(len(seen) - 1)), "every frame shows another pose"


# ------------------------------------------------------------------------------------------ K1 inside the fused launches
@pytest.mark.parametrize("lcls", G.LUT_PREV_CLASSES)
@pytest.mark.parametrize("route", ["default", "no_trace_fusion"])      # k_gbuffer_pathtrace / k_gbuffer_gradient
def test_gradient_inside_the_fused_launches(hip_lib, oracle, monkeypatch, route, lcls):
    """ids and world positions are K0's own there: the cull scenes with every class of push constants and an injected LUT_PREV of
    every class; GRADIENT equals the oracle's K1 fed the oracle's G-buffer (and every other plane the oracle's)"""
    _env(monkeypatch, route)
    W, H = G.MAIN_SHAPE
    li = G.LUT_PREV_CLASSES.index(lcls)
    moved = 0
    for pi, pcls in enumerate(G.PC_CLASSES):
        kind = (("cull", 40), ("cull", 63), ("cull", 64), ("fan", 32))[(li + pi) % 4]
        cam = G.MAIN_CAMERAS[(li + 2 * pi) % 4]
        k2 = G.K2_CAMERAS[(3 * li + pi) % len(G.K2_CAMERAS)]
        tag = ("fused K1", cam, kind, W, H, None, k2, pcls, lcls)
        ref = run_case(hip_lib, oracle, route, G.scene(kind), cam, W, H, None, k2, pcls, lcls, tag, key=tag[1:])
        lam = ref["GRADIENT"][..., 0]
        moved += int(((lam > 0) & (lam < 1)).sum())
    assert moved > 1000, "gradients strictly inside (0, 1) were compared"


# ------------------------------------------------------------------------------------------ K1 alone on injected planes
def _k1_combos(first):
    """every world-position class x previous-LUT class x push-constant class, starting at number `first`"""
    combos = [(w, l, p) for w in G.WP_CLASSES for l in G.LUT_PREV_CLASSES for p in G.PC_CLASSES]
    first %= len(combos)
    return combos[first:] + combos[:first]


def _k1_reference(oracle, tris, W, H, rows, combo, key):
    if key in _ref_cache:
        return _ref_cache[key]
    T = len(tris)
    y0, y1 = rows or (0, H)
    wcls, lcls, pcls = combo
    ids = np.array(G.k1_ids(T, W, H))
    wp = G.k1_worldpos(wcls, tris, ids)
    lut, lut_prev = oracle.lut(tris, EYE), G.k1_lut_prev(lcls, tris)
    values = G.k1_push_constants(pcls, ids[y0:y1], wp[y0:y1])
    pc = _push_constants(oracle.PushConstants, values, 0)
    grad = oracle.temporal_gradient(oracle.config_default(W, H), pc, FP.check_ids(ids, T), wp, lut, lut_prev, y0, y1)
    out = dict(ids=np.ascontiguousarray(ids[y0:y1]), wp=np.ascontiguousarray(wp[y0:y1]), lut=lut, lut_prev=lut_prev, values=values,
               grad=grad[y0:y1])
    _ref_cache[key] = out
    return out


K1_SHAPES = tuple((W, H, None) for (W, H) in G.SHAPES) + ((G.STRIP[0], G.STRIP[1], G.STRIP[2:]),)
ONE = np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], np.float32)
MOVED = np.ascontiguousarray(_rot(0.8, (1.0, 0.5, 0.2), (0.3, -0.2, 0.1)).reshape(4, 4).T[:3].reshape(1, 12))


def _k1_alone(abi, oracle, how, W, H, rows, first):
    """one context: the scene arrives as `how` says, then every combination of classes is injected (VIS_ID, WORLDPOS, LUT_PREV)
    and rtpt_temporal_gradient runs alone; the FIRST call is the one that meets the state `how` left"""
    T = G.K1_T
    soup = FP.soup(T)
    xyz, idx = FP.mesh_of(soup)
    tris = oracle.flatten(xyz, idx, MOVED) if how == "moved_instances" else soup
    cfg = abi.config_default(W, H)
    if rows:
        cfg.row_begin, cfg.row_end = rows
    ubo = _ubo(abi.Ubo, oracle, "outside", W, H)
    with abi.Context(cfg) as ctx:
        if how == "reupload":         # another scene uploaded and rendered before: its tables must not survive
            ctx.scene_upload(*FP.mesh_of(FP.soup(T, seed=1)))
            ctx.gbuffer(ubo)
            ctx.sync()
        if how == "moved_instances":  # rendered in one pose, then moved: the tables are those of the pose before
            ctx.scene_upload(xyz, idx, ONE)
            ctx.gbuffer(ubo)
            ctx.sync()
            ctx.scene_set_instances(MOVED)
        else:
            ctx.scene_upload(xyz, idx)
        if how == "gbuffer_first":
            ctx.gbuffer(ubo)
        ctx.timing_enable(1)
        combos = _k1_combos(first)
        for n, combo in enumerate(combos):
            r = _k1_reference(oracle, tris, W, H, rows, combo, ("K1", how == "moved_instances", W, H, rows, combo))
            ctx.set_plane(abi.PLANE_VIS_ID, FP.check_ids(r["ids"], T))
            ctx.set_plane(abi.PLANE_WORLDPOS, r["wp"])
            ctx.set_plane(abi.PLANE_LUT_PREV, r["lut_prev"])
            ctx.temporal_gradient(_push_constants(abi.PushConstants, r["values"], 0))
            same_bits(ctx.readback(abi.PLANE_GRADIENT), r["grad"], (how, W, H, rows, n) + combo)
            if n == 0:
                same_bits(ctx.readback(abi.PLANE_LUT), r["lut"], (how, W, H, "LUT"))
        tm = ctx.timing_collect()
        assert tm["k_gradient"][1] == len(combos) and tm["k_gbuffer_gradient"][1] == 0, tm


@pytest.mark.parametrize("shape", range(len(K1_SHAPES)))
@pytest.mark.parametrize("how", ["gbuffer_first", "k1_first"])
def test_gradient_alone_on_injected_planes(hip_lib, oracle, how, shape):
    W, H, rows = K1_SHAPES[shape]
    _k1_alone(hip_lib, oracle, how, W, H, rows, first=31 * shape)


@pytest.mark.parametrize("shape", [5, 3])
@pytest.mark.parametrize("how", ["reupload", "moved_instances"])
def test_gradient_first_after_a_reupload_or_a_move(hip_lib, oracle, how, shape):
    """the two calls besides the first upload that leave the tables stale.  A changed ubo.model is not a third: it reaches the
    library only as an argument of rtpt_gbuffer, which rebuilds the tables in the same call, so K1 never arrives first after it
    (the stand-alone k_gradient behind a turned model: test_bounds_follow_the_pose, route no_filter_fusion)"""
    W, H, rows = K1_SHAPES[shape]
    _k1_alone(hip_lib, oracle, how, W, H, rows, first=7 + 31 * shape)


def test_gradient_first_defines_an_unwritten_lut_prev(hip_lib, oracle):
    """no RTPT_PLANE_LUT_PREV either: K1 as the first pass defines it as the LUT it has just built (D3, as rtpt_gbuffer does)"""
    T = G.K1_T
    soup = FP.soup(T)
    W, H = G.MAIN_SHAPE
    for pcls in ("moved", "rest"):
        r = _k1_reference(oracle, soup, W, H, None, ("on", "equal", pcls), ("K1", False, W, H, None, ("on", "equal", pcls)))
        with hip_lib.Context(hip_lib.config_default(W, H)) as ctx:
            ctx.scene_upload(*FP.mesh_of(soup))
            ctx.set_plane(hip_lib.PLANE_VIS_ID, FP.check_ids(r["ids"], T))
            ctx.set_plane(hip_lib.PLANE_WORLDPOS, r["wp"])
            ctx.temporal_gradient(_push_constants(hip_lib.PushConstants, r["values"], 0))
            same_bits(ctx.readback(hip_lib.PLANE_GRADIENT), r["grad"], ("LUT_PREV never written", pcls))
            same_bits(ctx.readback(hip_lib.PLANE_LUT_PREV), r["lut"], ("LUT_PREV is the LUT", pcls))
