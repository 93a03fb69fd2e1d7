"""The device-side BVH build (csrc/bvh_build.hip, RTPT_FLAG_DEVICE_BVH_BUILD / RTPT_DEVICE_BVH=1) and rtpt_scene_rebuild.

Closest hit = min over (t, id) of one ray-triangle routine, boxes only cull and order (D4): any valid tree must give the
same bits.  So the checkers are the ones the host-built tree already answers to — rtpt_debug_bvh_check for the
structure, the oracle's brute force (through the unmodified cases of test_traversal_gpu.py) for the rays, the oracle's
frames and the host-built context's planes for whole frames.  Every test first asserts on a context of its own that the
tree really was built on the device (or that the stated fallback was taken): without the feature the flag and the
variable are ignored and the entry point does not exist.
"""
import os
import subprocess

import numpy as np
import pytest

import test_traversal_gpu as T
from conftest import bits

pytestmark = pytest.mark.gpu

F32 = np.float32
CLEAN = ("bad_refs_to_triangles", "boxes_not_containing", "boxes_beyond_scene", "dangling")
STRIP_KEYS = [(), ("E",), ("J",), ()]  # the camera and light script of the strip tests (test_fullsize_gpu.py)


def _upload(hip_lib, xyz, idx, xf=None, flags=0):
    c = hip_lib.config_default(64, 64)
    c.flags = flags
    ctx = hip_lib.Context(c)
    ctx.scene_upload(xyz, idx, xf)
    return ctx


def _assert_clean(st, info, n_tris, tag):
    assert all(st[k] == 0 for k in CLEAN), (tag, st)
    assert st["largest_leaf"] <= 2, (tag, st)
    assert st["nodes"] == info["n_nodes"], (tag, st, info)
    # info.depth counts like the host builder: the level of the deepest leaf, the root pair's children at 1; the check
    # reports the level of the deepest node
    assert info["depth"] == st["depth"] + (1 if info["n_primitives"] >= 2 else 0) and info["depth"] < 48, (tag, st, info)
    assert st["leaves"] == info["n_primitives"], (tag, st, info)


def _assert_device_tree(hip_lib, xyz, idx, xf=None, flags=0, tag=""):
    """one upload of the scene under the current environment / flags: the tree on the device was built there"""
    with _upload(hip_lib, xyz, idx, xf, flags) as ctx:
        info = ctx.scene_build_info()
        assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, (tag, info)
        return info


def _structure_cases(cornell):
    cases = {}
    for i, name in enumerate(T.SCENES):
        cases[name] = T.SCENES[name](np.random.default_rng([101, 0, i])) + (0,)
    cases["duplicates"] = T._duplicates(np.random.default_rng(404)) + (0,)
    for n in (1, 2, 3, 64, 65, 66):
        for force in (0, 2):
            cases[f"n={n} flags={force}"] = T._soup(np.random.default_rng([202, n]), n, size=0.15) + (force,)
            if n % 2 == 0:
                hx, hi = T._heightfield(8)
                cases[f"pairs n={n} flags={force}"] = (hx, hi[:n], force)
    cases["cornell"] = (cornell[0], cornell[1], 0)
    return cases


# ------------------------------------------------------------------------------ 1. structure
def test_structure_of_device_built_trees(hip_lib, oracle, cornell):
    D = hip_lib.FLAG_DEVICE_BVH_BUILD
    for tag, (xyz, idx, flags) in _structure_cases(cornell).items():
        tris = oracle.flatten(xyz, idx)
        seen = []
        for _ in range(2):
            with _upload(hip_lib, xyz, idx, flags=flags | D) as ctx:
                info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
            assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, (tag, info)
            _assert_clean(st, info, len(tris), tag)
            paired = T._pair_ok(tris)
            assert info["leaf_pairs"] == int(paired), (tag, info)
            assert info["n_primitives"] == (len(tris) // 2 if paired else len(tris)), (tag, info)
            assert info["build_ms"] > 0 and info["upload_ms"] > 0, (tag, info)
            seen.append((st, {k: v for k, v in info.items() if not k.endswith("_ms")}))
        assert seen[0] == seen[1], (tag, "the same scene built twice", seen)
        with _upload(hip_lib, xyz, idx, flags=flags) as ctx:
            info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
        assert info["builder"] == hip_lib.BVH_BUILDER_HOST_SAH and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, (tag, info)
        assert all(st[k] == 0 for k in CLEAN) and st["nodes"] == info["n_nodes"], (tag, st, info)


def test_environment_switch_sets_the_flag(hip_lib, monkeypatch):
    xyz, idx = T._soup(np.random.default_rng(1), 500)
    with _upload(hip_lib, xyz, idx) as ctx:
        assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_HOST_SAH
    monkeypatch.setenv("RTPT_DEVICE_BVH", "1")
    _assert_device_tree(hip_lib, xyz, idx)
    monkeypatch.setenv("RTPT_DEVICE_BVH", "0")
    with _upload(hip_lib, xyz, idx) as ctx:
        assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_HOST_SAH


def test_build_info_and_rebuild_need_a_scene(hip_lib):
    with hip_lib.Context(hip_lib.config_default(64, 64)) as ctx:
        for call in (ctx.scene_build_info, ctx.scene_rebuild):
            with pytest.raises(hip_lib.RtptError) as e:
                call()
            assert e.value.code == hip_lib.RTPT_E_NO_SCENE


# ------------------------------------------------------------------------------ 2. closest hit against the oracle
# The cases, seeds, families, floors and exclusions are test_traversal_gpu.py's own: its test functions are called as they
# are, with RTPT_DEVICE_BVH=1 in the environment of every context their check_case creates (it fixes cfg.flags itself).
@pytest.fixture
def device_env(monkeypatch):
    monkeypatch.setenv("RTPT_DEVICE_BVH", "1")
    return monkeypatch


@pytest.mark.parametrize("seed", T.SEEDS)
@pytest.mark.parametrize("scene", list(T.SCENES))
def test_closest_hit_scene_families(hip_lib, oracle, device_env, scene, seed):
    xyz, idx = T.SCENES[scene](np.random.default_rng([101, seed, list(T.SCENES).index(scene)]))
    _assert_device_tree(hip_lib, xyz, idx, tag=scene)
    T.test_scene_families(hip_lib, oracle, device_env, scene, seed)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 66])
def test_closest_hit_counts_around_the_brute_force_switch(hip_lib, oracle, device_env, n):
    _assert_device_tree(hip_lib, *T._soup(np.random.default_rng([202, n]), n, size=0.15), flags=2, tag=f"n={n}")
    if n % 2 == 0:
        hx, hi = T._heightfield(8)
        assert _assert_device_tree(hip_lib, hx, hi[:n], flags=2, tag=f"pairs n={n}")["leaf_pairs"] == 1
    T.test_counts_around_the_brute_force_switch(hip_lib, oracle, device_env, n)


def _scaled_soup(oracle, scale):
    """test_traversal_gpu.test_scale_extremes' scene and rays: the soup and its ray families scaled together"""
    rng = np.random.default_rng([303, 100 + int(np.log10(scale))])
    xyz, idx = T._soup(rng, 2000)
    fams = T.ray_families(oracle.flatten(xyz, idx), rng)
    s = F32(scale)
    return (xyz * s).astype(F32), idx, {k: (r * s).astype(F32) for k, r in fams.items()}


@pytest.mark.parametrize("scale", [1e-13, 1e13])
def test_closest_hit_scale_extremes(hip_lib, oracle, device_env, scale):
    """test_traversal_gpu.test_scale_extremes under the device build.  At 1e13 it is that test as it stands.  At 1e-13 its
    `tiny_components` family is left to test_known_gap_subnormal_triple_products below (one ray of its 2,000, a finding of
    this file: DESIGN.md 4, K2/K0, gap 3) and every other family — 8,000 rays — runs here with that test's seeds and
    floors; the tree itself is checked clean, so the ray is not lost to a box that fails to hold its triangle."""
    xyz, idx, fams = _scaled_soup(oracle, scale)
    with _upload(hip_lib, xyz, idx) as ctx:
        info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
    assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, info
    _assert_clean(st, info, 2000, f"scale {scale:g}")
    if scale > 1:
        T.test_scale_extremes(hip_lib, oracle, device_env, scale)
        return
    del fams["tiny_components"]
    assert list(fams) == ["random", "aimed", "on_surface", "axis"]
    T.check_case(hip_lib, oracle, device_env, f"scale {scale:g}", xyz, idx, fams, floors={"aimed": 200, "random": 50})
    tris = oracle.flatten(xyz, idx).astype(np.float64)
    n = np.cross(tris[:, 3:6] - tris[:, :3], tris[:, 6:9] - tris[:, :3])
    assert ((np.abs(n).max(1) * float(scale)) < np.finfo(F32).tiny).mean() > 0.5, "the triple products should be subnormal at this scale"


@pytest.mark.xfail(strict=True, reason="open D4 gap 3, found by this file (DESIGN.md 4, K2/K0): at scale 1e-13 every triple product of the "
                   "ray-triangle routine is subnormal, and for a ray with two direction components of 1e-38 it accepts a hit whose "
                   "point lies outside the triangle's own box; the leaf box of the device-built tree culls it")
def test_known_gap_subnormal_triple_products(hip_lib, oracle, device_env):
    """Where a device-built tree and the brute force disagree, and the host-built tree happens not to: the `tiny_components`
    family of test_scale_extremes' soup at scale 1e-13, 1 ray of 2,000 (#709 of the family, #8709 of the case):
    o = (1.6207730e-14, 8.3033335e-15, -2.6675936e-14), d = (1e-38, -6.5939464e-17, 1e-38).  The brute force reports
    triangle 211 at t = 98.0 — d.n is 1-2 units of the smallest subnormal, t a ratio of two such integers — a point 7 % of the
    triangle's extent (918 box paddings) outside the triangle's box; the BVH culls the one-triangle leaf (left child of node
    1169, level 10) and reports triangle 16 at t = 132.5, which the ray does pass through.  Every box holds its triangles
    (test_closest_hit_scale_extremes checks it), so this is the routine accepting a ray it geometrically misses — the
    class of test_known_gaps' first gap; no box margin bounds it.  Strict: when the gap is closed this passes, and the
    marker must go."""
    xyz, idx, fams = _scaled_soup(oracle, 1e-13)
    _assert_device_tree(hip_lib, xyz, idx, tag="scale 1e-13")
    T.check_case(hip_lib, oracle, device_env, "scale 1e-13 known gap", xyz, idx, {"tiny_components": fams["tiny_components"]})


def test_closest_hit_duplicates_and_coplanar_overlaps(hip_lib, oracle, device_env):
    rng = np.random.default_rng(404)
    _assert_device_tree(hip_lib, *T._duplicates(rng), tag="duplicates")
    eye = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32), (2, 1))
    _assert_device_tree(hip_lib, *T._soup(rng, 1500), xf=eye, tag="two identity instances")
    T.test_duplicates_and_coplanar_overlaps(hip_lib, oracle, device_env)


@pytest.mark.parametrize("dist", [10, 100, 1000, 5000])
def test_closest_hit_distant_origins(hip_lib, oracle, device_env, dist):
    for name, (xyz, idx) in (("soup", T._soup(np.random.default_rng([505, dist]), 3000, lo=-0.3, hi=0.3)),
                             ("heightfield", T._heightfield(24)), ("sphere", T._sphere())):
        _assert_device_tree(hip_lib, xyz, idx, tag=name)
    T.test_distant_origins(hip_lib, oracle, device_env, dist)


def test_closest_hit_small_ray_tmax(hip_lib, oracle, device_env):
    _assert_device_tree(hip_lib, *T._soup(np.random.default_rng(606), 3000, lo=-2.0, hi=2.0, size=0.1), tag="ray_tmax=3")
    T.test_small_ray_tmax(hip_lib, oracle, device_env)


def test_height_numbering_switch_gives_a_valid_tree_and_the_same_hits(hip_lib, oracle, device_env):
    """RTPT_LBVH_ORDER=height (A/B switch): the device tree's nodes numbered by descending height instead of
    pre-order — still every child behind its parent and node 0 the root, the same counts, the oracle's hits"""
    device_env.setenv("RTPT_LBVH_ORDER", "height")
    for i, scene in enumerate(("soup", "sphere")):
        rng = np.random.default_rng([909, i])
        xyz, idx = T.SCENES[scene](rng)
        tris = oracle.flatten(xyz, idx)
        with _upload(hip_lib, xyz, idx) as ctx:
            info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
        assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH, info
        _assert_clean(st, info, len(tris), scene)
        with device_env.context() as mp:
            mp.delenv("RTPT_LBVH_ORDER")
            with _upload(hip_lib, xyz, idx) as ctx:
                info2, st2 = ctx.scene_build_info(), ctx.debug_bvh_check()
        assert st == st2 and {k: v for k, v in info.items() if not k.endswith("_ms")} == {k: v for k, v in info2.items() if not k.endswith("_ms")}
        T.check_case(hip_lib, oracle, device_env, f"{scene} numbered by height", xyz, idx, T.ray_families(tris, rng), floors={"aimed": 200})


# ------------------------------------------------------------------------------ 3. frames against the oracle, refit of a device tree
@pytest.mark.parametrize("scene", ["heightfield", "soup"])
def test_posed_frames_of_a_device_tree_match_oracle(hip_lib, oracle, scene):
    """test_traversal_gpu.test_posed_frames_match_oracle with the tree built on the device: two rotating model matrices,
    so the device-built topology is refit twice"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import HipBackend, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan
    if scene == "heightfield":
        xyz, idx = T._heightfield(20)
        xyz = (xyz * F32(2.0) + np.array([0, 1.0, 0], F32)).astype(F32)
    else:
        xyz, idx = T._soup(np.random.default_rng(707), 3000, lo=-0.8, hi=0.8, size=0.08)
        xyz = (xyz + np.array([0, 1.0, 0], F32)).astype(F32)
    w, h, seg, n = 96, 64, 3, 3
    be = HipBackend(w, h, StripPlan(h, 1, 0, n), max_segments=seg, flags=hip_lib.FLAG_EXACT_FILTER | hip_lib.FLAG_DEVICE_BVH_BUILD,
                    debug_mask=hip_lib.DEBUG_HIT_ID)
    app = PathTracingApplication(be, w, h, n)
    app.objVertices, app.objIndices = xyz, idx
    app.buildAccelerationStructure()
    tris = oracle.flatten(xyz, idx)
    ref = oracle.OracleApp(w, h, tris, max_segments=seg, iterations=n)
    ctx = be.ctx
    try:
        info = ctx.scene_build_info()
        assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, info
        for f, m in enumerate([T._rot(0.7, 0.4, (0.0, 0.3, 0.0)), T._rot(0.75, 0.55, (0.05, 0.25, -0.1))]):
            app.modelMatrix = m
            ref.model = m
            app.updateScene(())
            app.drawVisbilityBuffer()
            app.computeTemporalGradient()
            app.drawSceneToImage()
            vis, hit = ctx.readback(hip_lib.PLANE_VIS_ID), ctx.readback(hip_lib.PLANE_HIT_ID)
            depth, traced = ctx.readback(hip_lib.PLANE_DEPTH), ctx.readback(hip_lib.PLANE_IMAGE)
            app.applyTemporalFiltering()
            app.copyImageToSwapChainsCurrentImage()
            app.frameCount += 1
            fo = ref.draw_scene()
            assert (vis > 0).mean() > 0.2, (scene, f, "the frame must show the geometry")
            assert np.array_equal(vis, fo.vis), (scene, f, int((vis != fo.vis).sum()))
            assert np.array_equal(hit, fo.hit_id), (scene, f, int((hit != fo.hit_id).sum()))
            assert np.array_equal(bits(depth), bits(fo.depth)), (scene, f)
            assert np.array_equal(bits(traced), bits(fo.traced)), (scene, f)
            _assert_clean(ctx.debug_bvh_check(), ctx.scene_build_info(), len(tris), (scene, f))
    finally:
        be.close()


# ------------------------------------------------------------------------------ 4. frames against the host-built tree
def _planes(hip_lib):
    A = hip_lib
    return {"image": A.PLANE_IMAGE, "filtered": A.PLANE_FILTERED, "previous": A.PLANE_PREVIOUS, "worldpos": A.PLANE_WORLDPOS,
            "gradient": A.PLANE_GRADIENT, "depth": A.PLANE_DEPTH, "vis": A.PLANE_VIS_ID, "prev_vis": A.PLANE_PREV_VIS_ID,
            "lut": A.PLANE_LUT, "lut_prev": A.PLANE_LUT_PREV, "hit_id": A.PLANE_HIT_ID, "prev_pixel": A.PLANE_PREV_PIXEL}


def _read_all(hip_lib, ctx):
    out = {name: ctx.readback(p) for name, p in _planes(hip_lib).items()}
    out["rays"] = np.array([ctx.raycount()], np.uint64)
    return out


def _assert_same_planes(got, want, tag):
    for name in want:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (tag, name)


def _small_scenes(cornell):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import scenes
    vx, ti, xf, cam, zfar = scenes.instanced_cornell(cornell[0], cornell[1], lattice=(3, 3, 3), tess=2)
    return {"cornell": (2, {}),  # RTPT_FLAG_FORCE_BVH
            "lattice": (0, dict(mesh=(vx, ti), instance_xforms=xf, cameraOrigin=cam, z_far=zfar,
                                lightPos=(1.0, float(cam[1]), float(cam[2]) - 8.0)))}


@pytest.mark.parametrize("scene", ["cornell", "lattice"])
def test_frames_of_a_device_tree_equal_the_host_trees(hip_lib, cornell, scene):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    force, kw = _small_scenes(cornell)[scene]
    w, h = 192, 128
    base = hip_lib.FLAG_EXACT_FILTER | force
    runs = []
    for flags in (base | hip_lib.FLAG_DEVICE_BVH_BUILD, base):
        app = make_app(w, h, max_segments=4, iterations=5, flags=flags, debug_mask=hip_lib.DEBUG_HIT_ID | hip_lib.DEBUG_PREV_PIXEL, **kw)
        ctx = app.backend.ctx
        try:
            info = ctx.scene_build_info()
            want = hip_lib.BVH_BUILDER_DEVICE_LBVH if flags & hip_lib.FLAG_DEVICE_BVH_BUILD else hip_lib.BVH_BUILDER_HOST_SAH
            assert info["builder"] == want and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, info
            if scene == "lattice":
                assert info["n_primitives"] > 64 and info["leaf_pairs"] == 1, info
            frames = []
            for keys in STRIP_KEYS:
                app.drawScene(keys)
                frames.append(_read_all(hip_lib, ctx))
            runs.append(frames)
        finally:
            app.backend.close()
    assert (runs[1][-1]["prev_vis"] > 0).mean() > 0.2 and runs[1][-1]["rays"][0] > w * h
    for f, (dev, host) in enumerate(zip(*runs)):
        _assert_same_planes(dev, host, (scene, f))


@pytest.mark.parametrize("mode", ["redundant", "exchange"])
@pytest.mark.parametrize("scene", ["cornell", "lattice"])
def test_two_strips_with_device_trees_equal_the_single_context(hip_lib, cornell, scene, mode):
    """two strip contexts, each with a device-built tree, against the single device-tree context — which the test above
    ties to the host-built one — every pixel of four frames, bit for bit"""
    from test_parity_gpu import _strips_vs_single
    force, kw = _small_scenes(cornell)[scene]
    flags = hip_lib.FLAG_EXACT_FILTER | force | hip_lib.FLAG_DEVICE_BVH_BUILD
    if scene == "cornell":
        _assert_device_tree(hip_lib, cornell[0], cornell[1], flags=flags)
    else:
        _assert_device_tree(hip_lib, *kw["mesh"], xf=kw["instance_xforms"], flags=flags)
    _strips_vs_single(192, 128, 4, 5, 2, mode, flags, STRIP_KEYS, **kw)


def test_brute_force_scene_with_a_device_tree_follows_the_model(hip_lib, cornell):
    """the Cornell box without FORCE_BVH traces by brute force and re-poses on the host; its (unused) device-built tree has
    no host copy and must be refit on the device: no error, the flag-clear context's frames, a clean tree after each"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    w, h = 160, 96
    models = [None, T._rot(0.3, 0.5, (0.1, 0.0, -0.2)), T._rot(-0.2, 0.9, (0.0, 0.2, 0.1))]
    runs = []
    for flags in (hip_lib.FLAG_EXACT_FILTER | hip_lib.FLAG_DEVICE_BVH_BUILD, hip_lib.FLAG_EXACT_FILTER):
        app = make_app(w, h, max_segments=4, iterations=5, flags=flags, debug_mask=hip_lib.DEBUG_HIT_ID | hip_lib.DEBUG_PREV_PIXEL)
        ctx = app.backend.ctx
        try:
            info = ctx.scene_build_info()
            if flags & hip_lib.FLAG_DEVICE_BVH_BUILD:
                assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["n_primitives"] <= 64, info
            frames = []
            for m in models:
                if m is not None:
                    app.modelMatrix = m
                app.drawScene(())
                frames.append(_read_all(hip_lib, ctx))
                st = ctx.debug_bvh_check()
                assert all(st[k] == 0 for k in CLEAN), (flags, st)
            runs.append(frames)
        finally:
            app.backend.close()
    assert not np.array_equal(runs[1][0]["prev_vis"], runs[1][1]["prev_vis"]), "the model did move the scene"
    for f, (dev, host) in enumerate(zip(*runs)):
        _assert_same_planes(dev, host, f)


# ------------------------------------------------------------------------------ 5. full size
def _fullsize_rays(tris, n=200_000):
    rng = np.random.default_rng(20250505)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    q = n // 4
    span = hi - lo
    rnd = np.concatenate([rng.uniform(lo - 0.2 * span, hi + 0.2 * span, (q, 3)), T._unit(rng.normal(size=(q, 3)))], 1)
    eye = np.array([0.0, float((lo[1] + hi[1]) / 2), float(hi[2] + 0.6 * span[1] / 0.2027)])
    tgt = rng.uniform(lo, hi, (q, 3))
    prim = np.concatenate([np.tile(eye, (q, 1)), T._unit(tgt - eye)], 1)
    axis = np.zeros((q, 6))
    axis[:, :3] = rng.uniform(lo - 0.1 * span, hi + 0.1 * span, (q, 3))
    axis[np.arange(q), 3 + rng.integers(0, 3, q)] = rng.choice([-1.0, 1.0], q)
    nan = rnd[rng.permutation(q)].copy()
    nan[np.arange(q), rng.integers(0, 6, q)] = np.nan
    return np.ascontiguousarray(np.concatenate([rnd, prim, axis, nan]).astype(F32))


def test_million_triangle_scene_built_on_the_device(hip_lib, oracle, cornell):
    """BASELINE configs[4] (3840 x 2160, 8 segments, 1,152,000 triangles): the device build against the host-built
    context (which test_fullsize_gpu.py ties to the oracle) — 200,000 rays and every plane of one frame bit for bit —
    and the one timing condition: the whole upload with the device build is faster than with the host build, both
    measured in this process after a warm-up upload that loads the builder's code objects.

    Measured on the MI355X: see DESIGN.md 4 (K2/K0, "device build")."""
    import test_fullsize_gpu as FS
    scene = FS._instanced(oracle, cornell)
    vx, ti, xf, cam, zfar = scene
    tris = oracle.flatten(vx, ti, xf)
    assert len(tris) == 1_152_000
    rays = _fullsize_rays(tris)
    X, D = hip_lib.FLAG_EXACT_FILTER, hip_lib.FLAG_DEVICE_BVH_BUILD
    _assert_device_tree(hip_lib, *T._soup(np.random.default_rng(5), 2000), flags=D, tag="warm-up")
    out = {}
    for name, flags in (("device", X | D), ("host", X)):
        app = FS._make_instanced_app(hip_lib, scene, flags)
        ctx = app.backend.ctx
        try:
            info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
            print(f"configs[4] {name} build: {info}")
            if name == "device":
                assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, info
                assert info["n_primitives"] == 576_000 and info["leaf_pairs"] == 1, info
                _assert_clean(st, info, len(tris), name)
            else:
                assert info["builder"] == hip_lib.BVH_BUILDER_HOST_SAH, info
            ids, ts = ctx.selftest_trace(rays)
            app.drawScene(())
            out[name] = (info, ids, ts, _read_all(hip_lib, ctx))
        finally:
            app.backend.close()
    dev, host = out["device"], out["host"]
    q = len(rays) // 4
    assert (host[1][:q] > 0).sum() > q // 20 and (host[1][q:2 * q] > 0).sum() > q // 4 and (host[1][2 * q:3 * q] > 0).sum() > q // 20
    assert np.array_equal(dev[1], host[1]) and np.array_equal(bits(dev[2]), bits(host[2])), \
        T._first_mismatch("configs[4] rays", rays, dev[1], dev[2], host[1], host[2])
    assert (host[3]["prev_vis"] > 0).mean() > 0.2
    _assert_same_planes(dev[3], host[3], "configs[4] frame")
    assert dev[0]["upload_ms"] < host[0]["upload_ms"], (dev[0], host[0])


# ------------------------------------------------------------------------------ 6. fallback
def _chain_scene():
    """66 triangles whose Morton keys differ in their leading bits one by one: for each axis a and k = 0 .. 21 one with
    vertices c, c + 2^-26 e_(a+1), c + 2^-26 e_(a+2), c = 2^-k e_a.  The radix tree over them is a chain deeper than
    the 48-entry traversal stack; the host's SAH builder gives depth 15."""
    e = np.eye(3, dtype=F32)
    h = F32(2.0 ** -26)
    tr = []
    for a in range(3):
        for k in range(22):
            c = (F32(2.0 ** -k) * e[a]).astype(F32)
            tr.append([c, c + h * e[(a + 1) % 3], c + h * e[(a + 2) % 3]])
    xyz = np.array(tr, F32).reshape(-1, 3)
    return xyz, np.arange(len(xyz), dtype=np.uint32).reshape(-1, 3)


def test_tree_deeper_than_the_stack_falls_back_to_the_host_builder(hip_lib, oracle):
    xyz, idx = _chain_scene()
    tris = oracle.flatten(xyz, idx)
    assert len(tris) == 66
    rays = T.ray_families(tris, np.random.default_rng(808))["aimed"]
    cfg = hip_lib.config_default(64, 64)
    wid, wts = oracle.trace_rays(tris, rays, tmax=cfg.ray_tmax)
    assert (wid > 0).sum() >= 100
    with _upload(hip_lib, xyz, idx, flags=hip_lib.FLAG_DEVICE_BVH_BUILD) as ctx:
        info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
        assert info["builder"] == hip_lib.BVH_BUILDER_HOST_SAH and info["fallback"] == hip_lib.BVH_FALLBACK_DEPTH, info
        assert all(st[k] == 0 for k in CLEAN) and info["depth"] < 48, (st, info)
        ids, ts = ctx.selftest_trace(rays)
        assert T._first_mismatch("chain scene", rays, ids, ts, wid, wts) is None
        # the same radix tree is refused by a rebuild, and the host tree stays
        with pytest.raises(hip_lib.RtptError) as e:
            ctx.scene_rebuild()
        assert e.value.code == hip_lib.RTPT_E_INVALID
        assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_HOST_SAH
        ids, ts = ctx.selftest_trace(rays)
        assert T._first_mismatch("chain scene after the refused rebuild", rays, ids, ts, wid, wts) is None


# ------------------------------------------------------------------------------ 7. rebuild
def _shear():
    m = np.eye(4)
    m[:3, :3] = [[1.0, 1.7, 0.0], [0.0, 1.0, 0.0], [0.9, 0.0, 1.0]]
    m[:3, 3] = (0.0, 0.1, 0.0)
    return np.ascontiguousarray(m.astype(F32).T).ravel()  # column-major


@pytest.mark.parametrize("uploaded_by", ["host", "device"])
def test_rebuild_changes_cost_only(hip_lib, uploaded_by):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import HipBackend, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan
    xyz, idx = T._soup(np.random.default_rng(707), 3000, lo=-0.8, hi=0.8, size=0.08)
    xyz = (xyz + np.array([0, 1.0, 0], F32)).astype(F32)
    w, h, seg, n = 128, 96, 3, 5
    flags = hip_lib.FLAG_EXACT_FILTER | (hip_lib.FLAG_DEVICE_BVH_BUILD if uploaded_by == "device" else 0)
    apps = []
    for _ in range(2):
        be = HipBackend(w, h, StripPlan(h, 1, 0, n), max_segments=seg, flags=flags, debug_mask=hip_lib.DEBUG_HIT_ID | hip_lib.DEBUG_PREV_PIXEL)
        app = PathTracingApplication(be, w, h, n)
        app.objVertices, app.objIndices = xyz, idx
        app.buildAccelerationStructure()
        apps.append(app)
    a, b = apps  # a rebuilds, b never does
    try:
        want = hip_lib.BVH_BUILDER_DEVICE_LBVH if uploaded_by == "device" else hip_lib.BVH_BUILDER_HOST_SAH
        assert a.backend.ctx.scene_build_info()["builder"] == want
        models = [_shear(), T._rot(0.7, 0.4, (0.0, 0.3, 0.0)), T._rot(0.75, 0.55, (0.05, 0.25, -0.1))]
        for f, m in enumerate(models):
            for app in apps:
                app.modelMatrix = m
                app.drawScene(())
            pa, pb = _read_all(hip_lib, a.backend.ctx), _read_all(hip_lib, b.backend.ctx)
            assert (pb["prev_vis"] > 0).mean() > 0.1, f  # the frame just ended
            _assert_same_planes(pa, pb, (uploaded_by, f))
            st = a.backend.ctx.debug_bvh_check()  # f == 1: the rebuilt tree, refit once to the rotated model
            assert all(st[k] == 0 for k in CLEAN), (f, st)
            if f == 0:
                a.backend.ctx.scene_rebuild()  # over the triangles as posed by the shear
                info, st = a.backend.ctx.scene_build_info(), a.backend.ctx.debug_bvh_check()
                assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, info
                assert info["n_primitives"] == 3000 and info["build_ms"] > 0 and info["upload_ms"] > 0, info
                _assert_clean(st, info, 3000, "after the rebuild")
            if f == 1:  # history and LUT_PREV survived the rebuild
                assert np.abs(pb["gradient"]).max() > 0 and np.abs(pb["lut_prev"]).max() > 0
        assert b.backend.ctx.scene_build_info()["builder"] == want
    finally:
        for app in apps:
            app.backend.close()


# ------------------------------------------------------------------------------ 8. C++ host
def test_cpp_host_device_bvh_switch(hip_lib, tmp_path):
    from test_cpp_host import APP, PKG
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    outs = {}
    for name, extra in (("device", ["--device-bvh"]), ("host", [])):
        pfm = tmp_path / f"{name}.pfm"
        out = subprocess.run([APP, "--width", "160", "--height", "96", "--segments", "4", "--iterations", "5", "--lattice", "3x3x3",
                              "--tessellate", "2", "--frames", "3", "--dump", str(pfm)] + extra, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        outs[name] = (out.stdout, pfm.read_bytes())
    assert "built by device LBVH" in outs["device"][0] and "built by host SAH" in outs["host"][0], outs["device"][0]
    assert len(outs["host"][1]) > 160 * 96 * 12 and outs["device"][1] == outs["host"][1]
