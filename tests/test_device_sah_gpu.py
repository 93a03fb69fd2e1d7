"""The device SAH builder (csrc/bvh_build_sah.hip, RTPT_FLAG_DEVICE_BVH_BUILD | RTPT_FLAG_DEVICE_BVH_SAH, RTPT_DEVICE_BVH=sah).

It restates the host's binned-SAH builder level by level, and the host's tree is a function of the triangle set, so the
first check is exact: the child references of every node and the leaf order, read back from the device with
rtpt_debug_bvh_topology, equal those of the host-built context (the leaf order after sorting the ids inside each leaf —
the two triangles of a triangle-mode leaf stand in the order an unstable partition left them in).  The LBVH's tree of the
same scenes differs, so the comparison discriminates.  Then the checks every tree answers to (test_device_bvh_gpu.py):
rtpt_debug_bvh_check, the unmodified closest-hit cases of test_traversal_gpu.py against the oracle's brute force, whole
frames against the host-built context and the oracle, rebuilds, the full-size scene, the C++ host.  Every test asserts on
a context of its own that the tree was built by the device SAH builder: without the feature the flag bit and the value
"sah" are ignored."""
import os
import subprocess

import numpy as np
import pytest

import test_device_bvh_gpu as B
import test_traversal_gpu as T
from conftest import bits
from test_device_bvh_gpu import CLEAN, STRIP_KEYS, _assert_same_planes, _read_all, _upload
from test_device_sah_cpu import deep_scene, stack_of_duplicates

pytestmark = pytest.mark.gpu

F32 = np.float32
SAH = 0x3000  # RTPT_FLAG_DEVICE_BVH_BUILD | RTPT_FLAG_DEVICE_BVH_SAH
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF


def _canonical(refs, leaf):
    """the leaf order with the ids inside each two-triangle leaf sorted"""
    out = leaf.copy()
    r = refs.reshape(-1)
    r = r[(r != EMPTY) & ((r & LEAF) != 0)]
    for f in ((r & 0x7FFFFFFF) >> 2)[(r & 3) == 1]:
        out[f:f + 2] = np.sort(out[f:f + 2])
    return out


def _topology(ctx):
    refs, leaf = ctx.debug_bvh_topology()
    return refs, _canonical(refs, leaf)


def _same_tree(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _assert_sah_info(hip_lib, info, tag=""):
    assert info["builder"] == hip_lib.BUILDER_DEVICE_SAH == 2 and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, (tag, info)


def _assert_sah_tree(hip_lib, xyz, idx, xf=None, flags=0, tag=""):
    """one upload of the scene under the current environment / flags: the tree on the device was built by the device SAH builder"""
    with _upload(hip_lib, xyz, idx, xf, flags) as ctx:
        info = ctx.scene_build_info()
        _assert_sah_info(hip_lib, info, tag)
        return info


def _assert_clean(st, info, tag):
    assert all(st[k] == 0 for k in CLEAN), (tag, st)
    assert st["largest_leaf"] <= 2, (tag, st)
    assert st["nodes"] == info["n_nodes"], (tag, st, info)


def _scaled_soup(scale):
    rng = np.random.default_rng([303, 100 + int(np.log10(scale))])
    xyz, idx = T._soup(rng, 2000)
    return (xyz * F32(scale)).astype(F32), idx


def _small_lattice(cornell):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import scenes
    vx, ti, xf, cam, zfar = scenes.instanced_cornell(cornell[0], cornell[1], lattice=(3, 3, 3), tess=2)
    return vx, ti, xf


def _topology_cases(cornell):
    cases = {tag: (xyz, idx, None, flags) for tag, (xyz, idx, flags) in B._structure_cases(cornell).items()}
    cases["chain"] = B._chain_scene() + (None, 0)
    cases["deep"] = deep_scene() + (None, 0)
    cases["stack of duplicates"] = stack_of_duplicates() + (None, 0)
    cases["soup x 1e-13"] = _scaled_soup(1e-13) + (None, 0)
    cases["soup x 1e13"] = _scaled_soup(1e13) + (None, 0)
    cases["lattice"] = _small_lattice(cornell) + (0,)
    return cases


# ------------------------------------------------------------------------------ 1. topology equals the host's
def test_topology_equals_the_host_builders(hip_lib, oracle, cornell):
    differs_from_lbvh = {}
    for tag, (xyz, idx, xf, flags) in _topology_cases(cornell).items():
        seen = []
        for _ in range(2):
            with _upload(hip_lib, xyz, idx, xf, flags | SAH) as ctx:
                info, st, topo = ctx.scene_build_info(), ctx.debug_bvh_check(), _topology(ctx)
                raw = ctx.debug_bvh_topology()
            _assert_sah_info(hip_lib, info, tag)
            _assert_clean(st, info, tag)
            assert info["build_ms"] > 0 and info["upload_ms"] > 0, (tag, info)
            seen.append((info, topo, raw))
        assert np.array_equal(seen[0][2][0], seen[1][2][0]) and np.array_equal(seen[0][2][1], seen[1][2][1]), (tag, "the same scene built twice")
        with _upload(hip_lib, xyz, idx, xf, flags) as ctx:
            hinfo, htopo = ctx.scene_build_info(), _topology(ctx)
        assert hinfo["builder"] == hip_lib.BVH_BUILDER_HOST_SAH and hinfo["fallback"] == hip_lib.BVH_FALLBACK_NONE, (tag, hinfo)
        info, topo, _ = seen[0]
        for k in ("n_nodes", "depth", "n_primitives", "leaf_pairs"):
            assert info[k] == hinfo[k], (tag, k, info, hinfo)
        assert topo[0].shape == htopo[0].shape, (tag, topo[0].shape, htopo[0].shape)
        bad = np.nonzero((topo[0] != htopo[0]).any(1))[0]
        assert not len(bad), (tag, f"{len(bad)} of {len(topo[0])} nodes differ, first {bad[0]}", topo[0][bad[0]], htopo[0][bad[0]])
        assert np.array_equal(topo[1], htopo[1]), (tag, "leaf order")
        if tag == "chain":
            assert hinfo["depth"] == 15, hinfo
        if tag == "deep":
            assert hinfo["depth"] >= 24, hinfo
        if tag in ("soup", "lattice"):
            with _upload(hip_lib, xyz, idx, xf, flags | hip_lib.FLAG_DEVICE_BVH_BUILD) as ctx:
                assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH
                differs_from_lbvh[tag] = not _same_tree(_topology(ctx), htopo)
    assert differs_from_lbvh == {"soup": True, "lattice": True}, differs_from_lbvh


def test_environment_switch_and_lone_bit(hip_lib, monkeypatch):
    xyz, idx = T._soup(np.random.default_rng(1), 500)
    with _upload(hip_lib, xyz, idx, flags=hip_lib.FLAG_DEVICE_BVH_SAH) as ctx:  # alone the bit is ignored
        assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_HOST_SAH
    monkeypatch.setenv("RTPT_DEVICE_BVH", "sah")
    _assert_sah_tree(hip_lib, xyz, idx)
    monkeypatch.setenv("RTPT_DEVICE_BVH", "1")
    with _upload(hip_lib, xyz, idx) as ctx:
        assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH
    monkeypatch.setenv("RTPT_DEVICE_BVH", "0")
    with _upload(hip_lib, xyz, idx) as ctx:
        assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_HOST_SAH


def test_topology_needs_a_scene(hip_lib):
    with hip_lib.Context(hip_lib.config_default(64, 64)) as ctx:
        with pytest.raises(hip_lib.RtptError) as e:
            ctx.debug_bvh_topology()
        assert e.value.code == hip_lib.RTPT_E_NO_SCENE


# ------------------------------------------------------------------------------ 2. closest hit against the oracle
# test_traversal_gpu.py's test functions as they are, with RTPT_DEVICE_BVH=sah in the environment of every context
@pytest.fixture
def sah_env(monkeypatch):
    monkeypatch.setenv("RTPT_DEVICE_BVH", "sah")
    return monkeypatch


@pytest.mark.parametrize("seed", T.SEEDS)
@pytest.mark.parametrize("scene", list(T.SCENES))
def test_closest_hit_scene_families(hip_lib, oracle, sah_env, scene, seed):
    xyz, idx = T.SCENES[scene](np.random.default_rng([101, seed, list(T.SCENES).index(scene)]))
    _assert_sah_tree(hip_lib, xyz, idx, tag=scene)
    T.test_scene_families(hip_lib, oracle, sah_env, scene, seed)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 66])
def test_closest_hit_counts_around_the_brute_force_switch(hip_lib, oracle, sah_env, n):
    _assert_sah_tree(hip_lib, *T._soup(np.random.default_rng([202, n]), n, size=0.15), flags=2, tag=f"n={n}")
    if n % 2 == 0:
        hx, hi = T._heightfield(8)
        assert _assert_sah_tree(hip_lib, hx, hi[:n], flags=2, tag=f"pairs n={n}")["leaf_pairs"] == 1
    T.test_counts_around_the_brute_force_switch(hip_lib, oracle, sah_env, n)


@pytest.mark.parametrize("scale", [1e-13, 1e13])
def test_closest_hit_scale_extremes(hip_lib, oracle, sah_env, scale):
    """test_traversal_gpu.test_scale_extremes as it stands, `tiny_components` included.  The LBVH tree loses one ray of that
    family at 1e-13 (gap 3: the routine accepts a hit outside the triangle's own box, and a one-triangle leaf
    box culls it); the host-built tree happens to pass it, and this tree has the host's topology with device-refit boxes."""
    xyz, idx = _scaled_soup(scale)
    with _upload(hip_lib, xyz, idx) as ctx:
        info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
    _assert_sah_info(hip_lib, info, f"scale {scale:g}")
    _assert_clean(st, info, f"scale {scale:g}")
    T.test_scale_extremes(hip_lib, oracle, sah_env, scale)


def test_closest_hit_duplicates_and_coplanar_overlaps(hip_lib, oracle, sah_env):
    rng = np.random.default_rng(404)
    _assert_sah_tree(hip_lib, *T._duplicates(rng), tag="duplicates")
    eye = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32), (2, 1))
    _assert_sah_tree(hip_lib, *T._soup(rng, 1500), xf=eye, tag="two identity instances")
    T.test_duplicates_and_coplanar_overlaps(hip_lib, oracle, sah_env)


@pytest.mark.parametrize("dist", [10, 100, 1000, 5000])
def test_closest_hit_distant_origins(hip_lib, oracle, sah_env, dist):
    for name, (xyz, idx) in (("soup", T._soup(np.random.default_rng([505, dist]), 3000, lo=-0.3, hi=0.3)),
                             ("heightfield", T._heightfield(24)), ("sphere", T._sphere())):
        _assert_sah_tree(hip_lib, xyz, idx, tag=name)
    T.test_distant_origins(hip_lib, oracle, sah_env, dist)


def test_closest_hit_small_ray_tmax(hip_lib, oracle, sah_env):
    _assert_sah_tree(hip_lib, *T._soup(np.random.default_rng(606), 3000, lo=-2.0, hi=2.0, size=0.1), tag="ray_tmax=3")
    T.test_small_ray_tmax(hip_lib, oracle, sah_env)


def test_closest_hit_on_the_median_paths(hip_lib, oracle, sah_env):
    """the deep scene (median from depth 22) and the stack of duplicates (median at the root, the two-sort path).  The deep
    scene spans 2^165 on x, so rays aimed from a box around it meet nothing: its rays run along x from between two
    neighbouring triangles (x = 0.75 x 2^-k), through the footprint all of them share, and meet triangle k or k + 1"""
    xyz, idx = deep_scene()
    _assert_sah_tree(hip_lib, xyz, idx, tag="deep")
    rng = np.random.default_rng(111)
    n = 1000
    k = rng.integers(-39, 125, n)
    yz = rng.uniform(0.05, 0.45, (n, 2))
    o = np.stack([0.75 * np.ldexp(1.0, -k), yz[:, 0], yz[:, 1]], 1)
    d = np.zeros((n, 3))
    d[:, 0] = rng.choice([-1.0, 1.0], n)
    rays = np.ascontiguousarray(np.concatenate([o, d], 1).astype(F32))
    out = T.check_case(hip_lib, oracle, sah_env, "deep", xyz, idx, {"along_x": rays}, tmax=1e30, floors={"along_x": 900})
    assert len(np.unique(out["along_x"][0])) > 100, "the rays should end in many different leaves"
    xyz, idx = stack_of_duplicates()
    _assert_sah_tree(hip_lib, xyz, idx, tag="stack of duplicates")
    fams = T.ray_families(oracle.flatten(xyz, idx), rng, n=1000)
    T.check_case(hip_lib, oracle, sah_env, "stack of duplicates", xyz, idx, {f: fams[f] for f in ("random", "aimed")}, floors={"aimed": 100})


# ------------------------------------------------------------------------------ 3. frames
@pytest.mark.parametrize("scene", ["cornell", "lattice"])
def test_frames_equal_the_host_trees(hip_lib, cornell, scene):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    force, kw = B._small_scenes(cornell)[scene]
    w, h = 192, 128
    base = hip_lib.FLAG_EXACT_FILTER | force
    runs = []
    for flags in (base | SAH, base):
        app = make_app(w, h, max_segments=4, iterations=5, flags=flags, debug_mask=hip_lib.DEBUG_HIT_ID | hip_lib.DEBUG_PREV_PIXEL, **kw)
        ctx = app.backend.ctx
        try:
            info = ctx.scene_build_info()
            if flags & SAH:
                _assert_sah_info(hip_lib, info, scene)
            else:
                assert info["builder"] == hip_lib.BVH_BUILDER_HOST_SAH, info
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
def test_two_strips_equal_the_single_context(hip_lib, cornell, scene, mode):
    from test_parity_gpu import _strips_vs_single
    force, kw = B._small_scenes(cornell)[scene]
    flags = hip_lib.FLAG_EXACT_FILTER | force | SAH
    if scene == "cornell":
        _assert_sah_tree(hip_lib, cornell[0], cornell[1], flags=flags)
    else:
        _assert_sah_tree(hip_lib, *kw["mesh"], xf=kw["instance_xforms"], flags=flags)
    _strips_vs_single(192, 128, 4, 5, 2, mode, flags, STRIP_KEYS, **kw)


@pytest.mark.parametrize("scene", ["heightfield", "soup"])
def test_posed_frames_match_oracle(hip_lib, oracle, scene):
    """test_device_bvh_gpu.test_posed_frames_of_a_device_tree_match_oracle with the SAH flag: the topology is refit twice"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import HipBackend, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan
    if scene == "heightfield":
        xyz, idx = T._heightfield(20)
        xyz = (xyz * F32(2.0) + np.array([0, 1.0, 0], F32)).astype(F32)
    else:
        xyz, idx = T._soup(np.random.default_rng(707), 3000, lo=-0.8, hi=0.8, size=0.08)
        xyz = (xyz + np.array([0, 1.0, 0], F32)).astype(F32)
    w, h, seg, n = 96, 64, 3, 3
    be = HipBackend(w, h, StripPlan(h, 1, 0, n), max_segments=seg, flags=hip_lib.FLAG_EXACT_FILTER | SAH, debug_mask=hip_lib.DEBUG_HIT_ID)
    app = PathTracingApplication(be, w, h, n)
    app.objVertices, app.objIndices = xyz, idx
    app.buildAccelerationStructure()
    tris = oracle.flatten(xyz, idx)
    ref = oracle.OracleApp(w, h, tris, max_segments=seg, iterations=n)
    ctx = be.ctx
    try:
        _assert_sah_info(hip_lib, ctx.scene_build_info(), scene)
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
            _assert_clean(ctx.debug_bvh_check(), ctx.scene_build_info(), (scene, f))
    finally:
        be.close()


# ------------------------------------------------------------------------------ 4. rebuild
def test_rebuild_changes_cost_only(hip_lib):
    """test_device_bvh_gpu.test_rebuild_changes_cost_only's scheme with the SAH flag: the builder of a rebuild is the
    context's, so both contexts are uploaded with the device SAH builder and one of them rebuilds under the shear"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import HipBackend, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan
    xyz, idx = T._soup(np.random.default_rng(707), 3000, lo=-0.8, hi=0.8, size=0.08)
    xyz = (xyz + np.array([0, 1.0, 0], F32)).astype(F32)
    w, h, seg, n = 128, 96, 3, 5
    apps = []
    for _ in range(2):
        be = HipBackend(w, h, StripPlan(h, 1, 0, n), max_segments=seg, flags=hip_lib.FLAG_EXACT_FILTER | SAH,
                        debug_mask=hip_lib.DEBUG_HIT_ID | hip_lib.DEBUG_PREV_PIXEL)
        app = PathTracingApplication(be, w, h, n)
        app.objVertices, app.objIndices = xyz, idx
        app.buildAccelerationStructure()
        apps.append(app)
    a, b = apps  # a rebuilds, b never does
    try:
        for app in apps:
            _assert_sah_info(hip_lib, app.backend.ctx.scene_build_info(), "upload")
        uploaded = a.backend.ctx.debug_bvh_topology()
        models = [B._shear(), T._rot(0.7, 0.4, (0.0, 0.3, 0.0)), T._rot(0.75, 0.55, (0.05, 0.25, -0.1))]
        for f, m in enumerate(models):
            for app in apps:
                app.modelMatrix = m
                app.drawScene(())
            pa, pb = _read_all(hip_lib, a.backend.ctx), _read_all(hip_lib, b.backend.ctx)
            assert (pb["prev_vis"] > 0).mean() > 0.1, f  # the frame just ended
            _assert_same_planes(pa, pb, f)
            st = a.backend.ctx.debug_bvh_check()  # f == 1: the rebuilt tree, refit once to the rotated model
            assert all(st[k] == 0 for k in CLEAN), (f, st)
            if f == 0:
                a.backend.ctx.scene_rebuild()  # over the triangles as posed by the shear
                info, st = a.backend.ctx.scene_build_info(), a.backend.ctx.debug_bvh_check()
                _assert_sah_info(hip_lib, info, "after the rebuild")
                assert info["n_primitives"] == 3000 and info["build_ms"] > 0 and info["upload_ms"] > 0, info
                _assert_clean(st, info, "after the rebuild")
                rebuilt = a.backend.ctx.debug_bvh_topology()
                assert rebuilt[0].shape != uploaded[0].shape or not np.array_equal(rebuilt[0], uploaded[0]), "the shear changes the SAH tree"
            if f == 1:  # history and LUT_PREV survived the rebuild
                assert np.abs(pb["gradient"]).max() > 0 and np.abs(pb["lut_prev"]).max() > 0
        _assert_sah_info(hip_lib, b.backend.ctx.scene_build_info(), "never rebuilt")
    finally:
        for app in apps:
            app.backend.close()


def test_rebuild_under_the_identity_reproduces_the_upload(hip_lib, cornell):
    for tag, (xyz, idx, xf) in (("soup", T._soup(np.random.default_rng(5), 4000) + (None,)), ("lattice", _small_lattice(cornell))):
        with _upload(hip_lib, xyz, idx, xf, SAH) as ctx:
            before = ctx.debug_bvh_topology()
            ctx.scene_rebuild()
            info, after = ctx.scene_build_info(), ctx.debug_bvh_topology()
            _assert_sah_info(hip_lib, info, tag)
            _assert_clean(ctx.debug_bvh_check(), info, tag)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), tag


# ------------------------------------------------------------------------------ 5. full size
def test_million_triangle_scene(hip_lib, oracle, cornell):
    """BASELINE configs[4] (3840 x 2160, 8 segments, 1,152,000 triangles): the device SAH tree equals the host's (575,999
    nodes, depth 25); 200,000 rays and every plane of one frame equal the host-built context's bit for bit; and the one
    timing condition: after a warm-up upload, the whole upload with the device SAH build is faster than with the host
    build in the same process.  Prints all three builders' build info.

    Measured on the MI355X: see DESIGN.md 4 (K2/K0, "device SAH build")."""
    import test_fullsize_gpu as FS
    scene = FS._instanced(oracle, cornell)
    vx, ti, xf, cam, zfar = scene
    tris = oracle.flatten(vx, ti, xf)
    assert len(tris) == 1_152_000
    rays = B._fullsize_rays(tris)
    X = hip_lib.FLAG_EXACT_FILTER
    _assert_sah_tree(hip_lib, *T._soup(np.random.default_rng(5), 2000), flags=SAH, tag="warm-up")
    out = {}
    for name, flags in (("device SAH", X | SAH), ("host", X)):
        app = FS._make_instanced_app(hip_lib, scene, flags)
        ctx = app.backend.ctx
        try:
            info, st, topo = ctx.scene_build_info(), ctx.debug_bvh_check(), _topology(ctx)
            print(f"configs[4] {name} build: {info}")
            if name == "host":
                assert info["builder"] == hip_lib.BVH_BUILDER_HOST_SAH, info
            else:
                _assert_sah_info(hip_lib, info, name)
                _assert_clean(st, info, name)
            assert info["n_primitives"] == 576_000 and info["leaf_pairs"] == 1 and info["n_nodes"] == 575_999 and info["depth"] == 25, info
            ids, ts = ctx.selftest_trace(rays)
            app.drawScene(())
            out[name] = (info, ids, ts, _read_all(hip_lib, ctx), topo)
        finally:
            app.backend.close()
    with _upload(hip_lib, vx, ti, xf, hip_lib.FLAG_DEVICE_BVH_BUILD) as ctx:
        print(f"configs[4] device LBVH build: {ctx.scene_build_info()}")
    dev, host = out["device SAH"], out["host"]
    assert np.array_equal(dev[4][0], host[4][0]) and np.array_equal(dev[4][1], host[4][1]), "configs[4] topology"
    q = len(rays) // 4
    assert (host[1][:q] > 0).sum() > q // 20 and (host[1][q:2 * q] > 0).sum() > q // 4 and (host[1][2 * q:3 * q] > 0).sum() > q // 20
    assert np.array_equal(dev[1], host[1]) and np.array_equal(bits(dev[2]), bits(host[2])), \
        T._first_mismatch("configs[4] rays", rays, dev[1], dev[2], host[1], host[2])
    assert (host[3]["prev_vis"] > 0).mean() > 0.2
    _assert_same_planes(dev[3], host[3], "configs[4] frame")
    assert dev[0]["upload_ms"] < host[0]["upload_ms"], (dev[0], host[0])


# ------------------------------------------------------------------------------ 6. C++ host
def test_cpp_host_device_bvh_sah_switch(hip_lib, tmp_path):
    from test_cpp_host import APP, PKG
    subprocess.check_call(["make", "-C", os.path.join(PKG, "host"), "-s"])
    outs = {}
    for name, extra in (("device", ["--device-bvh-sah"]), ("host", [])):
        pfm = tmp_path / f"{name}.pfm"
        out = subprocess.run([APP, "--width", "160", "--height", "96", "--segments", "4", "--iterations", "5", "--lattice", "3x3x3",
                              "--tessellate", "2", "--frames", "3", "--dump", str(pfm)] + extra, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        outs[name] = (out.stdout, pfm.read_bytes())
    assert "built by device SAH" in outs["device"][0] and "built by host SAH" in outs["host"][0], outs["device"][0]
    assert len(outs["host"][1]) > 160 * 96 * 12 and outs["device"][1] == outs["host"][1]
