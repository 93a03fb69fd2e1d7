"""Moving instances (rtpt_scene_set_instances) and the device-side flatten + fan-pair test (RTPT_FLAG_DEVICE_FLATTEN,
csrc/scene_flatten.hip).

The tree stays ONE tree over world-space triangles; a move re-flattens, re-poses and refits it.  Closest hit = min over
(t, id) of one ray-triangle routine, boxes only cull and order (D4), and the flattened vertices are the host's and the
oracle's arithmetic bit for bit, so every check here is bit for bit: against `oracle.flatten` for the triangles, against the
oracle's frames for moving instances (`OracleApp.tris` is a plain attribute: setting it moves the instances and keeps
lut_prev from the frame before), against the host-flattened context for trees and build info.  rtpt_debug_upload_info
tells the device path from a host path that computes the same pixels.  The moves here are gentle and seen through a camera;
test_refit_moves_gpu.py traces adversarial rays after hostile ones (stacked, swapped, flung, collapsed, mirrored instances).
"""
import ctypes as C

import numpy as np
import pytest

import test_traversal_gpu as T
from conftest import bits
from test_scene_ext import rot_y_translate

pytestmark = pytest.mark.gpu

F32 = np.float32
CLEAN = ("bad_refs_to_triangles", "boxes_not_containing", "boxes_beyond_scene", "dangling")
D_LBVH, D_SAH, D_FLAT = 0x1000, 0x2000, 0x4000
IDENT = np.eye(4, dtype=F32).ravel()
CAM, ZFAR = (0.2, 2.3, 9.0), 30.0
W, H, SEG, N = 96, 64, 3, 3


# ------------------------------------------------------------------------------ scenes and transforms
def _base(cornell):
    """tessellated Cornell box (128 triangles) x a 2 x 2 x 2 lattice = 1,024 triangles"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import scenes
    vx, ti = scenes.tessellate_quads(cornell[0], cornell[1], 2)
    return vx, ti, scenes.lattice_xforms(2, 2, 2, 2.5)


def _about_centre(xf_row, angle, centre=(0.0, 1.0, 0.0)):
    """the instance rotated about y through its own centre (the box's, in mesh space), then placed as before"""
    c, s = np.cos(angle), np.sin(angle)
    r = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    m = np.asarray(xf_row, np.float64).reshape(3, 4)
    c0 = np.asarray(centre, np.float64)
    out = np.zeros((3, 4))
    out[:, :3] = m[:, :3] @ r
    out[:, 3] = m[:, :3] @ (c0 - r @ c0) + m[:, 3]
    return out.astype(F32).ravel()


def _moves(xf):
    """X1: one instance rotates about its own centre, another is translated; X2: every instance moves"""
    x0 = np.ascontiguousarray(xf, F32).reshape(-1, 12)
    x1 = x0.copy()
    x1[len(x0) // 2 - 1] = _about_centre(x0[len(x0) // 2 - 1], 0.5)
    x1[-1, [3, 7, 11]] += np.array([0.35, -0.2, 0.4], F32)
    rng = np.random.default_rng(31)
    x2 = np.stack([_about_centre(r, a) for r, a in zip(x1, rng.uniform(-0.4, 0.4, len(x1)))])
    x2[:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(x1), 3)).astype(F32)
    return x0, x1, np.ascontiguousarray(x2, F32)


def _general_xforms(n):
    """rotation x shear x non-uniform scale with irrational entries, no two alike"""
    rng = np.random.default_rng(77)
    out = []
    for i in range(n):
        ax, ay = rng.uniform(-np.pi, np.pi, 2)
        rot = np.asarray(T._rot(ax, ay, (0, 0, 0)), np.float64).reshape(4, 4).T[:3, :3]
        shear = np.array([[1.0, np.sqrt(2.0) / 3, 0.0], [0.0, 1.0, -1 / np.pi], [np.e / 10, 0.0, 1.0]])
        scale = np.diag([np.sqrt(3.0) / 2, 1.0 / np.sqrt(5.0) + 0.5, np.pi / 3])
        m = np.zeros((3, 4))
        m[:, :3] = rot @ shear @ scale
        m[:, 3] = [2.5 * (i % 2) - np.sqrt(1.5), 2.5 * ((i // 2) % 2) + 1 / np.e, -2.5 * (i // 4) + np.pi / 10]
        out.append(m)
    return np.ascontiguousarray(np.stack(out).astype(F32).reshape(-1, 12))


def _flatten_cases(cornell):
    vx, ti, xf = _base(cornell)
    rolled = ti.copy()
    rolled[-1] = np.roll(ti[-1], 1)   # the same triangle starting at another vertex: no longer (a, c, d) behind (a, b, c)
    one = np.ascontiguousarray(_general_xforms(3)[2:3])
    hx, hi = T._heightfield(8)
    return {
        "base": (vx, ti, xf, True),
        "last triangle dropped": (vx, ti[:-1], xf, False),        # 127 x 8: even, unpaired, instances off the wave grid
        "last triangle rolled": (vx, rolled, xf, False),          # the last pair of every instance fails, the very last too
        "last pair of all fails": (vx, rolled, one, False),       # one instance: ONLY the final pair fails
        "one instance": (vx, ti, one, True),
        "no transforms": (hx, hi, None, True),                    # 128 triangles, copied
        "general transforms": (vx, ti, _general_xforms(8), True),
    }


def _ubo(hip_lib, w, h):
    u = hip_lib.Ubo()
    u.model[:] = IDENT
    u.view[:] = hip_lib.look_at(CAM, (CAM[0], CAM[1], CAM[2] - 6.0), (0.0, 1.0, 0.0))
    proj = hip_lib.perspective(F32(0.4), F32(w) / F32(h), 0.1, ZFAR)
    proj[5] *= -1
    u.proj[:] = proj
    u.modelPrev[:], u.viewPrev[:], u.projPrev[:] = u.model[:], u.view[:], u.proj[:]
    return u


def _upload(hip_lib, xyz, idx, xf, flags):
    c = hip_lib.config_default(64, 64)
    c.flags = flags
    ctx = hip_lib.Context(c)
    ctx.scene_upload(xyz, idx, xf)
    return ctx


def _geometry_bytes(xyz, idx, xf):
    return 12 * len(xyz) + 12 * len(idx) + (48 * len(xf) if xf is not None else 0)


# ------------------------------------------------------------------------------ 1. device flatten equals host flatten
@pytest.mark.parametrize("case", ["base", "last triangle dropped", "last triangle rolled", "last pair of all fails", "one instance",
                                  "no transforms", "general transforms"])
def test_device_flatten_equals_host_flatten(hip_lib, oracle, cornell, case):
    xyz, idx, xf, paired = _flatten_cases(cornell)[case]
    tris = oracle.flatten(xyz, idx, xf)
    assert len(tris) > 64 and T._pair_ok(tris) == paired, case
    want_lut = oracle.lut(tris, IDENT)
    ubo = _ubo(hip_lib, 64, 64)
    for builder in (D_LBVH, D_LBVH | D_SAH):
        seen = []
        for flat in (D_FLAT, 0):
            with _upload(hip_lib, xyz, idx, xf, builder | flat) as ctx:
                up = ctx.debug_upload_info()
                info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
                topo = ctx.debug_bvh_topology()
                ctx.gbuffer(ubo)
                lut = ctx.readback(hip_lib.PLANE_LUT)
            tag = (case, hex(builder | flat))
            assert np.array_equal(bits(lut), bits(want_lut)), tag
            assert all(st[k] == 0 for k in CLEAN), (tag, st)
            assert info["fallback"] == hip_lib.BVH_FALLBACK_NONE and info["leaf_pairs"] == int(paired), (tag, info)
            assert info["builder"] == (hip_lib.BUILDER_DEVICE_SAH if builder & D_SAH else hip_lib.BVH_BUILDER_DEVICE_LBVH), (tag, info)
            if flat:
                assert up["device_flatten"] == 1 and up["device_pairs"] == 1, (tag, up)
                assert up["h2d_bytes"] == _geometry_bytes(xyz, idx, xf), (tag, up)
            else:
                assert up["device_flatten"] == 0 and up["device_pairs"] == 0 and up["h2d_bytes"] == 2 * tris.nbytes, (tag, up)
            seen.append(({k: v for k, v in info.items() if not k.endswith("_ms")}, st, topo))
        assert seen[0][0] == seen[1][0] and seen[0][1] == seen[1][1], (case, hex(builder), seen[0][:2], seen[1][:2])
        if builder & D_SAH:   # the SAH builder is deterministic in its input: the same triangles, the same tree
            assert np.array_equal(seen[0][2][0], seen[1][2][0]) and np.array_equal(seen[0][2][1], seen[1][2][1]), case


def test_the_flatten_flag_alone_and_small_scenes_keep_the_host_path(hip_lib, cornell):
    vx, ti, xf = _base(cornell)
    with _upload(hip_lib, vx, ti, xf, D_FLAT) as ctx:   # alone the bit is ignored, like the SAH bit
        assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_HOST_SAH
        assert ctx.debug_upload_info()["device_flatten"] == 0
    with _upload(hip_lib, cornell[0], cornell[1], xf[:2], D_LBVH | D_FLAT) as ctx:   # 64 triangles: screen bounds need them on the host
        assert ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH
        up = ctx.debug_upload_info()
        assert up["device_flatten"] == 0 and up["h2d_bytes"] == 2 * 64 * 36, up


# ------------------------------------------------------------------------------ 2. depth fallback
def test_flattened_tree_deeper_than_the_stack_falls_back_to_the_host_path(hip_lib, oracle):
    from test_device_bvh_gpu import _chain_scene
    xyz, idx = _chain_scene()
    tris = oracle.flatten(xyz, idx)
    assert len(tris) == 66   # past the 64 triangles below which the flag does not apply
    rays = T.ray_families(tris, np.random.default_rng(808))["aimed"]
    wid, wts = oracle.trace_rays(tris, rays, tmax=hip_lib.config_default(64, 64).ray_tmax)
    assert (wid > 0).sum() >= 100
    with _upload(hip_lib, xyz, idx, None, D_LBVH | D_FLAT) as ctx:
        info, st, up = ctx.scene_build_info(), ctx.debug_bvh_check(), ctx.debug_upload_info()
        assert info["builder"] == hip_lib.BVH_BUILDER_HOST_SAH and info["fallback"] == hip_lib.BVH_FALLBACK_DEPTH, info
        assert all(st[k] == 0 for k in CLEAN) and info["depth"] < 48, (st, info)
        # the scene stands on the host's triangles; the device attempt copied the mesh first
        assert up["device_flatten"] == 0 and up["h2d_bytes"] == _geometry_bytes(xyz, idx, None) + 2 * tris.nbytes, up
        ids, ts = ctx.selftest_trace(rays)
        assert T._first_mismatch("chain scene, device flatten", rays, ids, ts, wid, wts) is None


# ------------------------------------------------------------------------------ 3. / 4. moving instances match the oracle
def _make_app(hip_lib, mesh, xf, flags, w=W, h=H, seg=SEG, n=N, cam=CAM, zfar=ZFAR, debug=True, **kw):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import HipBackend, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan
    be = HipBackend(w, h, StripPlan(h, 1, 0, n), max_segments=seg, flags=flags,
                    debug_mask=(hip_lib.DEBUG_HIT_ID | hip_lib.DEBUG_PREV_PIXEL) if debug else 0)
    app = PathTracingApplication(be, w, h, n, cameraOrigin=cam, z_far=zfar, **kw)
    app.objVertices, app.objIndices = mesh
    app.buildAccelerationStructure(xf)
    return app


PLANES = ("VIS_ID", "HIT_ID", "WORLDPOS", "DEPTH", "GRADIENT", "IMAGE", "LUT", "LUT_PREV")


def _assert_same_ubo(got, want, f):
    """both sides were given the same matrices: equal as numbers, and bit for bit except for the sign of a zero.  From CAM
    the first view looks at (0, 1, 0) with a side vector exactly perpendicular to the eye, so its translation
    -dot(s, eye) is a zero: rtpt_util_look_at negates the sum (-0, as glm::lookAtRH is written), the oracle's compiler
    folds the negation into the sum (+0).  That matrix is viewPrev on frame 0 only; every plane below stays bit for bit."""
    a, b = np.frombuffer(bytes(got), F32), np.frombuffer(bytes(want), F32)
    differ = bits(a) != bits(b)
    assert np.array_equal(a, b) and not (differ & (a != 0)).any(), (f, np.flatnonzero(differ))
    if f > 0:
        assert not differ.any(), (f, np.flatnonzero(differ))


def _moving_frames_match_the_oracle(hip_lib, oracle, mesh, xf, flags, device_moves, expect_builder=None, expect_flatten=0):
    """seven frames with transforms [X0, X0, X0, X0, X1, X1, X2]; frame 6 also moves the camera and the model"""
    from test_parity_gpu import l2_ok
    vx, ti = mesh
    x0, x1, x2 = _moves(xf)
    app = _make_app(hip_lib, mesh, x0, flags)
    ctx = app.backend.ctx
    try:
        if expect_builder is not None:
            assert ctx.scene_build_info()["builder"] == expect_builder, ctx.scene_build_info()
        assert ctx.debug_upload_info()["device_flatten"] == expect_flatten
        ref = oracle.OracleApp(W, H, oracle.flatten(vx, ti, x0), max_segments=SEG, iterations=N, camera=CAM, z_far=ZFAR)
        model6 = rot_y_translate(0.1, (0.1, 0.05, -0.1))
        total, moves, served, current = 0, 0, [], x0
        for f, x in enumerate([x0, x0, x0, x0, x1, x1, x2]):
            if x is not current:
                app.setInstanceTransforms(x)
                current = x
                moves += 1
                ref.tris = oracle.flatten(vx, ti, x)
                st, up = ctx.debug_bvh_check(), ctx.debug_upload_info()
                assert all(st[k] == 0 for k in CLEAN), (f, st)
                assert up["moves_without_sync"] == (moves if device_moves else 0), (f, up)
                assert up["device_flatten"] == int(device_moves) and up["device_pairs"] == 0, (f, up)
                if device_moves:   # 48 bytes per instance; the first move of a host-flattened scene brings the mesh, once
                    mesh_bytes = 0 if (expect_flatten or moves > 1) else 12 * len(vx) + 12 * len(ti)
                    assert up["h2d_bytes"] == 48 * len(x) + mesh_bytes, (f, up)
            if f == 6:
                app.modelMatrix = model6
                ref.model = model6
            before = ctx.reuse_info()["frames_skipped"]
            app.updateScene(("D",) if f == 6 else ())
            app.drawVisbilityBuffer()
            app.computeTemporalGradient()
            app.drawSceneToImage()
            got = {p: ctx.readback(getattr(hip_lib, "PLANE_" + p)) for p in PLANES}
            app.applyTemporalFiltering()
            final, pp = ctx.readback(hip_lib.PLANE_IMAGE), ctx.readback(hip_lib.PLANE_PREV_PIXEL)
            app.copyImageToSwapChainsCurrentImage()
            app._end_instance_move()
            app.frameCount += 1
            served.append(ctx.reuse_info()["frames_skipped"] - before)
            lut_prev_want = ref.lut_prev
            fo = ref.draw_scene(move_camera=(0.1, 0, 0) if f == 6 else None)
            _assert_same_ubo(app.ubo, ref.ubo, f)
            assert np.array_equal(bits(got["LUT"]), bits(fo.lut)), f
            if lut_prev_want is not None:
                assert np.array_equal(bits(got["LUT_PREV"]), bits(lut_prev_want)), f
            assert np.array_equal(got["VIS_ID"], fo.vis) and np.array_equal(got["HIT_ID"], fo.hit_id), f
            assert np.array_equal(bits(got["WORLDPOS"]), bits(fo.worldpos)), f
            assert np.array_equal(bits(got["DEPTH"]), bits(fo.depth)), f
            assert np.array_equal(bits(got["GRADIENT"]), bits(fo.gradient)), f
            assert np.array_equal(bits(got["IMAGE"]), bits(fo.traced)), f
            assert np.array_equal(pp, fo.prev_pixel), f
            ok, rel = l2_ok(final, fo.image)
            assert ok, (f, rel)
            total += fo.rays
            if f == 0:
                assert (got["VIS_ID"] > 0).mean() > 0.2, "the frame must show the geometry"
            if f == 4:
                assert (got["GRADIENT"][..., 0] > 0).any(), "a moved surface point changes its Phong shade"
        assert ctx.raycount() == total
        assert served == [0, 0, 1, 1, 0, 0, 0], served   # rest is served; a frame of moved instances never is
        assert moves == 2
    finally:
        app.backend.close()


@pytest.mark.parametrize("flags,host_refit", [(0, False), (D_LBVH, False), (D_LBVH | D_SAH, False), (D_LBVH | D_SAH | D_FLAT, False), (0, True)])
def test_moving_instances_match_the_oracle(hip_lib, oracle, cornell, monkeypatch, flags, host_refit):
    monkeypatch.setenv("RTPT_HOST_REFIT", "1" if host_refit else "0")
    vx, ti, xf = _base(cornell)
    builder = {0: hip_lib.BVH_BUILDER_HOST_SAH, D_LBVH: hip_lib.BVH_BUILDER_DEVICE_LBVH}.get(flags & ~D_FLAT, hip_lib.BUILDER_DEVICE_SAH)
    _moving_frames_match_the_oracle(hip_lib, oracle, (vx, ti), xf, flags, device_moves=not host_refit, expect_builder=builder,
                                    expect_flatten=int(bool(flags & D_FLAT)))


@pytest.mark.parametrize("flags", [0, 2])   # wave-uniform brute force (re-flattened and re-posed on the host) / BVH traversal
def test_moving_instances_of_a_brute_force_scene_match_the_oracle(hip_lib, oracle, cornell, flags):
    xf = np.zeros((2, 3, 4), F32)
    xf[:, 0, 0] = xf[:, 1, 1] = xf[:, 2, 2] = 1.0
    xf[0, :, 3], xf[1, :, 3] = (-1.15, 1.2, 0.0), (1.15, 1.3, -0.5)
    xf = xf.reshape(-1, 12)
    assert 2 * len(cornell[1]) == 64
    _moving_frames_match_the_oracle(hip_lib, oracle, (cornell[0], cornell[1]), xf, flags, device_moves=bool(flags & 2))


# ------------------------------------------------------------------------------ 5. rebuild after a move
def test_rebuild_after_a_move_changes_cost_only(hip_lib, cornell):
    from test_device_bvh_gpu import _assert_same_planes, _read_all
    vx, ti, xf = _base(cornell)
    _, _, x2 = _moves(xf)
    apps = [_make_app(hip_lib, (vx, ti), xf, hip_lib.FLAG_EXACT_FILTER | D_LBVH) for _ in range(2)]
    a, b = apps   # a rebuilds, b never does
    try:
        for app in apps:
            app.drawScene(())
            app.setInstanceTransforms(x2)
        a.backend.ctx.scene_rebuild()
        info, st = a.backend.ctx.scene_build_info(), a.backend.ctx.debug_bvh_check()
        assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["n_primitives"] == 512, info
        assert all(st[k] == 0 for k in CLEAN) and st["leaves"] == 512, st
        for f, keys in enumerate([(), ("D",), ()]):
            for app in apps:
                app.drawScene(keys)
            pa, pb = _read_all(hip_lib, a.backend.ctx), _read_all(hip_lib, b.backend.ctx)
            assert (pb["prev_vis"] > 0).mean() > 0.2, f
            _assert_same_planes(pa, pb, f)
            if f == 0:   # the frame of the move: history and LUT_PREV (the pose before) survived the rebuild
                assert np.abs(pb["gradient"]).max() > 0 and not np.array_equal(bits(pb["lut"]), bits(pb["lut_prev"]))
        st = b.backend.ctx.debug_bvh_check()
        assert all(st[k] == 0 for k in CLEAN), st
    finally:
        for app in apps:
            app.backend.close()


# ------------------------------------------------------------------------------ 6. errors
def test_refused_calls_leave_the_scene_untouched(hip_lib, cornell):
    from test_device_bvh_gpu import _assert_same_planes, _read_all
    vx, ti, xf = _base(cornell)
    with hip_lib.Context(hip_lib.config_default(64, 64)) as ctx:
        with pytest.raises(hip_lib.RtptError) as e:
            ctx.scene_set_instances(xf)
        assert e.value.code == hip_lib.RTPT_E_NO_SCENE
        assert ctx.debug_upload_info() == {"h2d_bytes": 0, "device_flatten": 0, "device_pairs": 0, "moves_without_sync": 0}
    lib = hip_lib.load()
    a, b = (_make_app(hip_lib, (vx, ti), xf, hip_lib.FLAG_EXACT_FILTER) for _ in range(2))   # a makes the refused calls
    plain = _make_app(hip_lib, T._heightfield(8), None, hip_lib.FLAG_EXACT_FILTER)           # uploaded without transforms: count 1
    try:
        _, x1, _ = _moves(xf)
        refused = [lambda: a.backend.ctx.scene_set_instances(x1[:-1]),                        # another count
                   lambda: a.backend.ctx.scene_set_instances(np.concatenate([x1, x1[:1]])),
                   lambda: hip_lib._check(lib.rtpt_scene_set_instances(a.backend.ctx._h, None, len(x1))),   # NULL transforms
                   lambda: hip_lib._check(lib.rtpt_scene_set_instances(a.backend.ctx._h, None, 0))]
        for f, call in enumerate(refused):
            with pytest.raises(hip_lib.RtptError) as e:
                call()
            assert e.value.code == hip_lib.RTPT_E_INVALID, f
            for app in (a, b):
                app.drawScene(("D",) if f == 1 else ())
            _assert_same_planes(_read_all(hip_lib, a.backend.ctx), _read_all(hip_lib, b.backend.ctx), f)
        assert a.backend.ctx.debug_upload_info()["moves_without_sync"] == 0
        assert lib.rtpt_debug_upload_info(a.backend.ctx._h, None) == hip_lib.RTPT_E_INVALID
        with pytest.raises(hip_lib.RtptError) as e:
            plain.backend.ctx.scene_set_instances(x1[:2])
        assert e.value.code == hip_lib.RTPT_E_INVALID
        plain.backend.ctx.scene_set_instances(x1[:1])   # one instance is the count of a scene without transforms
        assert plain.backend.ctx.debug_upload_info()["moves_without_sync"] == 1
    finally:
        for app in (a, b, plain):
            app.backend.close()


# ------------------------------------------------------------------------------ 7. full size once
def test_million_triangles_move_without_an_upload(hip_lib, cornell):
    """BASELINE configs[4]'s scene (1,152,000 triangles): two moves of a device-flattened scene against fresh contexts that
    were uploaded (host flatten, 0x3000) with the same transforms and run at the same frame number"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import scenes
    vx, ti, xf, cam, zfar = scenes.instanced_cornell(cornell[0], cornell[1])
    assert len(ti) * len(xf) == 1_152_000
    w, h, seg, n = 480, 270, 4, 3
    rng = np.random.default_rng(5)
    x1 = xf.copy()
    x1[:, [3, 7, 11]] += rng.uniform(-0.4, 0.4, (len(xf), 3)).astype(F32)
    x2 = np.stack([_about_centre(r, a) for r, a in zip(x1, rng.uniform(-0.5, 0.5, len(xf)))])
    kw = dict(w=w, h=h, seg=seg, n=n, cam=cam, zfar=zfar, debug=False, lightPos=(1.0, float(cam[1]), float(cam[2]) - 8.0))
    planes = ("VIS_ID", "WORLDPOS", "DEPTH", "IMAGE")

    def frame(app):
        app.updateScene(())
        app.pushConstants.cameraPos[:] = app.cameraOrigin   # (updateScene sets it on frame 0 only: the fresh apps start later)
        app.drawVisbilityBuffer()
        app.computeTemporalGradient()
        app.drawSceneToImage()
        out = {p: app.backend.ctx.readback(getattr(hip_lib, "PLANE_" + p)) for p in planes}
        app.applyTemporalFiltering()
        app.copyImageToSwapChainsCurrentImage()
        app.frameCount += 1
        return out

    moved = {}
    app = _make_app(hip_lib, (vx, ti), xf, D_LBVH | D_SAH | D_FLAT, **kw)
    try:
        ctx = app.backend.ctx
        up, info = ctx.debug_upload_info(), ctx.scene_build_info()
        print(f"configs[4] device flatten upload: {info} {up}")
        assert up["device_flatten"] == 1 and up["device_pairs"] == 1 and up["h2d_bytes"] == _geometry_bytes(vx, ti, xf) < 1_000_000, up
        assert info["builder"] == hip_lib.BUILDER_DEVICE_SAH and info["n_primitives"] == 576_000 and info["leaf_pairs"] == 1, info
        frame(app)
        for f, x in ((1, x1), (2, x2)):
            app.setInstanceTransforms(x)
            up = ctx.debug_upload_info()
            assert up == {"h2d_bytes": 48 * len(x), "device_flatten": 1, "device_pairs": 0, "moves_without_sync": f}, up
            moved[f] = frame(app)
        st = ctx.debug_bvh_check()
        assert all(st[k] == 0 for k in CLEAN) and st["leaves"] == 576_000, st
    finally:
        app.backend.close()
    for f, x in ((1, x1), (2, x2)):
        fresh = _make_app(hip_lib, (vx, ti), x, D_LBVH | D_SAH, **kw)
        try:
            assert fresh.backend.ctx.debug_upload_info()["device_flatten"] == 0
            fresh.frameCount = f
            want = frame(fresh)
        finally:
            fresh.backend.close()
        assert (want["VIS_ID"] > 0).mean() > 0.2
        for p in planes:
            assert np.array_equal(bits(moved[f][p]), bits(want[p])), (f, p)
    assert not np.array_equal(moved[1]["VIS_ID"], moved[2]["VIS_ID"]), "the second move did move the scene"


# ------------------------------------------------------------------------------ 8. strips
@pytest.mark.parametrize("mode", ["redundant", "exchange"])
def test_two_strips_with_moving_instances_equal_the_single_context(hip_lib, cornell, monkeypatch, mode):
    """two strip contexts against the single context over a key script with one setInstanceTransforms call (before frame
    2): the frame of the move reprojects across the strip boundary like a camera move, so the ranks must swap history"""
    from test_device_bvh_gpu import STRIP_KEYS, _small_scenes
    from test_parity_gpu import _strips_vs_single
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import PathTracingApplication
    _, kw = _small_scenes(cornell)["lattice"]
    x1 = np.ascontiguousarray(kw["instance_xforms"], F32).reshape(-1, 12).copy()
    x1[::3, 7] += F32(0.8)    # every third box moves up by a third of its height
    x1[1::3, 3] -= F32(0.3)
    calls, statics = [], []
    update = PathTracingApplication.updateScene

    def update_and_move(self, keys=()):
        if self.frameCount == 2 and self._instances_moved != 2:
            self.setInstanceTransforms(x1)
            calls.append(self.backend.ctx.debug_upload_info())
        update(self, keys)
        if self.frameCount == 2:
            statics.append(self._camera_static())

    monkeypatch.setattr(PathTracingApplication, "updateScene", update_and_move)
    flags = hip_lib.FLAG_EXACT_FILTER | D_LBVH | D_SAH | D_FLAT
    _strips_vs_single(192, 128, 4, 5, 2, mode, flags, STRIP_KEYS, **kw)
    assert len(calls) == 3 and all(c["device_flatten"] == 1 and c["moves_without_sync"] == 1 for c in calls), calls
    assert statics == [False] * 3, "STRIP_KEYS[2] moves the light only: the instances alone make this frame a moved one"


# ------------------------------------------------------------------------------ 9. two frames in flight
def test_both_contexts_of_a_pipelined_backend_receive_the_transforms(hip_lib, cornell):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    vx, ti, xf = _base(cornell)
    _, x1, _ = _moves(xf)
    kw = dict(max_segments=SEG, iterations=N, flags=D_LBVH | D_FLAT, mesh=(vx, ti), instance_xforms=xf, cameraOrigin=CAM, z_far=ZFAR)
    two, one = make_app(W, H, frames_in_flight=2, **kw), make_app(W, H, **kw)
    try:
        for app in (two, one):
            app.drawScene(())
            app.setInstanceTransforms(x1)
        assert [b.ctx.debug_upload_info()["moves_without_sync"] for b in two.backend.be] == [1, 1]
        for f in range(2):   # one frame in each context; the traced image does not depend on the history
            traced = []
            for app in (two, one):
                app.updateScene(())
                app.drawVisbilityBuffer()
                app.computeTemporalGradient()
                app.drawSceneToImage()
                traced.append((app.backend.ctx.readback(hip_lib.PLANE_VIS_ID), app.backend.ctx.readback(hip_lib.PLANE_IMAGE)))
                app.applyTemporalFiltering()
                app.copyImageToSwapChainsCurrentImage()
                app.frameCount += 1
            assert np.array_equal(traced[0][0], traced[1][0]) and np.array_equal(bits(traced[0][1]), bits(traced[1][1])), f
    finally:
        two.backend.close()
        one.backend.close()
