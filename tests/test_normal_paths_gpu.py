"""Smooth shading (rtpt_scene_set_normals) on the device against tests/normal_paths.py, whole frames bit for bit: IMAGE, HIT_ID, the
ray count and, with RTPT_FLAG_EXT_DEMODULATE, ALBEDO.  No tolerance appears anywhere.  tests/test_normal_paths_cpu.py holds the walker
to the walker without normals and to float64 first.

Frames are 70 x 10: one full tile column, a partial one, partial tile rows.  Both scenes have more than 64 triangles in three
instances — the identity, a rotation with a non-uniform scale, a mirror — so they trace through the BVH: over triangles (uv_sphere,
scene mode 1) and over fan pairs (half_cylinder, mode 2), asserted on rtpt_scene_build_info.

CELLS lists the sampled cells of scene mode x SPEC x TEX x DEMOD x launch form x samples per pixel x budget; test_cells_cover_the_axes
asserts that every value the kernels are instantiated for appears in it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_planes as FP
import gbuffer_scenes as G
import path_walker as WK
import normal_paths as NP
import pathtrace_scenes as P
import shading_scenes as SS
import test_pathtrace_scenes_gpu as T
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

W, H = NP.SHAPE
NO_PATH_COMPACTION = 0x8
# (scene, SPEC, TEX, DEMOD, launch form, samples per pixel, segments)
CELLS = (
    ("uv_sphere", 0, 0, False, "fused", 1, 3),
    ("half_cylinder", 1, 1, True, "fused", 1, 3),
    ("uv_sphere", 2, 2, False, "unfused", 1, 4),
    ("half_cylinder", 3, 0, True, "unfused", 1, 3),
    ("uv_sphere", 4, 1, False, "fused", 2, 2),
    ("half_cylinder", 5, 2, False, "fused", 1, 3),
    ("uv_sphere", 10, 2, True, "fused", 1, 4),
    ("half_cylinder", 10, 0, False, "unfused", 2, 2),
    ("uv_sphere", 2, 0, False, "fused", 1, 12),          # the BVH window of 8 is crossed: k_pathtrace_queue
    ("half_cylinder", 2, 1, False, "unfused-window2", 1, 5),   # ... and behind RTPT_PT_WINDOW=2, where this open scene still has paths
)
_ref = {}


def test_cells_cover_the_axes():
    col = lambda i: {c[i] for c in CELLS}
    assert col(0) == set(NP.CASES) and col(1) >= {0, 1, 2, 3, 4, 5, 10} and col(2) == {0, 1, 2} and col(3) == {False, True}
    assert col(4) == {"fused", "unfused", "unfused-window2"} and col(5) == {1, 2} and 12 in col(6)


def _env(monkeypatch, form="fused", host_refit=False):
    monkeypatch.delenv("RTPT_PT_WINDOW", raising=False)
    if form == "unfused-window2":
        monkeypatch.setenv("RTPT_PT_WINDOW", "2")
    if form != "fused":
        monkeypatch.setenv("RTPT_NO_TRACE_FUSION", "1")
    else:
        monkeypatch.delenv("RTPT_NO_TRACE_FUSION", raising=False)
    monkeypatch.setenv("RTPT_HOST_REFIT", "1" if host_refit else "0")


def reference(oracle, name, spec, tex, demod, spp, segments, moved=False, model=None, smooth=True, rows=None, frame=0):
    key = (name, spec, tex, demod, spp, segments, moved, None if model is None else tuple(model), smooth, rows, frame)
    if key not in _ref:
        c, nrm = NP.case(oracle, name, moved, model)
        if not smooth:
            nrm = nrm._replace(tri_smooth=np.zeros_like(nrm.tri_smooth))
        r = WK.walk(oracle, c.sh.scene, W, H, segments, normals=nrm, spp=spp, tex=WK.textures(c.sh, tex), demod=demod, rows=rows, frame=frame,
                    **NP.setup(oracle, c, spec))
        FP.check_ids(r["HIT_ID"], len(c.sh.scene.tris))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ref[key] = r
    return _ref[key]


def upload(abi, ctx, c, spec, tex, normals=True, smooth=None):
    sh = c.sh
    ctx.scene_upload(sh.mesh[0], sh.mesh[1], NP.xforms())
    ctx.set_materials_ext(sh.scene.tri_material, abi.materials_ext(sh.scene.materials, sh.spec if spec >= 1 else None, c.glass if spec >= 2 else None))
    if tex:
        ctx.set_textures(sh.tri_uv, sh.tri_texture, *SS.atlas(sh, tex))
    if normals:
        ctx.set_normals(c.tri_normals, c.tri_smooth if smooth is None else smooth)


def context(abi, c, segments, flags=0, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, c.sh.scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def frame(abi, oracle, ctx, c, demod, frame_no=0, model=None):
    """K0, K1, K2 in the reference's order under ubo.model `model`; IMAGE, HIT_ID, the ray count, ALBEDO"""
    sc = c.sh.scene
    pc = G.fill_push_constants(abi.PushConstants(), P.push_constants(sc), frame_no)
    u = T._ubo(abi, oracle, sc, W, H)
    if model is not None:
        u.model[:] = np.asarray(model, np.float32).ravel()
    ctx.reset_counters()
    ctx.gbuffer(u)
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


def flags_of(spec, demod):
    return NP.SPEC_FLAGS[spec] | (NP.DEMODULATE if demod else 0)


# ------------------------------------------------------------------------------------------ 1. nothing smooth is no normals at all
@pytest.mark.parametrize("name", list(NP.CASES))
def test_no_smooth_triangle_changes_nothing(hip_lib, oracle, monkeypatch, name):
    """normals with every tri_smooth 0 against a RTPT_FLAG_FORCE_BVH context without normals: IMAGE, ALBEDO, HIT_ID and RAYCOUNT bit for
    bit (SPEC 10, the mixed atlas, DEMOD, 4 segments), and the same after the normals are removed again"""
    abi = hip_lib
    _env(monkeypatch)
    c, _ = NP.case(oracle, name)
    fl = flags_of(10, True) | NP.FORCE_BVH
    with context(abi, c, 4, fl) as plain, context(abi, c, 4, fl) as ctx:
        upload(abi, plain, c, 10, 2, normals=False)
        upload(abi, ctx, c, 10, 2, smooth=np.zeros_like(c.tri_smooth))
        want = frame(abi, oracle, plain, c, True)
        compare(frame(abi, oracle, ctx, c, True), want, (name, "all flat"))
        ctx.end_frame()
        plain.end_frame()
        ctx.set_normals(None)
        compare(frame(abi, oracle, ctx, c, True, 1), frame(abi, oracle, plain, c, True, 1), (name, "removed"))


# ------------------------------------------------------------------------------------------ 2. frames
@pytest.mark.parametrize("cell", CELLS, ids=["-".join(str(v) for v in c) for c in CELLS])
def test_frames(hip_lib, oracle, monkeypatch, cell):
    name, spec, tex, demod, form, spp, segments = cell
    abi = hip_lib
    _env(monkeypatch, form)
    c, _ = NP.case(oracle, name)
    ref = reference(oracle, name, spec, tex, demod, spp, segments)
    with context(abi, c, segments, flags_of(spec, demod), spp) as ctx:
        upload(abi, ctx, c, spec, tex)
        assert bool(ctx.scene_build_info()["leaf_pairs"]) == (name == "half_cylinder"), cell
        got = frame(abi, oracle, ctx, c, demod)
    compare(got, ref, cell)
    assert ref["smooth"] > 0, cell
    if segments == 12 or form == "unfused-window2":
        assert P.alive_after(ref["seq_n"], [2 if form == "unfused-window2" else 8])[0] > 0, (cell, "nothing reaches the queue kernel")


# ------------------------------------------------------------------------------------------ 3. re-posed scenes
MODEL = np.array([[0.96, 0.0, 0.28, 0.0], [0.0, 1.1, 0.0, 0.0], [-0.28, 0.0, 0.96, 0.0], [0.05, -0.02, 0.1, 1.0]], np.float32).ravel()   # column-major


def _repose(abi, oracle, name):
    """set_instances, then a changed ubo.model, then rtpt_scene_rebuild: the frame is the walker's on the new pose every time"""
    c, _ = NP.case(oracle, name)
    spec, tex, demod, seg = 10, 1, True, 3
    with context(abi, c, seg, flags_of(spec, demod)) as ctx:
        upload(abi, ctx, c, spec, tex)
        compare(frame(abi, oracle, ctx, c, demod), reference(oracle, name, spec, tex, demod, 1, seg), (name, "first"))
        ctx.end_frame()
        ctx.scene_set_instances(NP.xforms(moved=True))
        moved, _ = NP.case(oracle, name, moved=True)
        compare(frame(abi, oracle, ctx, moved, demod, 1), reference(oracle, name, spec, tex, demod, 1, seg, moved=True, frame=1), (name, "moved"))
        ctx.end_frame()
        posed, _ = NP.case(oracle, name, moved=True, model=MODEL)
        compare(frame(abi, oracle, ctx, posed, demod, 2, MODEL), reference(oracle, name, spec, tex, demod, 1, seg, moved=True, model=MODEL, frame=2),
                (name, "model"))
        ctx.end_frame()
        ctx.scene_rebuild()
        compare(frame(abi, oracle, ctx, posed, demod, 3, MODEL), reference(oracle, name, spec, tex, demod, 1, seg, moved=True, model=MODEL, frame=3),
                (name, "rebuilt"))


@pytest.mark.parametrize("name", list(NP.CASES))
def test_reposed_on_the_device_route(hip_lib, oracle, monkeypatch, name):
    _env(monkeypatch)
    _repose(hip_lib, oracle, name)


def test_reposed_on_the_host_route_in_a_child_process():
    """the same with RTPT_HOST_REFIT=1 (read at rtpt_create), in a process of its own: set_instances and a changed model"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import torch; torch.cuda.is_available()\n"
            "from oracle import oracle as O; O.build()\n"
            "from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi; abi.load()\n"
            "import test_normal_paths_gpu as T\n"
            "T._repose_host(abi, O, 'uv_sphere')\n"
            "print('host route ok')\n") % (here, os.path.dirname(here))
    env = dict(os.environ, RTPT_HOST_REFIT="1")
    env.pop("RTPT_NO_TRACE_FUSION", None)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "host route ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _repose_host(abi, oracle, name):
    c, _ = NP.case(oracle, name)
    spec, tex, demod, seg = 2, 0, False, 3
    with context(abi, c, seg, flags_of(spec, demod)) as ctx:
        upload(abi, ctx, c, spec, tex)
        compare(frame(abi, oracle, ctx, c, demod), reference(oracle, name, spec, tex, demod, 1, seg), (name, "host first"))
        ctx.end_frame()
        ctx.scene_set_instances(NP.xforms(moved=True))
        assert ctx.debug_upload_info()["device_flatten"] == 0
        moved, _ = NP.case(oracle, name, moved=True)
        compare(frame(abi, oracle, ctx, moved, demod, 1), reference(oracle, name, spec, tex, demod, 1, seg, moved=True, frame=1), (name, "host moved"))
        ctx.end_frame()
        posed, _ = NP.case(oracle, name, moved=True, model=MODEL)
        compare(frame(abi, oracle, ctx, posed, demod, 2, MODEL), reference(oracle, name, spec, tex, demod, 1, seg, moved=True, model=MODEL, frame=2),
                (name, "host model"))


# ------------------------------------------------------------------------------------------ 4. strips
def test_two_strips_equal_the_single_context(hip_lib, oracle, monkeypatch):
    """rows [0, 6) and [6, 10) in two contexts against the walker's full frame, each strip's counted rays its own"""
    abi = hip_lib
    _env(monkeypatch)
    name, spec, tex, demod, seg = "uv_sphere", 4, 2, True, 3
    c, _ = NP.case(oracle, name)
    full = reference(oracle, name, spec, tex, demod, 1, seg)
    total = 0
    for rows in ((0, 6), (6, 10)):
        counted = reference(oracle, name, spec, tex, demod, 1, seg, rows=rows)["rays"]
        with context(abi, c, seg, flags_of(spec, demod), rows=rows) as ctx:
            upload(abi, ctx, c, spec, tex)
            got = frame(abi, oracle, ctx, c, demod)
        compare(got, dict(full, rays=counted), (name, "strip", rows), rows)
        total += counted
    assert total == full["rays"]


# ------------------------------------------------------------------------------------------ 5. the rules, operand by operand
def test_selftest_shading_normal(hip_lib, oracle):
    abi = hip_lib
    cases = NP.hostile_operands()
    want = NP.shading_normal32(oracle, cases)
    with abi.Context(abi.config_default(64, 16)) as ctx:
        got = ctx.selftest_shading_normal(cases)
    same_bits(got, want, ("rtpt_selftest_shading_normal",))
    assert 0 < want[:, 0].sum() < len(want) and 0 < want[:, 4].sum() < len(want) and 0 < want[:, 5].sum() < len(want)


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_scene_untouched(hip_lib, oracle, monkeypatch):
    abi = hip_lib
    _env(monkeypatch)
    name, spec, tex, demod, seg = "half_cylinder", 2, 0, False, 3
    c, _ = NP.case(oracle, name)
    ref = reference(oracle, name, spec, tex, demod, 1, seg)

    def refused(ctx, code, *a):
        with pytest.raises(abi.RtptError) as e:
            ctx.set_normals(*a)
        assert e.value.code == code, (e.value.code, str(e.value))

    with context(abi, c, seg, flags_of(spec, demod)) as ctx:
        refused(ctx, abi.RTPT_E_NO_SCENE, c.tri_normals, c.tri_smooth)                 # before an upload
        upload(abi, ctx, c, spec, tex)
        refused(ctx, abi.RTPT_E_INVALID, c.tri_normals[:-1], c.tri_smooth[:-1])        # not the upload's base count
        refused(ctx, abi.RTPT_E_INVALID, np.tile(c.tri_normals, (3, 1)), np.tile(c.tri_smooth, 3))   # the posed count is not it either
        rc = ctx._lib.rtpt_scene_set_normals(ctx._h, None, None, 5)               # NULL normals with a count
        assert rc == abi.RTPT_E_INVALID
        compare(frame(abi, oracle, ctx, c, demod), ref, (name, "after refusals"))
    with context(abi, c, seg, flags_of(spec, demod) | NO_PATH_COMPACTION) as ctx:
        upload(abi, ctx, c, spec, tex, normals=False)
        refused(ctx, abi.RTPT_E_INVALID, c.tri_normals, c.tri_smooth)                  # that A/B flag has no smooth kernels
        flat = reference(oracle, name, spec, tex, demod, 1, seg, smooth=False)
        compare(frame(abi, oracle, ctx, c, demod), flat, (name, "no compaction"))


# ------------------------------------------------------------------------------------------ 7. a scene small enough for brute force
def test_a_small_scene_moves_onto_its_tree_and_back(hip_lib, oracle, monkeypatch):
    """40 triangles uploaded without transforms, no RTPT_FLAG_FORCE_BVH: brute force (with primary-ray culling and, from the second
    frame on, the deferred final pass's launch) until rtpt_scene_set_normals, through the BVH while the scene holds normals, brute
    force again once they are removed — every frame the walker's, and rtpt_scene_set_instances in between on both sides"""
    abi = hip_lib
    _env(monkeypatch)
    c, nrm = NP.small_case(oracle)
    sc = c.sh.scene
    assert len(sc.tris) <= 64
    spec, seg = 2, 3
    s = NP.setup(oracle, c, spec)

    def want(normals, frame_no):
        return WK.walk(oracle, sc, W, H, seg, normals=normals, frame=frame_no, n_base=len(nrm.tri_smooth), **s)
    with context(abi, c, seg, flags_of(spec, False)) as ctx:
        ctx.scene_upload(c.sh.mesh[0], c.sh.mesh[1])
        ctx.set_materials_ext(sc.tri_material, abi.materials_ext(sc.materials, c.sh.spec, c.glass))
        compare(frame(abi, oracle, ctx, c, False, 0), want(None, 0), ("small", "before"))
        ctx.end_frame()
        ctx.set_normals(c.tri_normals, c.tri_smooth)
        compare(frame(abi, oracle, ctx, c, False, 1), want(nrm, 1), ("small", "smooth"))
        ctx.end_frame()
        compare(frame(abi, oracle, ctx, c, False, 2, MODEL), WK.walk(oracle, _posed(oracle, sc), W, H, seg, normals=nrm._replace(cof=NP.cof_table(oracle, MODEL)),
                                                                       frame=2, **s), ("small", "smooth, model"))
        ctx.end_frame()
        ctx.set_normals(None)
        compare(frame(abi, oracle, ctx, c, False, 3), want(None, 3), ("small", "removed"))
    assert want(nrm, 1)["smooth"] > 0


def _posed(oracle, sc):
    t = np.asarray(sc.tris, np.float32).reshape(-1, 3)
    p = NP._contract(oracle, "mat_row_point", np.broadcast_to(MODEL, (len(t), 16)), t)[:, :3]
    return sc._replace(tris=np.ascontiguousarray(p.reshape(-1, 9)))


# ------------------------------------------------------------------------------------------ 8. the hosts
def test_hosts_apply_the_obj_normals(hip_lib, tmp_path):
    """the project's Cornell asset (32 triangles, vn records): make_app(smooth_normals=True), make_app with the arrays of
    abi.load_obj_normals handed to set_normals, and rtpt_app --smooth-normals give the same frames bit for bit and count the same rays"""
    import json
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import DEFAULT_SCENE, make_app
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    abi = hip_lib
    Wh, Hh, seg, n_it = 96, 64, 3, 5
    keys = ["", "J", "D"]
    tri_normals, tri_smooth = abi.load_obj_normals(DEFAULT_SCENE)
    assert tri_smooth.any() and len(tri_smooth) <= 64
    frames = []
    for how in ("switch", "arrays"):
        app = make_app(Wh, Hh, max_segments=seg, iterations=n_it, smooth_normals=how == "switch")
        if how == "arrays":
            app.backend.set_normals(tri_normals, tri_smooth)
        for k in keys:
            app.drawScene(tuple(k))
        frames.append((app.backend.ctx.readback(abi.PLANE_IMAGE), app.backend.ctx.raycount()))
        app.backend.close()
    assert np.array_equal(frames[0][0].view(np.uint32), frames[1][0].view(np.uint32)) and frames[0][1] == frames[1][1]
    binary = os.path.join(os.path.dirname(abi.LIB_PATH), "rtpt_app")
    assert os.path.exists(binary), "the C++ host is not built"
    pfm = tmp_path / "out.pfm"
    out = subprocess.run([binary, "--scene", DEFAULT_SCENE, "--smooth-normals", "--width", str(Wh), "--height", str(Hh), "--segments", str(seg),
                          "--iterations", str(n_it), "--frames", str(len(keys)), "--script", ",".join(keys), "--dump", str(pfm)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    stats = json.loads(out.stdout.strip().splitlines()[-1])
    got = np.ascontiguousarray(read_pfm(str(pfm)), np.float32)
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(frames[0][0][..., :3]).view(np.uint32))
    assert stats["rays"] == frames[0][1]
