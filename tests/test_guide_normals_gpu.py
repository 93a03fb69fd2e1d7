"""RTPT_FLAG_EXT_SMOOTH_GUIDE on the device: the guide normals K0 writes against tests/guide_normals.py bit for bit, the per-pixel-normal
filter kernels against each other and against the by-id kernels bit for bit, one float64 comparison with a measured bar, frame reuse, the
ignored cases and the hosts.  tests/test_guide_normals_cpu.py holds the numpy statements to float64 first.

Frames are 70 x 19: one full 64-pixel tile column and a partial one, two 8-row comb chunks and a partial one.  Scenes are
tests/normal_paths.py's: small (40 triangles, the id-pair-table size class), uv_sphere and half_cylinder (three instances, above 63
triangles, the BVH over triangles and over fan pairs), with their hostile records.  Every comparison covers every pixel."""
import json
import os
import subprocess

import numpy as np
import pytest

import filter_planes as FP
import gbuffer_scenes as G
import guide_normals as GN
import normal_paths as NP
import pathtrace_scenes as P
import test_pathtrace_scenes_gpu as T
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

W, H = GN.SHAPE
GUIDE = GN.SMOOTH_GUIDE
X, DIRECT, NOFUSE, EXT_ALL = 0x1, 0x4, 0x400, 0x9F0
MODEL = np.array([[0.96, 0.0, 0.28, 0.0], [0.0, 1.1, 0.0, 0.0], [-0.28, 0.0, 0.96, 0.0], [0.05, -0.02, 0.1, 1.0]], np.float32).ravel()   # column-major
MIRROR = np.array([[-1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.02, 0.0, 0.0, 1.0]], np.float32).ravel()      # det < 0


def _env(monkeypatch, trace_fusion=True, host_refit=False):
    if trace_fusion:
        monkeypatch.delenv("RTPT_NO_TRACE_FUSION", raising=False)
    else:
        monkeypatch.setenv("RTPT_NO_TRACE_FUSION", "1")
    monkeypatch.setenv("RTPT_HOST_REFIT", "1" if host_refit else "0")
    monkeypatch.delenv("RTPT_PT_WINDOW", raising=False)


def case(oracle, name, moved=False, model=None):
    if name == "small":
        assert not moved and model is None
        return NP.small_case(oracle)
    return NP.case(oracle, name, moved, model)


def context(abi, c, flags, rows=None, debug=0):
    ctx = abi.Context(T._config(abi, c.sh.scene, W, H, 2, 1, flags, rows))
    if debug:
        ctx.enable_debug(debug)
    return ctx


def upload(ctx, c, name, normals=True, smooth=None, tri_normals=None):
    if name == "small":
        ctx.scene_upload(c.sh.mesh[0], c.sh.mesh[1])
    else:
        ctx.scene_upload(c.sh.mesh[0], c.sh.mesh[1], NP.xforms())
    if normals:
        ctx.set_normals(c.tri_normals if tri_normals is None else tri_normals, c.tri_smooth if smooth is None else smooth)


def ubo_of(abi, oracle, c, model=None, cam=None):
    sc = c.sh.scene if cam is None else c.sh.scene._replace(cam=cam)
    u = T._ubo(abi, oracle, sc, W, H)
    if model is not None:
        u.model[:] = np.asarray(model, np.float32).ravel()
        u.modelPrev[:] = u.model[:]
    return u


def trace(abi, ctx, c, u, frame_no=0, cam=None):
    """K0, K1, K2 in the reference's order"""
    sc = c.sh.scene if cam is None else c.sh.scene._replace(cam=cam)
    pc = G.fill_push_constants(abi.PushConstants(), P.push_constants(sc), frame_no)
    ctx.gbuffer(u)
    ctx.temporal_gradient(pc)
    ctx.raytrace(pc)
    return pc


def filter_all(ctx, pc, u, N=3):
    pc.maxWaveletIteration = N
    for k in range(1, N + 1):
        pc.waveletIteration = k
        ctx.temporal_filter(pc, u)


def expected_plane(oracle, abi, c, nrm, u, guide=True, tri_normals=None):
    """(cells [H, W, 4], guided [H, W]) K0 must write for the posed case under ubo u (u.model is already in c's triangles)"""
    if tri_normals is not None:
        nrm = nrm._replace(tri_normals=tri_normals)
    hits = GN.k0_hits(oracle, c.sh.scene.tris, np.array(u.view[:], np.float32), np.array(u.proj[:], np.float32), W, H,
                      abi.config_default(W, H).ray_tmax)
    FP.check_ids(hits[0], len(c.sh.scene.tris))
    return GN.guide_plane(oracle, c.sh.scene.tris, nrm, len(nrm.tri_smooth), hits, guide)


# ------------------------------------------------------------------------------------------ 1. K0's plane, bit for bit
K0_CELLS = (("small", 0, True), ("small", NOFUSE, True), ("uv_sphere", 0, True), ("uv_sphere", NOFUSE, True), ("half_cylinder", 0, True),
            ("half_cylinder", 0, False), ("uv_sphere", 0, False))       # (scene, flags, the tracing launch carries K0)


@pytest.mark.parametrize("cell", K0_CELLS, ids=["-".join(str(v) for v in c) for c in K0_CELLS])
def test_k0_writes_the_guide_normals(hip_lib, oracle, monkeypatch, cell):
    """the fused launch, RTPT_FLAG_NO_FILTER_FUSION and RTPT_NO_TRACE_FUSION=1 (k_gbuffer alone); hostile records are the scenes' own"""
    abi = hip_lib
    name, flags, fused = cell
    _env(monkeypatch, trace_fusion=fused)
    c, nrm = case(oracle, name)
    u = ubo_of(abi, oracle, c)
    want, guided = expected_plane(oracle, abi, c, nrm, u)
    plain, _ = expected_plane(oracle, abi, c, nrm, u, guide=False)
    with context(abi, c, GUIDE | flags) as ctx:
        upload(ctx, c, name)
        trace(abi, ctx, c, u)
        got = ctx.debug_guide_normals()
        vis = ctx.readback(abi.PLANE_VIS_ID)
    hit = vis > 0
    assert guided.any() and (hit & ~guided).any() and (~hit).any(), cell            # guide cells, fallback cells and sky
    assert (want[guided].view(np.uint32) != plain[guided].view(np.uint32)).any(), cell
    same_bits(got, want, cell + ("guide plane",))


def _hostile_lengths(c):
    """the scene's records with every fifth one at length 1e20 (|w|^2 overflows binary32: G4) and every seventh at 1e-30"""
    n = np.array(c.tri_normals, np.float32)
    with np.errstate(over="ignore"):
        n[::5] *= np.float32(1e20)
        n[3::7] *= np.float32(1e-30)
    return n


@pytest.mark.parametrize("host_refit", [False, True], ids=["device route", "host route"])
def test_k0_follows_reposed_scenes(hip_lib, oracle, monkeypatch, host_refit):
    """moved instances, a moved model and a mirrored model (det < 0) on both re-pose routes; then records of length 1e20 and 1e-30"""
    abi = hip_lib
    _env(monkeypatch, host_refit=host_refit)
    name = "uv_sphere"
    c, nrm = case(oracle, name)
    with context(abi, c, GUIDE) as ctx:
        upload(ctx, c, name)
        steps = ((False, None), (True, None), (True, MODEL), (True, MIRROR))
        for no, (moved, model) in enumerate(steps):
            if moved and no == 1:
                ctx.scene_set_instances(NP.xforms(moved=True))
            posed, pn = case(oracle, name, moved, model)
            u = ubo_of(abi, oracle, posed, model)
            want, guided = expected_plane(oracle, abi, posed, pn, u)
            trace(abi, ctx, posed, u, no)
            same_bits(ctx.debug_guide_normals(), want, (name, host_refit, moved, model is not None and tuple(model[:3])))
            assert guided.any()
            ctx.end_frame()
        hostile = _hostile_lengths(c)
        ctx.set_normals(hostile, c.tri_smooth)
        want, guided = expected_plane(oracle, abi, posed, pn, u, tri_normals=hostile)
        before = expected_plane(oracle, abi, posed, pn, u)[1]
        assert (before & ~guided).any(), "no record of length 1e20 is hit"
        trace(abi, ctx, posed, u, len(steps))
        same_bits(ctx.debug_guide_normals(), want, (name, host_refit, "lengths"))


def test_k0_of_a_strip(hip_lib, oracle, monkeypatch):
    """a context that stores rows [8, 19): K0 per row range, the plane indexed from row_begin"""
    abi = hip_lib
    _env(monkeypatch)
    c, nrm = case(oracle, "half_cylinder")
    u = ubo_of(abi, oracle, c)
    want, _ = expected_plane(oracle, abi, c, nrm, u)
    with context(abi, c, GUIDE, rows=(8, H)) as ctx:
        upload(ctx, c, "half_cylinder")
        pc = G.fill_push_constants(abi.PushConstants(), P.push_constants(c.sh.scene), 0)
        ctx.gbuffer(u, 8, 12)
        ctx.gbuffer(u, 12, H)
        ctx.temporal_gradient(pc)
        ctx.raytrace(pc)
        same_bits(ctx.debug_guide_normals(), want[8:], ("strip",))


# ------------------------------------------------------------------------------------------ 2. nothing smooth is nothing changed
def _planes(abi, ctx, flags):
    which = dict(IMAGE=abi.PLANE_IMAGE, FILTERED=abi.PLANE_FILTERED, VIS_ID=abi.PLANE_VIS_ID, WORLDPOS=abi.PLANE_WORLDPOS, DEPTH=abi.PLANE_DEPTH,
                 GRADIENT=abi.PLANE_GRADIENT, PREVIOUS=abi.PLANE_PREVIOUS)
    if flags & 0x100:
        which.update(MOMENTS=abi.PLANE_MOMENTS, VARIANCE=abi.PLANE_VARIANCE)
    return {k: ctx.readback(v) for k, v in which.items()}


@pytest.mark.parametrize("flags", [0, X, DIRECT, NOFUSE, EXT_ALL], ids=hex)
@pytest.mark.parametrize("name", ["small", "uv_sphere"])
def test_nothing_smooth_is_nothing_changed(hip_lib, oracle, monkeypatch, name, flags):
    """the flag on a scene whose tri_smooth is all 0 against a context without it: three frames, the camera moved in between, every
    readable plane and the finished frame bit for bit.  On the small scene the flag's side runs the per-pixel comb kernel and the
    per-pixel direct kernels, the other side the id-pair table's and the by-id ones"""
    abi = hip_lib
    _env(monkeypatch)
    c, _ = case(oracle, name)
    flat = np.zeros_like(c.tri_smooth)
    cams = (None, (0.15, 0.05, 2.3), (0.15, 0.05, 2.3))
    with context(abi, c, flags) as off, context(abi, c, flags | GUIDE) as on:
        for ctx in (off, on):
            upload(ctx, c, name, smooth=flat)
        for no, cam in enumerate(cams):
            got = []
            for ctx in (off, on):
                u = ubo_of(abi, oracle, c, cam=cam)
                pc = trace(abi, ctx, c, u, no, cam)
                filter_all(ctx, pc, u)
                got.append(_planes(abi, ctx, flags))
                ctx.end_frame()
            for k in got[0]:
                same_bits(got[1][k], got[0][k], (name, hex(flags), no, k))
        cells = on.debug_guide_normals()
        tab = GN.normal_table(oracle, c.sh.scene.tris)
        same_bits(cells, tab[on.readback(abi.PLANE_PREV_VIS_ID).astype(np.int64)], (name, "the plane holds normal_tab[id]"))


# ------------------------------------------------------------------------------------------ 3. injected by-id cells
def test_injected_by_id_cells_give_the_by_id_frame(hip_lib, oracle, monkeypatch):
    """uv_sphere with its smooth normals: the plane of a context without the flag (normal_tab[id]) injected, with the same colour, depth
    and ids, into one with it — k = 1, 2, 3 and the final pass give the other context's frame"""
    abi = hip_lib
    _env(monkeypatch)
    c, _ = case(oracle, "uv_sphere")
    u = ubo_of(abi, oracle, c)
    with context(abi, c, 0) as off, context(abi, c, GUIDE) as on:
        for ctx in (off, on):
            upload(ctx, c, "uv_sphere")
        pc = trace(abi, off, c, u)
        traced, depth, vis = off.readback(abi.PLANE_IMAGE), off.readback(abi.PLANE_DEPTH), off.readback(abi.PLANE_VIS_ID)
        by_id = off.debug_guide_normals()
        filter_all(off, pc, u)
        want = off.readback(abi.PLANE_IMAGE)
        pc = trace(abi, on, c, u)
        assert (on.debug_guide_normals().view(np.uint32) != by_id.view(np.uint32)).any()
        on.set_plane(abi.PLANE_IMAGE, traced)
        on.set_plane(abi.PLANE_DEPTH, depth)
        on.set_plane(abi.PLANE_VIS_ID, vis)
        on.debug_set_guide_normals(by_id)
        filter_all(on, pc, u)
        same_bits(on.readback(abi.PLANE_IMAGE), want, ("injected by-id cells",))


# ------------------------------------------------------------------------------------------ 4. the kernel families agree
# (k, final): k <= 16 runs the comb kernel's NRM form, 17 the direct kernel by its stride; (2, "zero") is the last iteration of an even N
PASSES = ((1, False), (2, False), (3, False), (5, False), (17, False), (1, True), (3, True), (5, True), (17, True), (2, "zero"))


class _Family:
    """one context per route, all with the flag and the small scene's smooth normals, planes injected per run"""

    def __init__(self, abi, oracle, flags_list):
        self.abi = abi
        self.c, _ = case(oracle, "small")
        self.nt = len(self.c.sh.scene.tris)
        self.u = ubo_of(abi, oracle, self.c)
        self.ids = FP.id_plane("random", self.nt, W, H)
        self.img, self.depth = FP.colour_depth("bounded", self.ids, self.nt)
        self.fin = FP.final_inputs(self.ids, self.nt)
        self.u.viewPrev[:], self.u.projPrev[:] = self.fin["view_prev"], self.fin["proj_prev"]
        self.ctxs = {}
        for fl in flags_list:
            ctx = context(abi, self.c, GUIDE | fl, debug=abi.DEBUG_PREV_PIXEL)
            upload(ctx, self.c, "small")
            self.ctxs[fl] = ctx

    def run(self, fl, cells, k, final):
        """a traced frame (rtpt_raytrace starts a frame: a final pass ended the one before), every plane injected over it, one filter call"""
        abi, ctx = self.abi, self.ctxs[fl]
        src = abi.PLANE_IMAGE if k & 1 else abi.PLANE_FILTERED
        dst = abi.PLANE_IMAGE if (final is True or not k & 1) else abi.PLANE_FILTERED
        trace(abi, ctx, self.c, self.u)
        for which, arr in ((abi.PLANE_DEPTH, self.depth), (abi.PLANE_WORLDPOS, self.fin["worldpos"]), (abi.PLANE_LUT_PREV, self.fin["lut_prev"]),
                           (abi.PLANE_PREVIOUS, self.fin["history"]), (abi.PLANE_GRADIENT, self.fin["gradient"]),
                           (abi.PLANE_VIS_ID, FP.check_ids(self.ids, self.nt)), (src, self.img)):
            ctx.set_plane(which, arr)
        ctx.debug_set_guide_normals(cells)
        pc = abi.PushConstants()
        pc.frameNumber, pc.waveletIteration, pc.maxWaveletIteration = 1, k, (k + 1 if final is False else k)
        ctx.temporal_filter(pc, self.u)
        out = dict(image=ctx.readback(dst))
        if final is True:
            out["prev_pixel"] = ctx.readback(abi.PLANE_PREV_PIXEL)
        return out

    def close(self):
        for ctx in self.ctxs.values():
            ctx.close()


@pytest.mark.parametrize("kind", GN.PLANE_KINDS)
def test_kernel_families_agree_on_injected_cells(hip_lib, oracle, monkeypatch, kind):
    """the comb NRM kernel against the per-pixel direct kernel (RTPT_FLAG_DIRECT_FILTER) and against RTPT_FLAG_NO_FILTER_FUSION, fast and
    RTPT_FLAG_EXACT_FILTER, non-final and final, on smooth and hostile cells: bit for bit"""
    abi = hip_lib
    _env(monkeypatch)
    cells = GN.normal_plane(kind, W, H)
    fam = _Family(abi, oracle, [0, DIRECT, NOFUSE, X, X | DIRECT, X | NOFUSE])
    try:
        differs = 0
        for k, final in PASSES:
            for ex in (0, X):
                comb = fam.run(ex, cells, k, final)
                for route in (DIRECT, NOFUSE):
                    other = fam.run(ex | route, cells, k, final)
                    for key in comb:
                        same_bits(other[key], comb[key], (kind, k, final, hex(ex | route), key))
            if kind == "unit" and final is False:
                flat = np.array(cells)
                flat[..., :3] = (0.0, 0.0, 1.0)
                differs += int((fam.run(X, flat, k, final)["image"].view(np.uint32) != comb["image"].view(np.uint32)).any())   # (comb: the EXACT run)
        assert kind != "unit" or differs == 5, "the cells do not reach the weights"
    finally:
        fam.close()


def test_reprojection_reuse_loads_under_the_guide(hip_lib, oracle, monkeypatch):
    """five frames at rest on uv_sphere's smooth normals: the comb kernel's final pass stores its reprojected pixels, then loads them
    (RLOAD), and every finished frame is the per-pixel direct kernel's"""
    abi = hip_lib
    _env(monkeypatch)
    c, _ = case(oracle, "uv_sphere")
    u = ubo_of(abi, oracle, c)
    with context(abi, c, GUIDE) as comb, context(abi, c, GUIDE | DIRECT) as direct:
        for ctx in (comb, direct):
            upload(ctx, c, "uv_sphere")
        for no in range(5):
            got = []
            for ctx in (comb, direct):
                pc = trace(abi, ctx, c, u, no)
                filter_all(ctx, pc, u)
                got.append(ctx.readback(abi.PLANE_IMAGE))
                ctx.end_frame()
            same_bits(got[1], got[0], ("rest", no))
        assert comb.reproj_info()["loads"] > 0 and comb.reuse_info()["frames_skipped"] > 0


EXT_STRIP = (0x20, 0x40, EXT_ALL)


@pytest.mark.parametrize("ext", EXT_STRIP, ids=hex)
def test_ext_kernel_per_pixel_on_a_strip_split(hip_lib, oracle, monkeypatch, ext):
    """k_atrous_ext's per-pixel form, iterations 1 and 2 of an N = 4 frame: rows [0, 10) of a context that stores the whole frame and rows
    [10, 19) of one that stores [1, 19) are the whole frame's rows, bit for bit.  Iteration 2 reaches 4 rows (5 x 5 taps at stride 2),
    so iteration 1 runs over [0, 14) and [6, 19)"""
    abi = hip_lib
    _env(monkeypatch)
    c, _ = case(oracle, "small")
    nt = len(c.sh.scene.tris)
    ids = FP.id_plane("random", nt, W, H)
    img, depth = FP.colour_depth("bounded", ids, nt)
    fin = FP.final_inputs(ids, nt)
    cells = GN.normal_plane("unit", W, H, seed=1)
    u = ubo_of(abi, oracle, c)
    u.viewPrev[:], u.projPrev[:] = fin["view_prev"], fin["proj_prev"]
    prev_vis = FP.id_plane("blocks", nt, W, H)

    def run(rows, r1, r2):
        y0, y1 = rows
        with context(abi, c, GUIDE | ext, rows=rows) as ctx:
            upload(ctx, c, "small")
            ctx.gbuffer(u)
            ctx.sync()
            for which, arr in ((abi.PLANE_IMAGE, img), (abi.PLANE_DEPTH, depth), (abi.PLANE_WORLDPOS, fin["worldpos"]), (abi.PLANE_PREVIOUS, fin["history"]),
                               (abi.PLANE_GRADIENT, fin["gradient"]), (abi.PLANE_PREV_VIS_ID, prev_vis), (abi.PLANE_VIS_ID, ids)):
                ctx.set_plane(which, np.ascontiguousarray(arr[y0:y1]))
            ctx.set_plane(abi.PLANE_LUT_PREV, fin["lut_prev"])
            if ext & 0x100:
                ctx.set_plane(abi.PLANE_MOMENTS_PREV, np.ascontiguousarray(fin["moments_prev"][y0:y1]))
            ctx.debug_set_guide_normals(np.ascontiguousarray(cells[y0:y1]))
            pc = abi.PushConstants()
            pc.frameNumber, pc.maxWaveletIteration = 1, 4
            pc.waveletIteration = 1
            ctx.temporal_filter(pc, u, *r1)
            pc.waveletIteration = 2
            ctx.temporal_filter(pc, u, *r2)
            return ctx.readback(abi.PLANE_IMAGE)

    whole = run((0, H), (0, H), (0, H))
    top = run((0, H), (0, 14), (0, 10))
    bottom = run((1, H), (6, H), (10, H))
    same_bits(top[:10], whole[:10], (hex(ext), "rows [0, 10)"))
    same_bits(bottom[10 - 1:], whole[10:], (hex(ext), "rows [10, 19)"))
    assert np.isfinite(whole[..., :3]).any()


# ------------------------------------------------------------------------------------------ 5. against float64
@pytest.mark.parametrize("stride", [1, 2, 3, 5])
def test_per_pixel_filter_against_float64(hip_lib, oracle, monkeypatch, stride):
    """one non-final RTPT_FLAG_EXACT_FILTER iteration on bounded planes with per-pixel unit normals against guide_normals.atrous_once_numpy_px
    at float64.  The bar is measured as in test_filter_planes_cpu.py: 4 x max |r32 - r64| of the numpy statement itself"""
    abi = hip_lib
    _env(monkeypatch)
    cells = GN.normal_plane("unit", W, H)
    fam = _Family(abi, oracle, [X])
    try:
        got = fam.run(X, cells, stride, False)["image"][..., :3].astype(np.float64)
        cfg = abi.config_default(W, H)
        kw = dict(sigma_n=cfg.sigma_n, sigma_z=cfg.sigma_z, sigma_l=cfg.sigma_l)
        r64 = GN.atrous_once_numpy_px(np.float64, fam.img, fam.depth, cells, stride, **kw)
        r32 = GN.atrous_once_numpy_px(np.float32, fam.img, fam.depth, cells, stride, **kw).astype(np.float64)
    finally:
        fam.close()
    bar = 4.0 * np.abs(r32 - r64).max()
    err = np.abs(got - r64).max()
    print(f"stride {stride}: device vs float64 {err:.3e}, bar {bar:.3e}")
    assert 0 < bar < 1e-3 and err <= bar, (err, bar)


# ------------------------------------------------------------------------------------------ 6. reuse and lifetime
def test_reuse_and_lifetime(hip_lib, oracle, monkeypatch):
    abi = hip_lib
    _env(monkeypatch)
    name = "uv_sphere"
    c, _ = case(oracle, name)
    u = ubo_of(abi, oracle, c)

    history = np.zeros((H, W, 4), np.float32)
    history[..., :3] = 0.25

    def one(ctx, no, inject_ids=False, same_history=False):
        pc = trace(abi, ctx, c, u, no)
        if inject_ids:
            ctx.set_plane(abi.PLANE_VIS_ID, ctx.readback(abi.PLANE_VIS_ID))      # the plane no longer matches the ids: the stale plane
        if same_history:
            ctx.set_plane(abi.PLANE_PREVIOUS, history)       # (the two contexts' earlier frames, and so their histories, differ)
        filter_all(ctx, pc, u)
        img = ctx.readback(abi.PLANE_IMAGE)
        ctx.end_frame()
        return img

    with context(abi, c, GUIDE) as on, context(abi, c, 0) as off:
        for ctx in (on, off):
            upload(ctx, c, name)
        skipped = []
        for no in range(4):
            a, b = one(on, no), one(off, no)
            skipped.append(on.reuse_info()["frames_skipped"])
        assert skipped[-1] > skipped[1] and skipped[-1] == off.reuse_info()["frames_skipped"], skipped     # at rest K0 is not launched
        assert (a.view(np.uint32) != b.view(np.uint32)).any(), "the guide changes no filtered pixel"
        before = on.debug_guide_normals()
        # other normals: the next frame runs K0 again and the plane changes
        other = np.array(c.tri_normals, np.float32).reshape(-1, 3, 3)[:, ::-1, :].reshape(-1, 9).copy()
        for ctx in (on, off):
            ctx.set_normals(other, c.tri_smooth)
        one(on, 4), one(off, 4)
        assert on.reuse_info()["frames_skipped"] == skipped[-1]
        assert (on.debug_guide_normals().view(np.uint32) != before.view(np.uint32)).any()
        # the stale plane: filtered with the triangles' normals, the frame of the context without the flag
        same_bits(one(on, 5, inject_ids=True, same_history=True), one(off, 5, inject_ids=True, same_history=True), ("stale plane",))
        # removed: the flag-off bits again
        for ctx in (on, off):
            ctx.set_normals(None)
        for no in (6, 7):
            same_bits(one(on, no), one(off, no), ("removed", no))


# ------------------------------------------------------------------------------------------ 7. ignored means untouched
@pytest.mark.parametrize("name", ["small", "half_cylinder"])
def test_ignored_means_untouched(hip_lib, oracle, monkeypatch, name):
    """the flag on a scene without normals: the frames and the device memory of a context without it; without the flag a small scene
    with normals has no per-pixel plane and refuses an injected one"""
    abi = hip_lib
    _env(monkeypatch)
    c, _ = case(oracle, name)
    u = ubo_of(abi, oracle, c)
    frames, held = [], []
    for flags in (0, GUIDE):
        base = abi.live_device_bytes()
        with context(abi, c, flags) as ctx:
            upload(ctx, c, name, normals=False)
            imgs = []
            for no in range(3):
                pc = trace(abi, ctx, c, u, no)
                filter_all(ctx, pc, u)
                imgs.append(ctx.readback(abi.PLANE_IMAGE))
                ctx.end_frame()
            held.append(abi.live_device_bytes() - base)
            frames.append(imgs)
    assert held[0] == held[1] > 0, held
    for no in range(3):
        same_bits(frames[1][no], frames[0][no], (name, "no normals", no))
    if name == "small":
        with context(abi, c, 0) as ctx:
            upload(ctx, c, name)
            trace(abi, ctx, c, u)
            for call in (ctx.debug_guide_normals, lambda: ctx.debug_set_guide_normals(np.zeros((H, W, 4), np.float32))):
                with pytest.raises(abi.RtptError) as e:
                    call()
                assert e.value.code == abi.RTPT_E_INVALID


# ------------------------------------------------------------------------------------------ 8. the hosts
def test_hosts_apply_the_switch(hip_lib, tmp_path):
    """the project's Cornell asset (32 triangles, vn records): make_app(smooth_normals=True, smooth_guide=True), the binding with the
    loader's arrays and the flag, and rtpt_app --smooth-normals --smooth-guide give the same frames bit for bit; without smooth_normals
    the switch changes nothing"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import DEFAULT_SCENE, make_app
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    abi = hip_lib
    Wh, Hh, seg, n_it = 96, 64, 3, 5
    keys = ["", "J", "D"]
    tri_normals, tri_smooth = abi.load_obj_normals(DEFAULT_SCENE)
    frames = {}
    for how in ("switch", "arrays", "plain", "guide alone", "no switch at all"):
        app = make_app(Wh, Hh, max_segments=seg, iterations=n_it, smooth_normals=how in ("switch", "plain"), smooth_guide=how in ("switch", "guide alone"),
                       flags=abi.FLAG_EXT_SMOOTH_GUIDE if how == "arrays" else 0)
        if how == "arrays":
            app.backend.set_normals(tri_normals, tri_smooth)
        for k in keys:
            app.drawScene(tuple(k))
        frames[how] = app.backend.ctx.readback(abi.PLANE_IMAGE)
        if how == "switch":
            assert app.backend.ctx.debug_guide_normals().shape == (Hh, Wh, 4)
        app.backend.close()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(frames["switch"]), bits(frames["arrays"]))
    assert not np.array_equal(bits(frames["switch"]), bits(frames["plain"])), "the guide changes no pixel of the Cornell box"
    assert np.array_equal(bits(frames["guide alone"]), bits(frames["no switch at all"]))
    binary = os.path.join(os.path.dirname(abi.LIB_PATH), "rtpt_app")
    assert os.path.exists(binary), "the C++ host is not built"
    pfm = tmp_path / "out.pfm"
    out = subprocess.run([binary, "--scene", DEFAULT_SCENE, "--smooth-normals", "--smooth-guide", "--width", str(Wh), "--height", str(Hh), "--segments",
                          str(seg), "--iterations", str(n_it), "--frames", str(len(keys)), "--script", ",".join(keys), "--dump", str(pfm)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    json.loads(out.stdout.strip().splitlines()[-1])
    got = np.ascontiguousarray(read_pfm(str(pfm)), np.float32)
    assert np.array_equal(bits(got), bits(frames["switch"][..., :3]))
