"""The a-trous filter kernels (k_atrous, k_atrous_ext, k_atrous_comb_sh, k_atrous_chain, the sliding-window variant) on
INJECTED planes against the oracle: every other GPU test feeds them frames rendered from the Cornell box or the lattice —
colours in [0, 1], smooth depth, a dozen id pairs, camera steps of 0.1.  Here the scene is a triangle soup with degenerate
members, the ids read every entry of the id-pair table, colour and depth are bounded / wide / overflowing / subnormal /
non-finite / flat, and the final pass reprojects arbitrary world positions through an unrelated previous LUT
(tests/filter_planes.py; its claims are checked in tests/test_filter_planes_cpu.py).

Harness: upload the scene, rtpt_gbuffer once (the per-id tables are built there), rtpt_set_plane every plane, rtpt_temporal_filter
for k = 1..N, read back; the oracle chains oracle.atrous the same way with oracle.lut(tris, identity).

  EXACT (0x1)    every route and class: bit for bit the oracle's, PLANE_PREV_PIXEL too after an odd final pass.  NaNs are
                 compared as positions (payload and sign differ between x86 and gfx950), everything else as bits.
  fast           every route and class: bit for bit the fast direct kernel's (RTPT_FLAG_DIRECT_FILTER) on the same planes;
                 the fast direct kernel within FILTER_TOL of the oracle on bounded and flat planes, every pixel, and with
                 the oracle's non-finite positions on planted planes.

Which kernel a route runs is taken from the documented flags, thresholds and environment (api_passes.hip, launch_atrous): the
timing table tells a chained launch from a single one and that is asserted, but it has one slot (k_atrous / k_atrous_final) for
the comb and the direct kernel alike — a route that fell back to the direct kernel would compare equal.  For the same reason
the three direct_* routes of the fast test compare the direct kernel with itself; they are there for the EXACT test.

Largest err / lim of the fast direct kernel against the oracle per flag set (lim = tol (1 + |ref|), tol 1e-5 plain, 1e-4
extension modes; test_fast_direct_kernel_within_filter_tol prints them), measured on an MI355X:
  0: 0.028   0x10: 0.0049   0x20: 0.0017   0x40: 0.0013   0x80: 0.0024   0xF0: 0.0063   0x100: 0.015   0x1F0: 0.0037
  0x900: 0.0017   0x9F0: 0.0047"""
import numpy as np
import pytest

import filter_planes as FP
from filter_planes import same_bits

pytestmark = pytest.mark.gpu

X, DIRECT, NOFUSE = 0x1, 0x4, 0x400
EXT_SETS = (0x10, 0x20, 0x40, 0x80, 0xF0, 0x100, 0x1F0, 0x900, 0x9F0)
EYE = np.eye(4, dtype=np.float32).ravel()

_planes_cache, _oracle_cache, _gpu_cache = {}, {}, {}


# ------------------------------------------------------------------------------------------ inputs
def _scene(T):
    """T: a triangle count (filter_planes.soup), ("cone", count) (cone_soup: large, distinct pair weights) or "grid" """
    if T == "grid":
        return FP.facing_grid()
    return FP.cone_soup(T[1]) if isinstance(T, tuple) else FP.soup(T)


def _set(mat, values):
    mat[:] = np.asarray(values, np.float32).ravel()


def _ubo(cls, W, H, fin):
    """model identity; view / proj: a camera at the origin looking down -z (what rtpt_gbuffer renders; its planes are
    overwritten except on the per-pixel-normal route); viewPrev / projPrev: the test's own (filter_planes.prev_matrices)"""
    from oracle import oracle as O
    u = cls()
    _set(u.model, EYE)
    _set(u.modelPrev, EYE)
    _set(u.view, O.look_at((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0)))
    proj = O.perspective(np.float32(0.4), np.float32(W) / np.float32(H), 0.1, 10.0)
    proj[5] *= -1
    _set(u.proj, proj)
    _set(u.viewPrev, fin["view_prev"])
    _set(u.projPrev, fin["proj_prev"])
    return u


def planes(oracle, T, W, H, kind, cls, finite=False, roll=0):
    """everything a run injects, once per key.  kind 'gbuffer': the ids (world positions, depth) are the G-buffer's own
    (oracle.gbuffer), for the route that must not inject VIS_ID.  finite: ids without the all-identical-vertex triangle.
    roll: the id plane moved down by that many rows (a pair plane then starts at a strip's first stored row)."""
    key = (T, W, H, kind, cls, finite) + ((roll,) if roll else ())
    if key in _planes_cache:
        return _planes_cache[key]
    tris = _scene(T)
    nt = len(tris)
    p = dict(key=key, T=T, nt=nt, W=W, H=H, tris=tris, lut=oracle.lut(tris, EYE))
    if kind == "gbuffer":
        fin0 = dict(zip(("view_prev", "proj_prev"), FP.prev_matrices()))
        cfg = oracle.config_default(W, H)
        ids, wp, gdepth = oracle.gbuffer(cfg, tris, _ubo(oracle.Ubo, W, H, fin0))
    else:
        ids = np.roll(np.array(FP.id_plane(kind, nt, W, H)), roll, axis=0)
    if finite:
        ids = FP.without_point(ids)
    FP.check_ids(ids, nt)
    p["ids"] = ids
    p["img"], p["depth"] = FP.colour_depth(cls, ids, nt)
    fin = FP.final_inputs(ids, nt)
    if kind == "gbuffer":
        fin["worldpos"] = wp
    p.update(fin)
    # where the pixels land in the previous frame (one oracle pass), so that the previous ids can agree with some of them
    cfg = oracle.config_default(W, H)
    pc = oracle.PushConstants()
    pc.waveletIteration = pc.maxWaveletIteration = 1
    pc.frameNumber = 1
    _, pp = oracle.atrous(cfg, pc, _ubo(oracle.Ubo, W, H, fin), p["img"], p["depth"], ids, p["lut"], p["lut_prev"], p["worldpos"],
                          p["history"], want_prev_pixel=True)
    p["prev_vis"] = FP.prev_ids(ids, nt, pp)
    p["landing"] = pp                      # [H, W, 2] the reprojected pixels (tests/strip_planes.py counts where they land)
    _planes_cache[key] = p
    return p


# ------------------------------------------------------------------------------------------ the two sides
def oracle_run(oracle, p, ext, N, frame):
    """the whole-frame reference.  out["iters"][k - 1]: (image, variance) after iteration k (what a strip's neighbour sends
    before iteration k + 1); p["prev_vis_moments"]: previous ids for the moment accumulation alone, where they differ"""
    key = (p["key"], ext, N, frame)
    if key in _oracle_cache:
        return _oracle_cache[key]
    W, H = p["W"], p["H"]
    cfg = oracle.config_default(W, H)
    cfg.ext_flags = ext
    pc = oracle.PushConstants()
    pc.frameNumber, pc.maxWaveletIteration = frame, N
    ubo = _ubo(oracle.Ubo, W, H, p)
    out = dict(moments=None, variance=None, prev_pixel=None, iters=[])
    var = None
    if ext & 0x100:
        pc.waveletIteration = 1
        out["moments"], var = oracle.moments(cfg, pc, ubo, p["img"], p["ids"], p["worldpos"], p["lut_prev"],
                                             p.get("prev_vis_moments", p["prev_vis"]), p["moments_prev"])
    cur = p["img"]
    for k in range(1, N + 1):
        pc.waveletIteration = k
        res = oracle.atrous(cfg, pc, ubo, cur, p["depth"], p["ids"], p["lut"], p["lut_prev"], p["worldpos"], p["history"],
                            want_prev_pixel=(k == N), gradient=p["gradient"], prev_vis=p["prev_vis"], var_in=var)
        if var is not None:
            var, res = res[-1], res[:-1]
        cur = res[0] if isinstance(res, tuple) else res
        out["iters"].append((cur, var))
        if k == N:
            out["prev_pixel"] = res[1]
    out["image"], out["variance"] = cur, var
    _oracle_cache[key] = out
    return out


def gpu_run(abi, p, flags, N, frame, *, gbuffer=True, inject_ids=True, timing=False, present=False, reupload=None, inject_lut_prev=True):
    """one context, one filtered frame.  gbuffer=False: the filter is the first pass after the upload (it has to build the
    per-id tables itself); reupload: a scene uploaded (and rendered) BEFORE p's, whose tables must not survive."""
    W, H, nt = p["W"], p["H"], p["nt"]
    cfg = abi.config_default(W, H)
    cfg.flags = flags
    ctx = abi.Context(cfg)
    try:
        ctx.enable_debug(abi.DEBUG_PREV_PIXEL)
        ubo = _ubo(abi.Ubo, W, H, p)
        if reupload is not None:
            ctx.scene_upload(*FP.mesh_of(reupload))
            ctx.gbuffer(ubo)
            ctx.sync()
        ctx.scene_upload(*FP.mesh_of(p["tris"]))
        out = {}
        if gbuffer:
            ctx.gbuffer(ubo)
            if not inject_ids:
                out["vis"] = ctx.readback(abi.PLANE_VIS_ID)
        inject = [(abi.PLANE_IMAGE, p["img"]), (abi.PLANE_DEPTH, p["depth"]), (abi.PLANE_WORLDPOS, p["worldpos"]),
                  (abi.PLANE_LUT_PREV, p["lut_prev"]), (abi.PLANE_PREVIOUS, p["history"]), (abi.PLANE_GRADIENT, p["gradient"]),
                  (abi.PLANE_PREV_VIS_ID, FP.check_ids(p["prev_vis"], nt))]
        if not inject_lut_prev:
            inject = [(w, a) for (w, a) in inject if w != abi.PLANE_LUT_PREV]
        if inject_ids:
            inject.append((abi.PLANE_VIS_ID, FP.check_ids(p["ids"], nt)))   # (drops the G-buffer's normal plane)
        if flags & 0x100:
            inject.append((abi.PLANE_MOMENTS_PREV, p["moments_prev"]))
        for which, arr in inject:
            ctx.set_plane(which, arr)
        if timing:
            ctx.timing_enable(1)
        img8 = None
        if present:
            import torch
            img8 = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
            torch.cuda.synchronize()
            ctx.present_target(img8[0].data_ptr(), 0, H)
        pc = abi.PushConstants()
        pc.frameNumber, pc.maxWaveletIteration = frame, N
        for k in range(1, N + 1):
            pc.waveletIteration = k
            ctx.temporal_filter(pc, ubo)
        out["image"] = ctx.readback(abi.PLANE_IMAGE)
        out["prev_pixel"] = ctx.readback(abi.PLANE_PREV_PIXEL) if N & 1 else None
        if flags & 0x100:
            out["moments"] = ctx.readback(abi.PLANE_MOMENTS)
            out["variance"] = ctx.readback(abi.PLANE_VARIANCE)
        if present:
            ctx.present(img8[0].data_ptr(), 0, H)     # returns at once where the final pass wrote the rows itself
            ctx.present_target(None)
            ctx.present(img8[1].data_ptr(), 0, H)     # k_present
            ctx.sync()
            out["present"] = [t.cpu().numpy() for t in img8]
        if timing:
            out["timing"] = {k: v[1] for k, v in ctx.timing_collect().items()}
        return out
    finally:
        ctx.close()


def compare_exact(got, ref, tag, N, ext=0):
    same_bits(got["image"], ref["image"], tag + ("image",))
    if N & 1:
        same_bits(got["prev_pixel"], ref["prev_pixel"], tag + ("prev_pixel",))
    if ext & 0x100:
        same_bits(got["moments"], ref["moments"], tag + ("moments",))
        same_bits(got["variance"], ref["variance"], tag + ("variance",))


def compare_runs(a, b, tag, N, ext=0):
    same_bits(a["image"], b["image"], tag + ("image",))
    if N & 1:
        same_bits(a["prev_pixel"], b["prev_pixel"], tag + ("prev_pixel",))
    if ext & 0x100:
        same_bits(a["moments"], b["moments"], tag + ("moments",))
        same_bits(a["variance"], b["variance"], tag + ("variance",))


# ------------------------------------------------------------------------------------------ routes and cases
CHAIN_ENV = {"RTPT_CHAIN_MIN_PIXELS": "0"}
# name -> (T, flags, environment read by rtpt_create, a chained launch is expected)
ROUTES = {
    # k_atrous
    "direct_flag_T40": (40, DIRECT, {}, False),
    "direct_T64_injected_ids": (64, 0, {}, False),
    "direct_T100_injected_ids": (100, NOFUSE, {}, False),
    # k_atrous_comb_sh, id-pair table in LDS
    "comb_pair_T1": (1, NOFUSE, {}, False),
    "comb_pair_T40": (40, NOFUSE, {}, False),
    "comb_pair_T63": (63, NOFUSE, {}, False),
    "default_T40": (40, 0, {}, False),
    # k_atrous_chain
    "chain_max2_final0": (40, 0, dict(CHAIN_ENV, RTPT_CHAIN_MAX="2", RTPT_CHAIN_FINAL="0"), True),
    "chain_max2_final1": (63, 0, dict(CHAIN_ENV, RTPT_CHAIN_MAX="2", RTPT_CHAIN_FINAL="1"), True),
    "chain_max3_final0": (63, 0, dict(CHAIN_ENV, RTPT_CHAIN_MAX="3", RTPT_CHAIN_FINAL="0"), True),
    "chain_max3_final1": (40, 0, dict(CHAIN_ENV, RTPT_CHAIN_MAX="3", RTPT_CHAIN_FINAL="1"), True),
}
NS = (5, 3, 2, 1)


def cases(route_index, T):
    """one case per class: shapes, id kinds, N (odd and even) and frame 0 / > 0 rotate with the route, so that over the
    routes every class meets every shape.  The pair planes need 2 x 861 (T = 40) / 2 x 2080 (T = 63) pixels."""
    out = []
    for ci, cls in enumerate(FP.CLASSES):
        v = route_index + ci
        W, H = FP.SHAPES[v % len(FP.SHAPES)]
        kind = FP.ID_KINDS[v % len(FP.ID_KINDS)]
        out.append((W, H, kind, cls, NS[(v // 2) % len(NS)], (v + 1) % 2))
    return out


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _direct(abi, p, flags, N, frame):
    """the direct-load kernel on the same planes (cached: many routes share planes)"""
    key = (p["key"], flags, N, frame)
    if key not in _gpu_cache:
        _gpu_cache[key] = gpu_run(abi, p, flags | DIRECT, N, frame)
    return _gpu_cache[key]


# ------------------------------------------------------------------------------------------ the plain filter
@pytest.mark.parametrize("route", list(ROUTES))
def test_exact_route_equals_the_oracle(hip_lib, oracle, monkeypatch, route):
    T, flags, env, chained = ROUTES[route]
    _env(monkeypatch, env)
    ran_chain = 0
    for (W, H, kind, cls, N, frame) in cases(list(ROUTES).index(route), T):
        p = planes(oracle, T, W, H, kind, cls)
        got = gpu_run(hip_lib, p, flags | X, N, frame, timing=True)
        compare_exact(got, oracle_run(oracle, p, 0, N, frame), (route, W, H, kind, cls, N, frame), N)
        tm = got["timing"]
        n_chain = tm["k_atrous_chain"] + tm["k_atrous_chain_final"]
        assert n_chain + tm["k_atrous"] + tm["k_atrous_final"] >= 1
        if not chained:
            assert n_chain == 0, (route, tm)
        elif N >= 2:
            assert n_chain >= 1, (route, N, tm)
        ran_chain += n_chain
    assert bool(ran_chain) == chained


@pytest.mark.parametrize("route", list(ROUTES))
def test_fast_route_equals_the_fast_direct_kernel(hip_lib, oracle, monkeypatch, route):
    T, flags, env, _ = ROUTES[route]
    for (W, H, kind, cls, N, frame) in cases(list(ROUTES).index(route), T):
        p = planes(oracle, T, W, H, kind, cls)
        want = _direct(hip_lib, p, 0, N, frame)
        with monkeypatch.context() as m:
            _env(m, env)
            got = gpu_run(hip_lib, p, flags, N, frame)
        compare_runs(got, want, (route, W, H, kind, cls, N, frame), N)


@pytest.mark.parametrize("T,shape", [(40, (70, 37)), (63, (130, 33))])
@pytest.mark.parametrize("exact", [1, 0])
def test_every_pair_table_entry(hip_lib, oracle, monkeypatch, T, shape, exact):
    """pairs_h / pairs_v: every (centre, neighbour) id pair is a stride-1 tap, and in the cone soup every entry between
    ordinary triangles is a distinct weight in (0.2, 1] (test_filter_planes_cpu.py asserts both), so a wrong, unwritten or
    mis-staged entry, a wrong row stride or size of the (T+1)^2 table — k_pair_weights' or the LDS copy's of the comb and
    chain kernels — changes a pixel of iteration 1.  (A transposed index alone cannot show: dot(n_p, n_q) commutes product
    by product, the table is symmetric bit for bit.)  Separate passes (comb) and chained; EXACT against the oracle, fast
    against the direct kernel, which gathers normals and never reads the table."""
    W, H = shape
    for kind in ("pairs_h", "pairs_v"):
        p = planes(oracle, ("cone", T), W, H, kind, "bounded")
        for N in (1, 2):
            want = oracle_run(oracle, p, 0, N, 0) if exact else _direct(hip_lib, p, 0, N, 0)
            for name, flags, env in (("comb", NOFUSE, {}), ("chain", 0, dict(CHAIN_ENV, RTPT_CHAIN_MAX="2"))):
                with monkeypatch.context() as m:
                    _env(m, env)
                    got = gpu_run(hip_lib, p, flags | exact, N, 0, timing=True)
                (compare_exact if exact else compare_runs)(got, want, (name, T, kind, N, exact), N)
                if name == "chain" and N == 2:
                    assert got["timing"]["k_atrous_chain"] == 1, got["timing"]


@pytest.mark.parametrize("exact", [1, 0])
def test_last_staged_stride_and_the_first_direct_one(hip_lib, oracle, exact):
    """k = 16 is the widest stride the comb kernel stages, k = 17 runs in the direct kernel (T = 40, also with
    RTPT_FLAG_NO_FILTER_FUSION): N = 16 and N = 17 on 130 x 33, strides far beyond the frame height, every class"""
    W, H, T = 130, 33, 40
    for ci, cls in enumerate(FP.CLASSES):
        p = planes(oracle, T, W, H, FP.ID_KINDS[ci % 4], cls)
        for N in (16, 17):
            frame = (ci + N) % 2
            want = oracle_run(oracle, p, 0, N, frame) if exact else _direct(hip_lib, p, 0, N, frame)
            got = gpu_run(hip_lib, p, (NOFUSE if ci % 2 else 0) | exact, N, frame, timing=True)
            (compare_exact if exact else compare_runs)(got, want, ("k16/17", cls, N, exact), N)
            assert got["timing"]["k_atrous"] + got["timing"]["k_atrous_final"] == N


@pytest.mark.parametrize("exact", [1, 0])
def test_per_pixel_normal_route(hip_lib, oracle, exact):
    """T >= 64 with the G-buffer's OWN ids: the comb kernel stages the normal plane k_gbuffer wrote (rtpt_set_plane(VIS_ID)
    would drop it, so ids and normals stay the G-buffer's; every other plane is injected).  100 triangles facing the camera,
    each quad tilted by itself."""
    for ci, cls in enumerate(FP.CLASSES):
        W, H = ((130, 33), (70, 37), (65, 7))[ci % 3]
        N, frame = NS[ci % 4], ci % 2
        p = planes(oracle, "grid", W, H, "gbuffer", cls)
        assert p["nt"] == 100 and len(np.unique(p["ids"])) > (20 if H > 7 else 5), "the grid is in view"
        got = gpu_run(hip_lib, p, exact, N, frame, inject_ids=False)
        assert np.array_equal(got["vis"], p["ids"]), "VIS_ID is oracle.gbuffer's"
        if exact:
            compare_exact(got, oracle_run(oracle, p, 0, N, frame), ("nrm", W, H, cls, N, frame), N)
        else:
            compare_runs(got, gpu_run(hip_lib, p, DIRECT, N, frame, inject_ids=False), ("nrm", W, H, cls, N, frame), N)


@pytest.mark.parametrize("g", [2, 3])
def test_sliding_window_variant(hip_lib, oracle, monkeypatch, g):
    """RTPT_CHAIN_SW=1 (only in -DRTPT_AB_VARIANTS=1 builds): the same planes, the same bits"""
    if not hasattr(hip_lib.load(), "rtpt_debug_ab_variants"):
        pytest.skip("the library was built without the A/B variants (scripts/build_variant.sh ab -DRTPT_AB_VARIANTS=1, RTPT_LIB_PATH)")
    _env(monkeypatch, dict(CHAIN_ENV, RTPT_CHAIN_SW="1", RTPT_CHAIN_SW_G1=str(g), RTPT_CHAIN_SW_G3=str(g)))
    for (W, H, kind, cls, N, frame) in cases(g, 40):
        p = planes(oracle, 40, W, H, kind, cls)
        for exact in (1, 0):
            got = gpu_run(hip_lib, p, exact, N, frame)
            if exact:
                compare_exact(got, oracle_run(oracle, p, 0, N, frame), ("sw", g, W, H, cls, N), N)
            else:
                compare_runs(got, _direct(hip_lib, p, 0, N, frame), ("sw", g, W, H, cls, N), N)


# ------------------------------------------------------------------------------------------ extension modes
@pytest.mark.parametrize("ext", EXT_SETS)
def test_extension_modes(hip_lib, oracle, ext):
    """every flag set LDS-staged (T = 40: k_atrous_comb_sh's extension instances) and direct (0x4: k_atrous_ext), every class:
    EXACT equals the oracle bit for bit — image, reprojected pixels, PLANE_MOMENTS (oracle.moments) and the filtered
    PLANE_VARIANCE (oracle.atrous on oracle.moments' variance, through oracle.var_prefilter's arithmetic with 0x800) —
    and the fast staged kernel equals the fast direct one.  T = 64 once per flag set: k_atrous_ext alone."""
    ei = EXT_SETS.index(ext)
    for ci, cls in enumerate(FP.CLASSES):
        v = ei + ci
        W, H = FP.SHAPES[v % 5]
        kind, N, frame = FP.ID_KINDS[v % 4], NS[v % 4], (v // 2) % 2
        p = planes(oracle, 40, W, H, kind, cls)
        ref = oracle_run(oracle, p, ext, N, frame)
        tag = (hex(ext), W, H, kind, cls, N, frame)
        compare_exact(gpu_run(hip_lib, p, ext | X, N, frame), ref, tag + ("staged",), N, ext)
        compare_exact(gpu_run(hip_lib, p, ext | X | DIRECT, N, frame), ref, tag + ("direct",), N, ext)
        compare_runs(gpu_run(hip_lib, p, ext, N, frame), _direct(hip_lib, p, ext, N, frame), tag + ("fast",), N, ext)
    p = planes(oracle, 64, 70, 37, "random", "planted")
    compare_exact(gpu_run(hip_lib, p, ext | X, 3, 1), oracle_run(oracle, p, ext, 3, 1), (hex(ext), "T64"), 3, ext)


# ------------------------------------------------------------------------------------------ fast against the oracle
@pytest.mark.parametrize("ext", (0,) + EXT_SETS)
def test_fast_direct_kernel_within_filter_tol(hip_lib, oracle, ext):
    """bounded and flat planes, every pixel: |got - ref| <= tol (1 + |ref|) over rgb, tol = 1e-5 (1e-4 in the extension
    modes) — the project's FILTER_TOL (test_fuzz_gpu.py).  The ids leave out the all-identical-vertex triangle (its pixels
    are 0 / 0 in the oracle and spread); then the oracle is finite everywhere (asserted; test_filter_planes_cpu.py), except
    under 0x10 where a NaN gradient makes the blend NaN in both.  Largest err / lim measured on an MI355X: 0.028 plain,
    0.0013 .. 0.015 in the extension modes (the module docstring has all ten); printed on every run."""
    tol = 1e-4 if ext else 1e-5
    worst = 0.0
    for cls in ("bounded", "flat"):
        for (T, (W, H), kind, N, frame) in ((40, (130, 33), "random", 5, 1), (63, (70, 37), "blocks", 3, 1), (100, (65, 7), "random", 2, 0)):
            p = planes(oracle, T, W, H, kind, cls, finite=True)
            ref = oracle_run(oracle, p, ext, N, frame)["image"]
            got = _direct(hip_lib, p, ext, N, frame)["image"]
            nan_ok = np.isnan(p["gradient"][..., 0]) if (ext & 0x10 and N & 1 and frame) else np.zeros((H, W), bool)
            assert np.array_equal(np.isnan(ref[..., :3]).any(-1), nan_ok & np.isnan(ref[..., :3]).any(-1))
            assert np.isfinite(ref[~nan_ok]).all(), "the reference needs no finite mask"
            same = np.isnan(got) == np.isnan(ref)
            assert same.all(), (hex(ext), cls, T, "non-finite positions")
            fin = ~np.isnan(ref[..., :3]).any(-1)
            err = np.linalg.norm((got[..., :3] - ref[..., :3]).astype(np.float64), axis=-1)[fin]
            lim = tol * (1.0 + np.linalg.norm(ref[..., :3].astype(np.float64), axis=-1))[fin]
            ratio = float((err / lim).max())
            print(f"FILTER_TOL ratio ext={ext:#x} {cls} T={T} {W}x{H} N={N}: {ratio:.3e}")
            worst = max(worst, ratio)
            assert (err <= lim).all(), (hex(ext), cls, T, ratio)
    print(f"FILTER_TOL worst ext={ext:#x}: {worst:.3e}")


@pytest.mark.parametrize("ext", (0, 0xF0, 0x9F0))
def test_fast_direct_kernel_non_finite_positions(hip_lib, oracle, ext):
    """planted planes: where the oracle's result is NaN / +Inf / -Inf, so is the fast kernel's, and nowhere else"""
    for (T, (W, H), kind, N, frame) in ((40, (130, 33), "random", 3, 1), (63, (70, 37), "blocks", 2, 0), (100, (65, 7), "random", 1, 1)):
        p = planes(oracle, T, W, H, kind, "planted")
        ref = oracle_run(oracle, p, ext, N, frame)["image"]
        got = _direct(hip_lib, p, ext, N, frame)["image"]
        for name, f in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
            assert np.array_equal(f(got), f(ref)), (hex(ext), T, name, int(f(got).sum()), int(f(ref).sum()),
                                                    np.argwhere(f(got) != f(ref))[:4].tolist())
        assert np.isnan(ref).any()


# ------------------------------------------------------------------------------------------ present
def _present_planes(oracle, T, W, H, finite=False):
    """colours that end up < 0, > 1, NaN, +-Inf and within an ulp of the rounding boundaries (n + 0.5) / 255 of unorm8: depths
    1000 apart give every tap but the pixel's own the weight exp(-1000) = 0, so a pixel keeps its colour up to rounding"""
    p = dict(planes(oracle, T, W, H, "random", "bounded", finite=finite))
    p["key"] = p["key"] + ("present",)
    ids = p["ids"]
    rng = np.random.default_rng(5)
    n = rng.integers(0, 255, (H, W, 3))
    edge = ((n + 0.5) / 255.0).astype(np.float32)
    step = rng.integers(-1, 2, (H, W, 3))
    edge = np.where(step < 0, np.nextafter(edge, np.float32(-1)), np.where(step > 0, np.nextafter(edge, np.float32(2)), edge)).astype(np.float32)
    img = np.zeros((H, W, 4), np.float32)
    img[..., :3] = edge
    special = np.array([-0.25, 1.5, -np.inf, np.inf, 0.0, 1.0, 3e38, -1e-40, np.nan], np.float32)
    pick = rng.random((H, W)) < 0.15
    img[pick, 0] = rng.choice(special[:-1], int(pick.sum()))
    img[pick, 2] = rng.choice(special[:-1], int(pick.sum()))
    if H * W > 9:
        img[H // 2, W // 2, 1] = np.nan
    p["img"] = img
    p["depth"] = (np.arange(H * W, dtype=np.float32) * np.float32(1000.0)).reshape(H, W)
    hist = p["history"] * np.float32(0.3)
    hist[..., 0][rng.random((H, W)) < 0.1] = np.inf          # (a pixel's own Inf turns NaN in the filter: Inf - Inf; the
    hist[..., 1][rng.random((H, W)) < 0.1] = -np.inf         # history's reaches the blend as it is)
    p["history"] = hist
    return p


@pytest.mark.parametrize("T,exact", [(40, 0), (40, 1), (100, 0)])
def test_present_bytes(hip_lib, oracle, T, exact):
    """the fused store of the final pass (id-pair routes, rtpt_present_target) and k_present, byte for byte
    oracle.present_bgra8 of the final image; T = 100 (direct final pass) has k_present serve both"""
    for (W, H) in ((130, 33), (7, 3)):
        p = _present_planes(oracle, T, W, H)
        for frame in (0, 1):
            got = gpu_run(hip_lib, p, exact, 1, frame, present=True, timing=True)
            final = got["image"]
            if exact:
                same_bits(final, oracle_run(oracle, p, 0, 1, frame)["image"], ("present", T, W, H, frame))
            want = oracle.present_bgra8(final)
            for which, img8 in zip(("fused", "k_present"), got["present"]):
                assert img8.tobytes() == want.tobytes(), (T, exact, W, H, frame, which, np.argwhere(img8 != want)[:4].tolist())
            assert got["timing"]["k_present"] == (1 if T <= 63 else 2)
            c = final[..., :3]
            if W > 7 and frame == 0:
                f = c[np.isfinite(c)].astype(np.float64) * 255.0 - 0.5
                near = np.abs(f - np.round(f)) < 255.0 * 2.0 ** -24
                assert near.sum() > 1000, "colours within an ulp of (n + 0.5) / 255 reach the conversion"
                assert (c < 0).any() and (c > 1).any() and np.isnan(c).any() and len(np.unique(want)) > 200
            if W > 7 and frame == 1:
                assert np.isposinf(c).any() and np.isneginf(c).any()


# ------------------------------------------------------------------------------------------ tables of the current pose
@pytest.mark.parametrize("T", [40, 100])
@pytest.mark.parametrize("how", ["no_gbuffer", "reupload"])
def test_filter_builds_the_tables_of_the_current_scene(hip_lib, oracle, T, how):
    """rtpt_temporal_filter right after rtpt_scene_upload — no rtpt_gbuffer yet, or one for the PREVIOUS scene only: the
    normal / id-pair tables it gathers from are the current scene's (the filter builds them when stale)"""
    p = planes(oracle, T, 70, 37, "pairs_h" if T == 40 else "random", "bounded")
    for flags in (X | NOFUSE, X | DIRECT):
        got = gpu_run(hip_lib, p, flags, 3, 1, gbuffer=False, reupload=FP.soup(T, seed=1) if how == "reupload" else None)
        compare_exact(got, oracle_run(oracle, p, 0, 3, 1), ("stale tables", T, how, hex(flags)), 3)
    if how == "no_gbuffer":
        # no RTPT_PLANE_LUT_PREV either: the filter defines it as the LUT it has just built (D3, as rtpt_gbuffer does), and
        # the final pass of a frame > 0 reprojects through it
        q = dict(p, key=p["key"] + ("lut_prev is lut",), lut_prev=p["lut"])
        got = gpu_run(hip_lib, q, X | NOFUSE, 3, 1, gbuffer=False, inject_lut_prev=False)
        compare_exact(got, oracle_run(oracle, q, 0, 3, 1), ("stale tables, LUT_PREV never written", T), 3)
        assert not np.array_equal(oracle_run(oracle, q, 0, 3, 1)["prev_pixel"], oracle_run(oracle, p, 0, 3, 1)["prev_pixel"])
