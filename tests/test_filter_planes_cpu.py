"""What tests/filter_planes.py claims about its planes, checked without a GPU, and the oracle — the reference of
tests/test_filter_planes_gpu.py — against an independent float64 restatement on inputs it has never seen."""
import numpy as np
import pytest

import filter_planes as FP


def _oracle_setup(oracle, W, H, ext=0):
    cfg = oracle.config_default(W, H)
    cfg.ext_flags = ext
    pc, ubo = oracle.PushConstants(), oracle.Ubo()
    eye = np.eye(4, dtype=np.float32).ravel()
    for name in ("model", "view", "proj", "modelPrev", "viewPrev", "projPrev"):
        getattr(ubo, name)[:] = eye
    return cfg, pc, ubo


@pytest.mark.parametrize("T", FP.T_VALUES)
def test_every_generated_id_is_a_table_index(T):
    for (W, H) in FP.SHAPES:
        for kind in FP.ID_KINDS:
            ids = FP.id_plane(kind, T, W, H)
            assert ids.shape == (H, W) and ids.dtype == np.uint32 and ids.max() <= T
            assert np.array_equal(ids, FP.id_plane.__wrapped__(kind, T, W, H)), "seeded: the same plane every time"
    with pytest.raises(AssertionError):
        FP.check_ids(np.full((2, 2), T + 1, np.uint32), T)
    ids = FP.id_plane("random", T, 70, 37)
    pv = FP.prev_ids(ids, T, np.zeros((37, 70, 2), np.int32))
    assert pv.max() <= T and pv[0, 0] in ids


def test_blocks_are_4_by_5():
    ids = FP.id_plane("blocks", 40, 130, 33)
    assert all((ids[y:y + 5, x:x + 4] == ids[y, x]).all() for y in range(0, 30, 5) for x in range(0, 128, 4))
    assert len(np.unique(ids)) > 20


@pytest.mark.parametrize("T,shape", [(40, (70, 37)), (40, (130, 33)), (63, (130, 33)), (1, (7, 3))])
def test_pair_planes_read_every_table_entry(T, shape):
    """every ordered pair (p, q) of ids is (centre, neighbour) of a stride-1 tap: horizontally in pairs_h, vertically in
    pairs_v.  What an entry is worth is test_cone_soup_pair_weights_are_large_and_distinct's business."""
    W, H = shape
    assert FP.pairs_read(FP.id_plane("pairs_h", T, W, H), T, True).all()
    assert FP.pairs_read(FP.id_plane("pairs_v", T, W, H), T, False).all()
    assert not FP.pairs_read(FP.id_plane("blocks", T, W, H), T, True).all() or T == 1


@pytest.mark.parametrize("T", [40, 63])
def test_cone_soup_pair_weights_are_large_and_distinct(T):
    """reading an entry only helps if a wrong value there changes a pixel: with uniformly random normals three quarters of
    max(0, n_p . n_q)^128 are exactly 0 in binary32 and 95 % lie under 1e-6.  The scene of the pair-table tests keeps its normals
    in a cone of 4 degrees: every entry between ordinary triangles (and id 0) lies in (0.2, 1], a row holds at most one
    tie besides the almost-parallel pair (ids 6, 7), and the rows of the degenerate members and of the back face are 0."""
    tris = FP.cone_soup(T)
    v = tris.reshape(T, 3, 3)
    assert np.array_equal(v[:3], FP.soup(T).reshape(T, 3, 3)[:3]), "the degenerate members are soup()'s"
    w = FP.pair_weights_numpy(tris)
    assert w.shape == (T + 1, T + 1) and np.array_equal(w, w.T) and not np.isnan(w).any()
    ordinary = np.array([i not in FP.CONE_ODD_IDS for i in range(T + 1)])
    sub = w[np.ix_(ordinary, ordinary)]
    assert sub.min() > 0.2 and sub.max() < 1.0001
    assert w[list(FP.CONE_ODD_IDS)][:, ordinary].max() < 1e-3 and w[FP.ID_POINT].max() == 0
    assert 0.99 < w[FP.ID_TILT_A, FP.ID_TILT_B] and FP.normals_numpy(np.float64, tris)[ordinary][:, 2].min() > 0.99
    keep = np.array([i not in FP.CONE_ODD_IDS + (FP.ID_TILT_B,) for i in range(T + 1)])
    sub = w[np.ix_(keep, keep)]
    off = sub[~np.eye(len(sub), dtype=bool)].reshape(len(sub), -1)
    assert off.max() < 0.995, "no off-diagonal entry passes for a self weight"
    assert min(len(np.unique(r)) for r in off) >= off.shape[1] - 1
    upper = sub[np.triu_indices(len(sub), 1)]
    assert len(np.unique(upper)) >= 0.98 * len(upper)


@pytest.mark.parametrize("T", [40, 63, 64, 100])
def test_soup_members(oracle, T):
    """the degenerate members are what the docstring says, seen through the oracle's own normal (fma-form cross)"""
    tris = FP.soup(T)
    assert tris.shape == (T, 9)
    v = tris.reshape(T, 3, 3)
    assert np.array_equal(v[0, 1], v[0, 2]) and not np.array_equal(v[0, 0], v[0, 1])
    assert np.array_equal(v[2, 0], v[2, 1]) and np.array_equal(v[2, 0], v[2, 2])
    n64 = FP.normals_numpy(np.float64, tris)
    assert np.linalg.norm(np.cross(v[1, 1].astype(np.float64) - v[1, 0], v[1, 2].astype(np.float64) - v[1, 0])) < 1e-5
    assert np.isnan(n64[FP.ID_POINT]).all()
    assert abs(np.dot(n64[FP.ID_FRONT], n64[FP.ID_BACK]) + 1.0) < 1e-12
    ang = np.arccos(min(1.0, np.dot(n64[FP.ID_TILT_A], n64[FP.ID_TILT_B])))
    assert 5e-5 < ang < 2e-4
    lut = oracle.lut(tris, np.eye(4, dtype=np.float32).ravel())
    assert lut.shape == (T + 1, 12) and np.array_equal(lut[1:].reshape(T, 3, 4)[..., :3].reshape(T, 9), tris)


def test_two_equal_vertices_give_a_finite_residue_normal(oracle):
    """id 1 (b == c): the oracle's cross is the rounding residue of fma(a.y, b.z, -(a.z * b.y)), not 0, so the normal is a
    finite direction and the triangle weighs against itself with 0 < w <= 1 or w = 0 but never NaN; id 3 (a point) has a
    NaN normal and self weight 0 — seen as filter outputs on a 2 x 1 frame of equal colours"""
    T = 40
    tris = FP.soup(T)
    lut = oracle.lut(tris, np.eye(4, dtype=np.float32).ravel())
    cfg, pc, ubo = _oracle_setup(oracle, 2, 1)
    pc.waveletIteration, pc.maxWaveletIteration = 1, 2
    img = np.zeros((1, 2, 4), np.float32)
    img[..., :3] = 1.5
    depth = np.zeros((1, 2), np.float32)
    out = oracle.atrous(cfg, pc, ubo, img, depth, np.full((1, 2), FP.ID_TWO_EQUAL, np.uint32), lut, lut, None, None)
    assert np.isfinite(out).all() and np.allclose(out[..., :3], 1.5, rtol=1e-6)
    out = oracle.atrous(cfg, pc, ubo, img, depth, np.full((1, 2), FP.ID_POINT, np.uint32), lut, lut, None, None)
    assert np.isnan(out[..., :3]).all(), "every weight is 0: 0 / 0"


@pytest.mark.parametrize("T", [40, 100])
def test_reprojection_landing_classes(oracle, T):
    """the final-pass inputs send pixels inside the previous frame, outside it on each side, to INT_MIN / INT_MAX and —
    through 0 / 0 barycentrics of a previous triangle without area — to pixel 0 from NaN"""
    W, H = 130, 33
    ids = FP.id_plane("random", T, W, H)
    fin = FP.final_inputs(ids, T)
    cfg, pc, ubo = _oracle_setup(oracle, W, H)
    ubo.viewPrev[:] = fin["view_prev"]
    ubo.projPrev[:] = fin["proj_prev"]
    pc.waveletIteration = pc.maxWaveletIteration = 1
    pc.frameNumber = 1
    img, depth = FP.colour_depth("bounded", ids, T)
    lut = oracle.lut(FP.soup(T), np.eye(4, dtype=np.float32).ravel())
    out, pp = oracle.atrous(cfg, pc, ubo, img, depth, ids, lut, fin["lut_prev"], fin["worldpos"], fin["history"], want_prev_pixel=True)
    got = FP.landing_classes(pp, W, H)
    assert got >= {"inside", "left", "right", "above", "below", "int_min", "int_max"}, got
    for pid in (FP.ID_PREV_HUGE_POS, FP.ID_PREV_HUGE_NEG):
        assert np.isin(pp[ids == pid], (2 ** 31 - 1, -2 ** 31)).all()
    # 0 / 0: the previous triangle is a point, its area exactly 0; f2i(NaN) = 0 in both coordinates.  (The needle's area
    # is rounding residue: finite barycentrics, some pixel.)
    assert (ids == FP.ID_PREV_POINT).any() and (pp[ids == FP.ID_PREV_POINT] == 0).all()
    assert (pp[ids == 0] == np.argwhere(ids == 0)[:, ::-1]).all(), "id 0 stays where it is"
    pv = FP.prev_ids(ids, T, pp)
    inside = (pp[..., 0] >= 0) & (pp[..., 0] < W) & (pp[..., 1] >= 0) & (pp[..., 1] < H)
    same = pv[pp[..., 1][inside], pp[..., 0][inside]] == ids[inside]
    assert same.any() and not same.all()
    g = fin["gradient"][..., 0]
    assert (g == 0).any() and (g == 1).any() and (g < 0).any() and (g > 1).any() and np.isnan(g).any()
    n = fin["moments_prev"][..., 2]
    assert (n < 3).any() and (n >= 4).any() and (n < 254).any() and (n >= 255).any()


EXT_SETS = (0, 0x10, 0x20, 0x40, 0x80, 0xF0, 0x100, 0x1F0, 0x900, 0x9F0)


@pytest.mark.parametrize("ext", EXT_SETS)
def test_oracle_is_finite_on_bounded_and_not_on_planted(oracle, ext):
    """bounded planes: every pixel finite after every iteration in all ten flag sets once the ids of the all-identical-vertex
    triangle are taken out (there every weight is 0 and the pixel is 0 / 0) — so the GPU comparison within FILTER_TOL
    needs no finite mask; the NaN gradients reach the adaptive alpha only.  planted planes: NaN appears"""
    T, (W, H), N = 40, (70, 37), 3
    ids = FP.without_point(FP.id_plane("blocks", T, W, H))
    fin = FP.final_inputs(ids, T)
    lut = oracle.lut(FP.soup(T), np.eye(4, dtype=np.float32).ravel())
    cfg, pc, ubo = _oracle_setup(oracle, W, H, ext)
    ubo.viewPrev[:] = fin["view_prev"]
    ubo.projPrev[:] = fin["proj_prev"]
    pc.frameNumber = 1
    pc.maxWaveletIteration = N
    for cls in ("bounded", "planted"):
        img, depth = FP.colour_depth(cls, ids, T)
        var = None
        pv = FP.prev_ids(ids, T, np.zeros((H, W, 2), np.int32))
        if ext & 0x100:
            _, var = oracle.moments(cfg, pc, ubo, img, ids, fin["worldpos"], fin["lut_prev"], pv, fin["moments_prev"])
        cur = img
        for k in range(1, N + 1):
            pc.waveletIteration = k
            res = oracle.atrous(cfg, pc, ubo, cur, depth, ids, lut, fin["lut_prev"], fin["worldpos"], fin["history"],
                                gradient=fin["gradient"], prev_vis=pv, var_in=var)
            if var is not None:
                cur, var = res
            else:
                cur = res
        if cls == "bounded":
            expect_nan = np.isnan(fin["gradient"][..., 0]) if ext & 0x10 else np.zeros((H, W), bool)
            assert np.isfinite(cur[~expect_nan]).all(), hex(ext)
        else:
            assert np.isnan(cur).any(), hex(ext)


@pytest.mark.parametrize("stride", [1, 2, 5])
def test_oracle_against_a_float64_restatement(oracle, stride):
    """one non-final iteration on bounded planes against tests/filter_planes.py's numpy statement of the shader at float64.
    The bar is measured, not chosen: 4 x the largest distance between that statement evaluated at float32 and at float64
    (the factor of tests/golden/refshader_bars.json).  Ids of triangles without area are left out: their normals are
    rounding residue, a property of the float32 arithmetic the GPU tests compare bit for bit."""
    T, (W, H) = 40, (70, 37)
    ids = FP.id_plane("random", T, W, H).copy()
    ids[ids <= FP.ID_POINT] = 0
    tris = FP.soup(T)
    img, depth = FP.colour_depth("bounded", ids, T)
    cfg, pc, ubo = _oracle_setup(oracle, W, H)
    pc.waveletIteration, pc.maxWaveletIteration = stride, stride + 1
    lut = oracle.lut(tris, np.eye(4, dtype=np.float32).ravel())
    got = oracle.atrous(cfg, pc, ubo, img, depth, ids, lut, lut, None, None)[..., :3].astype(np.float64)
    kw = dict(sigma_n=cfg.sigma_n, sigma_z=cfg.sigma_z, sigma_l=cfg.sigma_l)
    r64 = FP.atrous_once_numpy(np.float64, img, depth, ids, FP.normals_numpy(np.float64, tris), stride, **kw)
    r32 = FP.atrous_once_numpy(np.float32, img, depth, ids, FP.normals_numpy(np.float32, tris), stride, **kw).astype(np.float64)
    bar = 4.0 * np.abs(r32 - r64).max()
    err = np.abs(got - r64).max()
    print(f"stride {stride}: oracle vs float64 {err:.3e}, bar {bar:.3e}")
    assert 0 < bar < 1e-3 and err <= bar, (err, bar)
