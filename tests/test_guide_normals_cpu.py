"""tests/guide_normals.py — the numpy restatement of RTPT_FLAG_EXT_SMOOTH_GUIDE — held to what it rests on, without a GPU: the per-pixel
form of the filter's restatement to the per-id one bit for bit, and the guide rules G1-G5 to float64, their flip on a mirrored pose and on
inverted records, and their fallback on every hostile record."""
import numpy as np
import pytest

import filter_planes as FP
import guide_normals as GN
import normal_paths as NP
import test_pathtrace_scenes_gpu as T

F32 = np.float32
W, H = GN.SHAPE
BAR = 1.0e-6        # test_normal_paths_cpu.py: the bound of rules 1 to 3 from the format; G5 only changes a sign
DOT_BAR = 4.0e-6    # ... and of a dot product of such an ns with a unit vector


# ------------------------------------------------------------------------------------------ 1. the filter's per-pixel restatement
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("stride", [1, 2, 3, 5])
def test_per_pixel_form_is_the_per_id_form(dtype, stride):
    """normals_px = normals[ids]: atrous_once_numpy's result bit for bit, degenerate triangles (NaN normals) included"""
    T_, ids = 40, FP.id_plane("random", 40, W, H)
    tris = FP.soup(T_)
    img, depth = FP.colour_depth("bounded", ids, T_)
    normals = FP.normals_numpy(dtype, tris)
    with np.errstate(all="ignore"):
        want = FP.atrous_once_numpy(dtype, img, depth, ids, normals, stride)
        got = GN.atrous_once_numpy_px(dtype, img, depth, normals[np.asarray(ids, np.int64)], stride)
    assert got.dtype == want.dtype == dtype
    FP.same_bits(got.view(np.uint32 if dtype is np.float32 else np.uint64), want.view(np.uint32 if dtype is np.float32 else np.uint64), (dtype, stride))
    assert np.isfinite(want).any()


# ------------------------------------------------------------------------------------------ 2. G1-G5 against float64
def _k0(oracle, c):
    """K0's hits of a case at the frame of the GPU tests, through the camera those use"""
    sc = c.sh.scene

    class _Abi:            # T._ubo only needs a Ubo class with the library's fields
        Ubo = oracle.Ubo
    u = T._ubo(_Abi, oracle, sc, W, H)
    return GN.k0_hits(oracle, sc.tris, np.array(u.view[:], F32), np.array(u.proj[:], F32), W, H, oracle.config_default(W, H).ray_tmax)


def _cases(oracle):
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0]).astype(F32).T.ravel()       # det < 0 on top of every instance's own pose
    yield "small", NP.small_case(oracle)
    yield "uv_sphere", NP.case(oracle, "uv_sphere")
    yield "half_cylinder", NP.case(oracle, "half_cylinder")
    yield "uv_sphere mirrored", NP.case(oracle, "uv_sphere", model=mirror)


def test_guide_rules_against_float64(oracle):
    """every hit of K0 on a smooth record whose float64 result is finite and whose G5 decision lies clear of 0: |ns32 - ns64| <= BAR and a
    unit vector on the table normal's side; at most 1 % of such hits are left out"""
    for name, (c, nrm) in _cases(oracle):
        n_base = len(nrm.tri_smooth)
        ids, b0, b1, b2 = _k0(oracle, c)
        hit = ids > 0
        hid = ids[hit].astype(np.int64) - 1
        tab = GN.normal_table(oracle, c.sh.scene.tris)
        ng = tab[hid + 1, :3]
        ns, guided = GN.guide32(oracle, nrm, n_base, hid, b0[hit], b1[hit], b2[hit], ng)
        rec = np.asarray(nrm.tri_smooth)[hid % n_base] != 0
        assert not guided[~rec].any() and FP.same_bits(ns[~guided], ng[~guided], (name, "G4")) is None
        ns64, flip, ok = GN.guide64(nrm, n_base, hid[rec], b0[hit][rec], b1[hit][rec], b2[hit][rec], ng[rec])
        assert not guided[rec][~ok].any(), (name, "a float64 NaN or zero is one in float32 too")
        clear = ok & (np.abs(flip) > DOT_BAR)
        total, left_out = int(ok.sum()), int((ok & ~clear).sum())
        assert total > 100 and left_out <= 0.01 * total, (name, total, left_out)
        assert guided[rec][clear].all(), name
        err = np.abs(ns[rec][clear].astype(np.float64) - ns64[clear]).max()
        side = (ns[rec][clear].astype(np.float64) * ng[rec][clear]).sum(1)
        print(f"{name}: hits {int(hit.sum())}, on smooth records {int(rec.sum())}, finite {total}, left out {left_out}, max |ns32 - ns64| = {err:.3e}")
        assert err <= BAR, (name, err)
        assert (side > 0).all(), (name, "G5")


def _one(oracle, n9, cof, ng, b=(0.25, 0.5, 0.25)):
    nrm = NP.Normals(np.asarray(n9, F32).reshape(1, 9), np.ones(1, np.uint32), np.asarray(cof, F32).reshape(1, 3, 3))
    b0, b1, b2 = (np.array([v], F32) for v in b)
    ns, guided = GN.guide32(oracle, nrm, 1, np.zeros(1, np.int64), b0, b1, b2, np.asarray(ng, F32).reshape(1, 3))
    return ns[0], bool(guided[0])


def test_g5_flips_mirrored_poses_and_inverted_records(oracle):
    up = np.tile([0.0, 0.6, 0.8], 3)
    ng = (0.0, 0.0, 1.0)
    eye = np.eye(3)
    ns, guided = _one(oracle, up, eye, ng)
    assert guided and np.allclose(ns, [0.0, 0.6, 0.8], atol=1e-6)
    # inverted vn: the same guide
    ns_inv, guided = _one(oracle, -up, eye, ng)
    assert guided and np.array_equal(ns_inv.view(np.uint32), ns.view(np.uint32))
    # a mirror x -> -x: L = diag(-1, 1, 1), its cofactor matrix det(L) L^-T = diag(1, -1, -1) turns the normal over, G5 turns it back
    cof = NP.cofactor(np.diag([-1.0, 1.0, 1.0]).astype(F32))
    assert np.linalg.det(np.diag([-1.0, 1.0, 1.0])) < 0 and np.array_equal(cof, np.diag([1.0, -1.0, -1.0]).astype(F32))
    ns_m, guided = _one(oracle, up, cof, ng)
    assert guided and np.allclose(ns_m, [0.0, 0.6, 0.8], atol=1e-6)
    # ... and against a table normal that faces the other way the guide follows it
    ns_b, guided = _one(oracle, up, eye, (0.0, 0.0, -1.0))
    assert guided and np.allclose(ns_b, [0.0, -0.6, -0.8], atol=1e-6)


def test_g4_falls_back_on_every_hostile_record(oracle):
    """NaN, zero, infinite and overflowing results, and a record that is not smooth: the cell keeps the table's normal, bit for bit"""
    ng = np.array([0.6, 0.0, 0.8], F32)
    eye = np.eye(3)
    up = np.tile([0.0, 0.0, 1.0], 3).astype(np.float64)
    nan = up.copy()
    nan[4] = np.nan
    huge = up * 1e20                                    # length 1e20: |w|^2 overflows binary32, the reciprocal square root is 0
    cancel = np.concatenate([[0, 0, 1], [0, 0, -1], [0, 0, 0]]).astype(np.float64)
    for name, n9, cof, b in (("nan", nan, eye, (0.25, 0.5, 0.25)), ("zero", up * 0.0, eye, (0.25, 0.5, 0.25)), ("huge", huge, eye, (0.25, 0.5, 0.25)),
                             ("inf", np.full(9, np.inf), eye, (0.25, 0.5, 0.25)), ("n0 = -n1 at b0 = b1", cancel, eye, (0.5, 0.5, 0.0)),
                             ("singular pose", up, eye * 0.0, (0.25, 0.5, 0.25))):
        with np.errstate(all="ignore"):
            ns, guided = _one(oracle, n9, cof, ng, b)
        assert not guided and np.array_equal(ns.view(np.uint32), ng.view(np.uint32)), name
    c, nrm = NP.small_case(oracle)
    flat = nrm._replace(tri_smooth=np.zeros_like(nrm.tri_smooth))
    hits = _k0(oracle, c)
    cells, mask = GN.guide_plane(oracle, c.sh.scene.tris, flat, len(flat.tri_smooth), hits)
    plain, _ = GN.guide_plane(oracle, c.sh.scene.tris, None, len(flat.tri_smooth), hits)
    assert not mask.any() and FP.same_bits(cells, plain, ("not smooth",)) is None
    # the scenes' own hostile records (normal_paths._hostile: zero, NaN, n0 = -n1, tri_smooth 0) fall back somewhere, and others do not
    cells, mask = GN.guide_plane(oracle, c.sh.scene.tris, nrm, len(nrm.tri_smooth), hits)
    ids = hits[0]
    assert mask.any() and (~mask & (ids > 0)).any()
    assert np.isfinite(cells[mask]).all()
    w = GN.self_weight(oracle, cells[mask][:, :3])
    assert np.array_equal(w.view(np.uint32), cells[mask][:, 3].view(np.uint32)) and (np.abs(w - 1.0) < 1e-4).all()
