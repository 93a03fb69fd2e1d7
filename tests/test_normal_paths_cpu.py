"""tests/normal_paths.py — the numpy restatement of smooth shading (csrc/shading_normal.hpp) — held to what it rests on, without a GPU:
the recorded frames of the walker that knew no normals where no triangle is smooth, float64 where they are, the exact sphere, float64 det(L) inv(L)^T for the cofactor
function, and the `vn` reader against the files of tests/golden/obj_normals/."""
import ctypes as C
import os

import numpy as np
import pytest

import path_walker as WK
import normal_paths as NP

F32 = np.float32
W, H = NP.SHAPE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj_normals")


def _same(a, b, tag):
    for k in ("IMAGE", "HIT_ID", "seq_n"):
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), tag + (k,)
    assert a["rays"] == b["rays"], tag + ("rays",)


# ------------------------------------------------------------------------------------------ 1. nothing smooth: the walker it extends
@pytest.mark.parametrize("name", list(NP.CASES))
@pytest.mark.parametrize("spec", [2, 4, 5])
def test_without_a_smooth_triangle_it_is_the_lattice_walker(oracle, name, spec):
    """every tri_smooth 0 (and no normals at all): the recorded lattice_paths.walk bit for bit, the mixed atlas, DEMOD off and on;
    and the two ways of having nothing smooth give each other's frame"""
    c, nrm = NP.case(oracle, name)
    s = NP.setup(oracle, c, spec)
    off = nrm._replace(tri_smooth=np.zeros_like(nrm.tri_smooth))
    tex = WK.textures(c.sh, 2)
    for demod in (False, True):
        kw = dict(rec=s["rec"], lights=s["lights"], sphere=s["sphere"], power=s["power"], tex=tex, demod=demod)
        ref = WK.recorded("normal_paths/LP" + ("/demod" if demod else ""), name, spec, demod)
        frames = []
        for n in (off, None):
            got = WK.walk(oracle, c.sh.scene, W, H, 4, normals=n, n_base=len(nrm.tri_smooth), **kw)
            _same(got, ref, (name, spec, demod, n is None))
            if demod:
                assert np.array_equal(got["ALBEDO"].view(np.uint32), ref["ALBEDO"].view(np.uint32))
            assert got["smooth"] == 0 and got["absorbed"] == 0 and got["side_invalid"] == 0 and got["offset_changed"] == 0
            frames.append(got)
        _same(frames[0], frames[1], (name, spec, demod, "tri_smooth 0 against None"))


# ------------------------------------------------------------------------------------------ 2. with normals: float64
# The float32 rounding of the rule, measured on the two scenes (4 segments, SPEC 10; hits where rule 4 fires have no ns):
# max |ns32 - ns64| per component = 1.00e-7 (uv_sphere), 1.05e-7 (half_cylinder), both unit vectors.  Bound from the format: m is
# three products and two fused adds of O(1) numbers (<= 3 ulp of its size), w three more per row (<= 3 ulp), the normalize a dot, a
# square root, a reciprocal and a product (<= 2.5 ulp): ~8 ulp of a unit vector = 8 x 2^-23 = 9.5e-7.  Records scaled by 37.5 and
# poses scaled by up to 1.25 change nothing: the normalize removes the scale.  BAR is that bound rounded up.  A dot product of
# such an ns with an exact unit vector then differs from float64's by at most sqrt(3) BAR + 2 ulp < 2e-6; DOT_BAR is twice that.
BAR = 1.0e-6          # measured: 1.05e-7
DOT_BAR = 4.0e-6      # (no decision of the two scenes lies within it of 0: 0 of 338 and 0 of 271 hits are left out)


_offset_changed = {}


def _replay64(nrm, n_base, h):
    """rules 1 to 7 in float64 from the hit records' float32 operands: ns64, the two dots rules 6 and 7 test, and rule 4's verdict"""
    t, i = (h["id"] - 1) % n_base, (h["id"] - 1) // n_base
    n9 = np.asarray(nrm.tri_normals, np.float64).reshape(-1, 3, 3)[t]
    b = np.stack([h["b0"], h["b1"], h["b2"]], 1).astype(np.float64)
    with np.errstate(all="ignore"):
        m = (b[:, :, None] * n9).sum(1)
        w = np.einsum("krc,kc->kr", np.asarray(nrm.cof, np.float64)[i], m)
        ns = w / np.linalg.norm(w, axis=1)[:, None]
        ng, d = h["ng"].astype(np.float64), h["d"].astype(np.float64)
        flip = (ns * ng).sum(1)
        ns6 = np.where((flip < 0)[:, None], -ns, ns)
        facing = (ns6 * d).sum(1)
        ns7 = np.where((facing < 0)[:, None], ns6, ng)
    return ns7, flip, facing, np.isfinite(ns).all(1)


@pytest.mark.parametrize("name", list(NP.CASES))
def test_with_normals_it_matches_float64(oracle, name):
    """SPEC 10, 4 segments: at every hit on a smooth record whose float64 decisions lie clear of 0, the walker's ns is float64's
    within BAR, its absorption is float64's, and at most 1 % of such hits are left out"""
    c, nrm = NP.case(oracle, name)
    s = NP.setup(oracle, c, 10)
    hits = []
    r = WK.walk(oracle, c.sh.scene, W, H, 4, normals=nrm, hits=hits, **s)
    h = WK.hit_table(hits)
    h = {k: v[h["bounced"]] for k, v in h.items()}      # a hit on a path's last segment has no bounce to judge
    n_base = len(nrm.tri_smooth)
    rec_smooth = np.asarray(nrm.tri_smooth)[(h["id"] - 1) % n_base] != 0
    ns64, flip, facing, ok4 = _replay64(nrm, n_base, {k: v[rec_smooth] for k, v in h.items()})
    got_smooth = h["smooth"][rec_smooth]
    # rule 4 itself: a float64 w that is exactly 0 or NaN is one in float32 too (zero and NaN corners, n0 = -n1 on the edge)
    assert not got_smooth[~ok4].any(), name
    dn = h["dn"][rec_smooth].astype(np.float64)
    ng = h["ng"][rec_smooth].astype(np.float64)
    side = (dn * ng).sum(1)
    bounce = ~h["glass"][rec_smooth]
    clear = ok4 & (np.abs(flip) > DOT_BAR) & (np.abs(facing) > DOT_BAR) & (~bounce | (np.abs(side) > DOT_BAR))
    left_out = int((ok4 & ~clear).sum())
    total = int(ok4.sum())
    print(f"{name}: hits {len(rec_smooth)}, on smooth records {int(rec_smooth.sum())}, finite {total}, left out {left_out}")
    assert total > 200 and left_out <= 0.01 * total, (name, total, left_out)
    assert got_smooth[clear].all(), name
    err = np.abs(h["ns"][rec_smooth][clear].astype(np.float64) - ns64[clear]).max()
    print(f"{name}: max |ns32 - ns64| = {err:.3e} (bar {BAR:.1e})")
    assert err <= BAR, (name, err)
    # the side test on d', where the walker's own d' decides it: absorbed exactly where float64's dot is not positive
    sel = clear & bounce & ~h["mirror"][rec_smooth]
    assert np.array_equal(h["gone"][rec_smooth][sel], ~(side[sel] > 0)), name
    # side rule 3: a dielectric's offset has the sign of float64's dot(d', ng), whatever `transmitted` said
    glass = clear & h["glass"][rec_smooth] & (np.abs(side) > DOT_BAR)
    assert glass.sum() > 20, (name, int(glass.sum()))
    assert np.array_equal(h["off"][rec_smooth][glass] < 0, side[glass] < 0), name
    _offset_changed[name] = r["offset_changed"]
    # what the scenes must show, by the walker alone
    for k in ("smooth", "fallback4", "fallback7", "absorbed", "transmitted", "reflected", "lit", "sphere_valid"):
        assert r[k] > 0, (name, k, {q: r[q] for q in WK.COUNTS if q in r})


def test_the_offset_rule_decides_somewhere(oracle):
    """on at least one scene side rule 3 chooses another sign than the `transmitted` flag would have (walker's count, 4 segments)"""
    for name in NP.CASES:
        if name not in _offset_changed:
            c, nrm = NP.case(oracle, name)
            _offset_changed[name] = WK.walk(oracle, c.sh.scene, W, H, 4, normals=nrm, **NP.setup(oracle, c, 10))["offset_changed"]
    assert max(_offset_changed.values()) > 0, _offset_changed


def test_ns_is_nearer_the_sphere_than_ng(oracle):
    """uv_sphere(16, 24) with its exact vertex normals under the identity: at seeded hits (barycentrics inside every triangle) ns is
    closer to normalize(pos - centre) than ng is, wherever the hit does not fall back"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.scenes import uv_sphere
    centre = np.array([0.3, -0.2, 0.1])
    xyz, idx, n9 = uv_sphere(16, 24, 0.75, centre)
    tris = xyz[idx].reshape(-1, 3, 3)
    rng = np.random.default_rng(11)
    t = rng.integers(0, len(tris), 4000)
    b = rng.dirichlet([1.0, 1.0, 1.0], len(t)).astype(F32)
    b1, b2 = b[:, 1].copy(), b[:, 2].copy()
    b0 = ((F32(1.0) - b1).astype(F32) - b2).astype(F32)
    pos = (b0[:, None] * tris[t, 0] + b1[:, None] * tris[t, 1] + b2[:, None] * tris[t, 2]).astype(np.float64)
    true = (pos - centre) / np.linalg.norm(pos - centre, axis=1)[:, None]
    ng = np.cross(tris[t, 1] - tris[t, 0], tris[t, 2] - tris[t, 0]).astype(np.float64)
    ng = (ng / np.linalg.norm(ng, axis=1)[:, None]).astype(F32)
    d = (-true + 0.3 * rng.standard_normal(true.shape))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32)
    nrm = NP.Normals(n9, np.ones(len(tris), np.uint32), NP.cof_table(oracle))
    ns, smooth = NP.hit_shading_normal(oracle, nrm, t.astype(np.int64), len(tris), b0, b1, b2, ng, d)
    kept = smooth & ~(ns == ng).all(1)              # not a fallback of rule 4 or rule 7
    assert kept.sum() > 3500
    e_ns = np.linalg.norm(ns[kept].astype(np.float64) - true[kept], axis=1)
    e_ng = np.linalg.norm(ng[kept].astype(np.float64) - true[kept], axis=1)
    assert (e_ns < e_ng).all(), float((e_ns - e_ng).max())


# ------------------------------------------------------------------------------------------ 3. the cofactor function
def _hostile_matrices():
    rng = np.random.default_rng(3)
    ms = [np.eye(3), np.diag([-1.0, 1.0, 1.0]), np.diag([2.0, 0.5, 3.0]), np.diag([1e-6, 1e6, 1.0]), np.diag([1e15, 1e15, 1e-15]),
          np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 10.0]]), np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])]
    ms += [rng.standard_normal((3, 3)) * 10.0 ** rng.integers(-3, 4) for _ in range(64)]
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    ms += [q, q @ np.diag([1.0, 1.0, -1.0]), q @ np.diag([3.0, 0.25, 1.5])]
    return np.array(ms).astype(F32)


def test_cofactor_against_float64(oracle):
    """cofactor(L) = det(L) inv(L)^T in float64 of the same float32 entries: each entry is two products and a difference, so it is
    within 1.5 ulp of the larger product (2^-23 x 1.5 = 1.8e-7, relative to |p q| + |s t|); and it carries normals: (C n) . (L t)
    = det(L) (n . t) for every n, t.  Singular and mirrored matrices included"""
    ls = _hostile_matrices()
    c = NP.cofactor(ls).astype(np.float64).reshape(-1, 9)
    l64 = ls.astype(np.float64)
    a = l64.reshape(-1, 9)
    terms = [(4, 8, 5, 7), (5, 6, 3, 8), (3, 7, 4, 6), (2, 7, 1, 8), (0, 8, 2, 6), (1, 6, 0, 7), (1, 5, 2, 4), (2, 3, 0, 5), (0, 4, 1, 3)]
    size = np.stack([np.abs(a[:, p] * a[:, q]) + np.abs(a[:, s] * a[:, t]) for p, q, s, t in terms], 1)
    minors = np.stack([a[:, p] * a[:, q] - a[:, s] * a[:, t] for p, q, s, t in terms], 1)
    # fl(fl(p q) - fl(s t)): half an ulp per product and half an ulp of the difference, at most 2^-23 (|p q| + |s t|)
    assert (np.abs(c - minors) <= 1.2e-7 * size).all()
    well = np.array([np.linalg.cond(m) < 1e6 for m in l64])
    assert well.sum() > 40
    want = np.stack([np.linalg.det(m) * np.linalg.inv(m).T for m in l64[well]]).reshape(-1, 9)
    assert (np.abs(c[well] - want) <= 1.2e-7 * size[well] + 1e-9 * (np.abs(l64[well]).max((1, 2)) ** 2)[:, None]).all()
    # a singular matrix and the identity, exactly
    assert np.array_equal(NP.cofactor(np.zeros((3, 3), F32)), np.zeros((3, 3), F32))
    assert np.array_equal(NP.cofactor(np.eye(3, dtype=F32)), np.eye(3, dtype=F32))
    mirror = NP.cofactor(np.diag(F32([-1, 1, 1])))
    assert np.array_equal(mirror, np.diag(F32([1, -1, -1])))          # det < 0 turns the normal over: rule 6 turns it back
    # linear_part: model x transform as one matrix, and the table of a scene without transforms
    xf = NP.xforms()
    tab = NP.cof_table(oracle, None, xf)
    assert np.array_equal(tab, np.stack([NP.cofactor(x[:, :3].astype(F32)) for x in xf]))
    assert np.array_equal(NP.cof_table(oracle), np.eye(3, dtype=F32)[None])


# ------------------------------------------------------------------------------------------ 4. the loader
def test_loader_against_the_golden_folder():
    """every file of tests/golden/obj_normals/ against its expected arrays (expected.npz: <stem>_normals, <stem>_smooth): `v//vn`
    and `v/vt/vn` corners, negative indices, fans, a face with a corner without vn, indices that are 0 or out of range"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi
    if not os.path.exists(abi.LIB_PATH):
        pytest.fail("librtpt_hip.so is not built: the loader under test lives in it")
    want = np.load(os.path.join(GOLDEN, "expected.npz"))
    stems = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".obj"))
    assert len(stems) >= 5
    for stem in stems:
        nrm, smooth = abi.load_obj_normals(os.path.join(GOLDEN, stem + ".obj"))
        assert np.array_equal(smooth, want[stem + "_smooth"]), stem
        assert np.array_equal(nrm.view(np.uint32), want[stem + "_normals"].view(np.uint32)), stem
        _, idx = abi.load_obj(os.path.join(GOLDEN, stem + ".obj"))
        assert len(idx) == len(smooth), stem      # the arrays line up with rtpt_util_load_obj's triangles


def test_make_app_refuses_smooth_normals_with_a_mesh_before_it_creates_anything():
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    with pytest.raises(ValueError, match="smooth_normals"):
        make_app(-1, -1, mesh=(np.zeros((3, 3), F32), np.zeros((1, 3), np.uint32)), smooth_normals=True)   # no context was asked for
