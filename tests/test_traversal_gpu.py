"""Closest hit on adversarial geometry: the device traversal (brute force, BVH over triangles, BVH over fan pairs, a stack
that spills) against the oracle's brute force, bit for bit.

D4 (closest_hit.hpp, bvh.hpp): the winner is the minimum over (t, id) of ONE ray-triangle routine, so no structure that
enumerates the candidates may change it.  The other GPU tests of that rule all use axis-aligned box walls near the
origin; the scenes here are soups in every orientation, degenerate and flat triangles, coordinates far from the origin,
scales whose triple products go subnormal or overflow, slivers, duplicates at other ids, and non-planar fan pairs.  The
rays aim at vertices, edges and shared edges, lie in planes, start on surfaces, run along axes, carry -0 / tiny /
subnormal direction components, and start up to 5 000 scene diagonals away.

Every case counts what it exercised against a floor, so a generator that drifts into missing everything fails.
Every tree here was just built for its geometry; test_refit_moves_gpu.py holds a tree that was REFIT to a hostile pose to D4.
RTPT_TRAVERSAL_SEEDS=k runs every case under k seeds instead of one."""
import os

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

SEEDS = range(int(os.environ.get("RTPT_TRAVERSAL_SEEDS", "1")))
F32 = np.float32


# ------------------------------------------------------------------------------ scenes (xyz, idx): seeded, float32
def _soup(rng, n, lo=-0.4, hi=0.4, size=0.06):
    """n triangles, centres uniform in a cube, vertices scattered around them in every orientation"""
    c = rng.uniform(lo, hi, (n, 1, 3))
    v = (c + rng.normal(0, size, (n, 3, 3))).astype(F32)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def _join(*meshes):
    xyz, idx, base = [], [], 0
    for v, i in meshes:
        xyz.append(v)
        idx.append(i + base)
        base += len(v)
    return np.concatenate(xyz).astype(F32), np.concatenate(idx).astype(np.uint32)


def _degenerate(rng, n):
    """zero-area (two equal vertices), collinear and point triangles"""
    p = rng.uniform(-0.4, 0.4, (n, 3)).astype(F32)
    q = (p + rng.normal(0, 0.08, (n, 3))).astype(F32)
    v = np.empty((n, 3, 3), F32)
    kind = np.arange(n) % 3
    v[kind == 0] = np.stack([p, q, q], 1)[kind == 0]                                    # two equal vertices
    v[kind == 1] = np.stack([p, q, (0.5 * (p + q)).astype(F32)], 1)[kind == 1]          # collinear
    v[kind == 2] = np.stack([p, p, p], 1)[kind == 2]                                    # a point
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def _slivers(rng, n):
    """long thin triangles that cross the scene"""
    a = rng.uniform(-0.45, 0.45, (n, 3))
    b = -a + rng.normal(0, 0.05, (n, 3))
    c = a + (b - a) * rng.uniform(0.2, 0.8, (n, 1)) + rng.normal(0, 2e-3, (n, 3))
    v = np.stack([a, b, c], 1).astype(F32)
    return v.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def _heightfield(g=24, odd=False):
    """(g x g) quads over a non-planar height function, each the fan pair (a, b, c), (a, c, d)"""
    x, z = np.meshgrid(np.linspace(-0.5, 0.5, g + 1), np.linspace(-0.5, 0.5, g + 1), indexing="ij")
    y = 0.15 * np.sin(7.0 * x) * np.cos(5.0 * z) + 0.4 * x * z
    xyz = np.stack([x, y, z], -1).reshape(-1, 3).astype(F32)
    i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
    a = (i * (g + 1) + j).ravel()
    b, c, d = a + (g + 1), a + (g + 2), a + 1
    idx = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)
    if odd:  # one more (unpaired) triangle: the scene is no longer all fan pairs, the pair path is off
        idx = np.concatenate([idx, [[0, g + 1, 1]]])
    return xyz, idx.astype(np.uint32)


def _sphere(nu=32, nv=16, r=0.45):
    """a UV sphere, every band quad a fan pair (the pole quads carry one zero-area half)"""
    th = np.linspace(0, np.pi, nv + 1)
    ph = np.linspace(0, 2 * np.pi, nu + 1)
    t, p = np.meshgrid(th, ph, indexing="ij")
    xyz = (r * np.stack([np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)], -1)).reshape(-1, 3).astype(F32)
    i, j = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    a = (i * (nu + 1) + j).ravel()
    b, c, d = a + (nu + 1), a + (nu + 2), a + 1
    idx = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)
    return xyz, idx.astype(np.uint32)


def _flat(rng, n):
    xyz, idx = _soup(rng, n, size=0.08)
    xyz[:, 1] = F32(0.25)  # zero extent on y
    return xyz, idx


def _duplicates(rng):
    """a soup, exact copies of some of its triangles at higher ids (three copies each: a leaf holds two at most, so at
    least two of them land in different leaves), and coplanar triangles overlapping others"""
    xyz, idx = _soup(rng, 400)
    tri = xyz[idx]                                            # (n, 3, 3)
    dup = rng.choice(400, 60, replace=False)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cop = rng.choice(400, 60, replace=False)
    s = rng.uniform(0.1, 0.3, (60, 2)).astype(F32)
    shift = (s[:, :1] * e1[cop] + s[:, 1:] * e2[cop]).astype(F32)
    coplanar = (tri[cop] + shift[:, None, :]).astype(F32)     # a translate within the plane (up to rounding)
    allt = np.concatenate([tri, tri[dup], coplanar, tri[dup]])
    perm = np.concatenate([np.arange(400), 400 + rng.permutation(len(allt) - 400)])
    allt = allt[perm]
    return allt.reshape(-1, 3), np.arange(3 * len(allt), dtype=np.uint32).reshape(-1, 3)


def _pair_ok(tris):
    """rtpt_scene_upload's test: every (2q, 2q+1) is a fan pair (a, b, c), (a, c, d), bitwise"""
    if len(tris) < 2 or len(tris) % 2:
        return False
    t = tris.reshape(-1, 2, 9).view(np.uint32)
    return bool((t[:, 0, 0:3] == t[:, 1, 0:3]).all() and (t[:, 0, 6:9] == t[:, 1, 3:6]).all())


# ------------------------------------------------------------------------------ rays: (n, 6) float32
def _unit(d):
    d = np.asarray(d, np.float64)
    n = np.linalg.norm(d, axis=1, keepdims=True)
    d = np.where(n > 0, d, [0.0, 0.0, 1.0])  # an origin on its target (a point triangle): any direction
    return (d / np.where(n > 0, n, 1.0)).astype(F32)


def _bounds(tris):
    v = tris.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    return lo, hi, float(np.linalg.norm(hi - lo))


def _targets(tris, rng, n):
    """vertices, edge midpoints and (for fan pairs) points on the shared edge a-c"""
    t = tris.reshape(-1, 3, 3)
    k = rng.integers(0, len(t), n)
    kind = rng.integers(0, 3, n)
    vtx = t[k, rng.integers(0, 3, n)]
    e = rng.integers(0, 3, n)
    mid = (F32(0.5) * (t[k, e] + t[k, (e + 1) % 3])).astype(F32)
    w = rng.uniform(0.05, 0.95, (n, 1)).astype(F32)
    shared = (t[k, 0] + w * (t[k, 2] - t[k, 0])).astype(F32)  # edge v0-v2: the shared edge of a fan pair
    return np.where(kind[:, None] == 0, vtx, np.where(kind[:, None] == 1, mid, shared)).astype(F32), k


def _aim(o, target):
    """direction = target - origin in binary32, then normalised"""
    return np.concatenate([o, _unit((target - o).astype(F32))], 1).astype(F32)


def ray_families(tris, rng, n=2000, in_plane=False):
    lo, hi, diag = _bounds(tris)
    c, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3)
    box = lambda m: rng.uniform(c - 0.75 * ext, c + 0.75 * ext, (m, 3)).astype(F32)
    fam = {}
    fam["random"] = np.concatenate([box(n), _unit(rng.normal(size=(n, 3)))], 1).astype(F32)
    tgt, _ = _targets(tris, rng, n)
    fam["aimed"] = _aim(box(n), tgt)
    # lying in a triangle's plane: from a point of the plane outside the triangle towards one inside or on its edge.  Only
    # where asked: in a tilted plane d.n and (o - v0).n are rounding noise, and so is the routine's t (test_known_gaps)
    t = tris.reshape(-1, 3, 3)
    k = rng.integers(0, len(t), n)
    e1, e2 = t[k, 1] - t[k, 0], t[k, 2] - t[k, 0]
    a = rng.uniform(-1.5, 2.5, (n, 2)).astype(F32)
    o = (t[k, 0] + a[:, :1] * e1 + a[:, 1:] * e2).astype(F32)
    b = rng.uniform(0, 0.5, (n, 2)).astype(F32)
    if in_plane:
        fam["in_plane"] = _aim(o, (t[k, 0] + b[:, :1] * e1 + b[:, 1:] * e2).astype(F32))
    # starting on a triangle's surface
    b = rng.uniform(0, 0.5, (n, 2)).astype(F32)
    o = (t[k, 0] + b[:, :1] * e1 + b[:, 1:] * e2).astype(F32)
    fam["on_surface"] = np.concatenate([o, _unit(rng.normal(size=(n, 3)))], 1).astype(F32)
    # axis-parallel, and components on both sides of the traversal's 1e-20 clamp: -0, 1e-25, subnormal, 1e-20, 3e-20
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(F32)
    tgt, _ = _targets(tris, rng, n)
    o = box(n)
    d = axes[rng.integers(0, 6, n)]
    ax = np.argmax(np.abs(d), 1)
    o2 = tgt.copy()  # the origin's other two coordinates are the target's: the ray runs along an axis through it
    o2[np.arange(n), ax] = o[np.arange(n), ax]
    fam["axis"] = np.concatenate([o2, d], 1).astype(F32)
    tiny = np.array([-0.0, 0.0, 1e-25, -1e-25, 1e-40, -1e-40, 1e-20, -1e-20, 3e-20, -3e-20], F32)
    r = _aim(box(n), tgt)
    for j in range(n):
        comps = rng.choice(3, rng.integers(1, 3), replace=False)
        r[j, 3 + comps] = tiny[rng.integers(0, len(tiny), len(comps))]
    fam["tiny_components"] = r
    return fam


def distant_rays(tris, rng, dist_diags, n=3000):
    """vertex-aimed rays from `dist_diags` scene diagonals away; also returns the target triangle and vertex"""
    lo, hi, diag = _bounds(tris)
    t = tris.reshape(-1, 3, 3)
    k = rng.integers(0, len(t), n)
    vi = rng.integers(0, 3, n)
    tgt = t[k, vi]
    u = _unit(rng.normal(size=(n, 3))).astype(np.float64)
    o = (tgt.astype(np.float64) - u * dist_diags * diag).astype(F32)
    return _aim(o, tgt), k, vi


def corner_vertex(tris, k, vi):
    """the vertex is extreme (min or max) on at least two axes of its triangle's box: the box of a one-triangle leaf, a
    ray through it grazes that box along an edge of two faces"""
    t = tris.reshape(-1, 3, 3)[k]
    v = t[np.arange(len(k)), vi]
    ext = (v == t.min(1)) | (v == t.max(1))
    return ext.sum(1) >= 2


# ------------------------------------------------------------------------------ the comparison
def _forms(n_tris, paired):
    forms = [("default", 0, {})]
    if n_tris <= 64:
        forms.append(("force_bvh", 2, {}))
    if paired:
        forms.append(("no_pairs", 0, {"RTPT_NO_TRI_PAIRS": "1"}))
    forms.append(("stack_lds_1", 2 if n_tris <= 64 else 0, {"RTPT_BVH_STACK_LDS": "1"}))
    return forms


def _first_mismatch(tag, rays, ids, ts, wid, wts):
    bad = np.nonzero((ids != wid) | (bits(ts) != bits(wts)))[0]
    if not len(bad):
        return None
    j = bad[0]
    return (f"{tag}: {len(bad)} of {len(rays)} rays differ; first #{j}: o={rays[j, :3].tolist()} d={rays[j, 3:].tolist()} "
            f"gpu id={int(ids[j])} t={float(ts[j])!r} ({int(bits(ts)[j]):#010x}), "
            f"oracle id={int(wid[j])} t={float(wts[j])!r} ({int(bits(wts)[j]):#010x})")


def check_case(hip_lib, oracle, monkeypatch, tag, xyz, idx, rays_by_family, xf=None, tmax=None, floors=None):
    """upload (xyz, idx[, instances]) under every traversal form that applies, trace every family, compare with the
    oracle bit for bit; returns the oracle's (ids, t) per family"""
    tris = oracle.flatten(xyz, idx, xf)
    n = len(tris)
    rays = np.concatenate(list(rays_by_family.values()))
    cfg = hip_lib.config_default(64, 64)
    if tmax is not None:
        cfg.ray_tmax = tmax
    wid, wts = oracle.trace_rays(tris, rays, tmax=cfg.ray_tmax)
    errors = []
    for name, flags, env in _forms(n, _pair_ok(tris)):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            c = hip_lib.config_default(64, 64)
            c.ray_tmax = cfg.ray_tmax
            c.flags = flags
            with hip_lib.Context(c) as ctx:
                ctx.scene_upload(xyz, idx, xf)
                ids, ts = ctx.selftest_trace(rays)
        msg = _first_mismatch(f"{tag} [{name}]", rays, ids, ts, wid, wts)
        if msg:
            errors.append(msg)
    assert not errors, "\n".join(errors)
    out, at = {}, 0
    for fam, r in rays_by_family.items():
        out[fam] = (wid[at:at + len(r)], wts[at:at + len(r)])
        at += len(r)
    for fam, floor in (floors or {}).items():
        hits = int((out[fam][0] > 0).sum())
        assert hits >= floor, f"{tag}: family {fam} hit only {hits} times (floor {floor}): the case no longer exercises it"
    return out


def _default_floors(fams, frac=0.05):
    return {f: int(frac * len(r)) for f, r in fams.items()}


# ------------------------------------------------------------------------------ cases
SCENES = {
    "soup": lambda rng: _soup(rng, 5000),
    "degenerate_mix": lambda rng: _join(_soup(rng, 1500), _degenerate(rng, 900)),
    "flat": lambda rng: _flat(rng, 1500),
    "far_1e5": lambda rng: (lambda v, i: ((v + F32(1.0e5)).astype(F32), i))(*_soup(rng, 2000)),
    "slivers": lambda rng: _join(_slivers(rng, 300), _soup(rng, 1500, size=0.02)),
    "heightfield": lambda rng: _heightfield(24),
    "heightfield_odd": lambda rng: _heightfield(24, odd=True),
    "sphere": lambda rng: _sphere(),
}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("scene", list(SCENES))
def test_scene_families(hip_lib, oracle, monkeypatch, scene, seed):
    rng = np.random.default_rng([101, seed, list(SCENES).index(scene)])
    xyz, idx = SCENES[scene](rng)
    tris = oracle.flatten(xyz, idx)
    if scene in ("heightfield", "sphere"):
        assert _pair_ok(tris), "the mesh must take the fan-pair path"
    if scene == "heightfield_odd":
        assert not _pair_ok(tris)
    # the flat scene's plane is y = const: a ray in it has d.y == 0 exactly, d.n == 0, and the routine rejects it exactly
    fams = ray_families(tris, rng, in_plane=scene == "flat")
    if scene.startswith("heightfield"):  # axis-parallel rays through its edge points: an open gap (test_known_gaps)
        del fams["axis"]
    floors = _default_floors(fams)
    if scene == "flat":  # every triangle is in the one plane: rays in it or starting on it meet none
        floors["in_plane"] = floors["on_surface"] = 0
    floors["tiny_components"] = len(fams["tiny_components"]) // 100
    if "axis" in fams:
        floors["axis"] = len(fams["axis"]) // 100
    check_case(hip_lib, oracle, monkeypatch, f"{scene}/seed{seed}", xyz, idx, fams, floors=floors)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 66])
def test_counts_around_the_brute_force_switch(hip_lib, oracle, monkeypatch, n):
    """1..3 triangles: the single-leaf root {leaf, absent}; 64 / 65 / 66: both sides of the brute-force / BVH switch"""
    rng = np.random.default_rng([202, n])
    xyz, idx = _soup(rng, n, size=0.15)
    tris = oracle.flatten(xyz, idx)
    fams = ray_families(tris, rng, n=1500)
    check_case(hip_lib, oracle, monkeypatch, f"n={n}", xyz, idx, fams,
               floors={"aimed": 150, "random": 1 if n < 64 else 30, "on_surface": 10})
    # the same counts as fan pairs (a heightfield strip): the pair path on the smallest trees
    if n % 2 == 0:
        hx, hi = _heightfield(8)
        hx, hi = hx, hi[:n]
        ht = oracle.flatten(hx, hi)
        assert _pair_ok(ht)
        check_case(hip_lib, oracle, monkeypatch, f"pairs n={n}", hx, hi, ray_families(ht, rng, n=1500), floors={"aimed": 150})


@pytest.mark.parametrize("scale", [1e-13, 1e13])
def test_scale_extremes(hip_lib, oracle, monkeypatch, scale):
    """the soup and its rays scaled together (directions not renormalised: t, in units of |d|, stays the same size):
    at 1e-13 the triple products tv.n and e.(tv x d) are subnormal, at 1e13 some overflow to inf — flush-to-zero or a
    contracted multiply-add on either side would change bits"""
    rng = np.random.default_rng([303, 100 + int(np.log10(scale))])
    xyz, idx = _soup(rng, 2000)
    fams = ray_families(oracle.flatten(xyz, idx), rng)
    s = F32(scale)
    xyz = (xyz * s).astype(F32)
    fams = {k: (r * s).astype(F32) for k, r in fams.items()}
    out = check_case(hip_lib, oracle, monkeypatch, f"scale {scale:g}", xyz, idx, fams,
                     floors={"aimed": 200, "random": 50})
    tris = oracle.flatten(xyz, idx).astype(np.float64)
    n = np.cross(tris[:, 3:6] - tris[:, :3], tris[:, 6:9] - tris[:, :3])
    mag = np.abs(n).max(1) * float(scale)          # |tv . n| for |tv| ~ scale
    if scale < 1:
        assert (mag < np.finfo(F32).tiny).mean() > 0.5, "the triple products should be subnormal at this scale"
    else:
        assert (mag > 1e36).mean() > 0.1, "some triple products should be near or past binary32 overflow at this scale"


def test_duplicates_and_coplanar_overlaps(hip_lib, oracle, monkeypatch):
    """exact copies at higher ids and coplanar overlaps: equal t, the lower id must win whichever leaf is met first
    (the inclusive `tl <= min(tf, h.t)` cull and TIE_BREAK in the leaves)"""
    rng = np.random.default_rng(404)
    xyz, idx = _duplicates(rng)
    tris = oracle.flatten(xyz, idx)
    t = tris.reshape(-1, 3, 3)
    # rays at the centroids (and other interior points) of triangles that have copies
    key = {}
    for i, row in enumerate(tris.view(np.uint32)):
        key.setdefault(row.tobytes(), []).append(i)
    dup_groups = [g for g in key.values() if len(g) > 1]
    assert len(dup_groups) >= 50
    first = np.array([g[0] for g in dup_groups])
    k = rng.choice(first, 3000)
    b = rng.dirichlet([2, 2, 2], 3000).astype(F32)
    tgt = (b[:, :1] * t[k, 0] + b[:, 1:2] * t[k, 1] + b[:, 2:] * t[k, 2]).astype(F32)
    lo, hi, _ = _bounds(tris)
    o = rng.uniform(lo - 0.5, hi + 0.5, (3000, 3)).astype(F32)
    fams = ray_families(tris, rng)
    fams["dup_aimed"] = _aim(o, tgt)
    out = check_case(hip_lib, oracle, monkeypatch, "duplicates", xyz, idx, fams, floors={"aimed": 200, "dup_aimed": 300})
    # rays whose winner has an exact copy at a higher id: the tie was decided for the lower one
    wid = out["dup_aimed"][0].astype(np.int64) - 1
    low = set(first.tolist())
    ties = sum(1 for w in wid if w in low)
    assert ties >= 300, f"only {ties} rays ended on a duplicated triangle"
    assert not any(w >= 0 and any(w in g[1:] for g in dup_groups) for w in wid[:200]), "a higher copy won a tie"
    # two identity instances: every triangle twice, ids n_tris apart
    xyz2, idx2 = _soup(rng, 1500)
    eye = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F32), (2, 1))
    t2 = oracle.flatten(xyz2, idx2, eye)
    f2 = ray_families(t2[:1500], rng)
    out2 = check_case(hip_lib, oracle, monkeypatch, "two identity instances", xyz2, idx2, f2, xf=eye,
                      floors={"aimed": 200, "random": 50})
    w = np.concatenate([v[0] for v in out2.values()])
    assert (w > 0).sum() >= 500 and (w <= 1500).all(), "the first instance's copy (lower id) wins every tie"


@pytest.mark.parametrize("dist", [10, 100, 1000, 5000])
def test_distant_origins(hip_lib, oracle, monkeypatch, dist):
    """vertex-aimed rays from far away: the slab distances round (origin - o) / d, an error that grows with the distance
    while the boxes' padding does not; a ray that reaches a vertex at the corner of two faces of its leaf box must not
    have that box culled"""
    cases = [("soup", _soup(np.random.default_rng([505, dist]), 3000, lo=-0.3, hi=0.3)), ("heightfield", _heightfield(24)),
             ("sphere", _sphere())]
    corners = 0
    for name, (xyz, idx) in cases:
        rng = np.random.default_rng([506, dist, len(name)])
        tris = oracle.flatten(xyz, idx)
        _, _, diag = _bounds(tris)
        assert dist * diag < 0.95 * 10000.0, "the farthest origin must stay inside ray_tmax"
        rays, k, vi = distant_rays(tris, rng, dist)
        out = check_case(hip_lib, oracle, monkeypatch, f"{name} from {dist} diagonals", xyz, idx, {"distant": rays},
                         floors={"distant": 300})
        wid = out["distant"][0].astype(np.int64) - 1
        corner = int((corner_vertex(tris, k, vi) & (wid == k)).sum())
        assert corner >= 10, f"{name} from {dist} diagonals: only {corner} hits on box-corner vertices"
        corners += corner
    assert corners >= 300, f"from {dist} diagonals: only {corners} hits on box-corner vertices"


@pytest.mark.xfail(strict=True, reason="open D4 gaps, present before this file existed (DESIGN.md 4, K2/K0): rays in a tilted "
                   "triangle's plane, and axis-parallel rays through the heightfield's edge points")
def test_known_gaps(hip_lib, oracle, monkeypatch):
    """Where the BVH and the brute force still disagree (found by this file, 1-4 rays of 2 000 per case, in every BVH form):
    - a ray in the plane of a tilted triangle: d.n and (o - v0).n are rounding noise, the routine can accept the ray with
      a t anywhere near the triangle, and a box whose interval does not hold that t is culled — no box margin bounds it;
    - an axis-parallel ray through a vertex / edge point of the non-planar heightfield: the BVH misses a nearer hit that the
      brute force reports; the cause is not established.
    Strict: when both gaps are closed this passes, and the marker must go."""
    errors = []
    for name, (xyz, idx) in (("soup", _soup(np.random.default_rng([101, 0, 0]), 5000)), ("heightfield", _heightfield(24))):
        rng = np.random.default_rng([101, 0, list(SCENES).index(name)])
        fams = ray_families(oracle.flatten(xyz, idx), rng, in_plane=True)
        keep = {"in_plane": fams["in_plane"]}
        if name == "heightfield":
            keep["axis"] = fams["axis"]
        try:
            check_case(hip_lib, oracle, monkeypatch, f"{name} known gaps", xyz, idx, keep, floors={"in_plane": 300})
        except AssertionError as e:
            errors.append(str(e).splitlines()[0])
    assert not errors, "\n".join(errors)


def test_small_ray_tmax(hip_lib, oracle, monkeypatch):
    """ray_tmax = 3: hits just past tmax are dropped the same way by the boxes and by the triangles"""
    rng = np.random.default_rng(606)
    xyz, idx = _soup(rng, 3000, lo=-2.0, hi=2.0, size=0.1)
    tris = oracle.flatten(xyz, idx)
    fams = ray_families(tris, rng)
    # origins 2.5..3.5 away from vertex targets: the hit sits on either side of tmax
    tgt, _ = _targets(tris, rng, 3000)
    u = _unit(rng.normal(size=(3000, 3))).astype(np.float64)
    o = (tgt - u * rng.uniform(2.5, 3.5, (3000, 1))).astype(F32)
    fams["around_tmax"] = _aim(o, tgt)
    out = check_case(hip_lib, oracle, monkeypatch, "ray_tmax=3", xyz, idx, fams, tmax=3.0, floors={"around_tmax": 300})
    wts = out["around_tmax"][1]
    assert (wts[out["around_tmax"][0] > 0] < 3.0).all()


# ------------------------------------------------------------------------------ whole frames, posed by ubo.model
def _rot(ax, ay, t):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    m = np.eye(4)
    m[:3, :3] = ry @ rx
    m[:3, 3] = t
    return np.ascontiguousarray(m.astype(F32).T).ravel()  # column-major


@pytest.mark.parametrize("scene", ["heightfield", "soup"])
def test_posed_frames_match_oracle(hip_lib, oracle, scene):
    """two 96x64 frames, 3 segments, of a non-axis-aligned scene under a rotating ubo.model: the device re-pose, the
    refit and the posed pair records against the oracle — hit ids, visibility ids, depth and traced colour bit for bit"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import HipBackend, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan
    if scene == "heightfield":
        xyz, idx = _heightfield(20)
        xyz = (xyz * F32(2.0) + np.array([0, 1.0, 0], F32)).astype(F32)
    else:
        xyz, idx = _soup(np.random.default_rng(707), 3000, lo=-0.8, hi=0.8, size=0.08)
        xyz = (xyz + np.array([0, 1.0, 0], F32)).astype(F32)
    w, h, seg, n = 96, 64, 3, 3
    be = HipBackend(w, h, StripPlan(h, 1, 0, n), max_segments=seg, flags=hip_lib.FLAG_EXACT_FILTER,
                    debug_mask=hip_lib.DEBUG_HIT_ID)
    app = PathTracingApplication(be, w, h, n)
    app.objVertices, app.objIndices = xyz, idx
    app.buildAccelerationStructure()
    tris = oracle.flatten(xyz, idx)
    ref = oracle.OracleApp(w, h, tris, max_segments=seg, iterations=n)
    ctx = be.ctx
    try:
        for f, m in enumerate([_rot(0.7, 0.4, (0.0, 0.3, 0.0)), _rot(0.75, 0.55, (0.05, 0.25, -0.1))]):
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
            st = ctx.debug_bvh_check()
            assert st["boxes_not_containing"] == 0 and st["dangling"] == 0 and st["bad_refs_to_triangles"] == 0, (scene, f, st)
    finally:
        be.close()
