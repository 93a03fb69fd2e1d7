"""Hostile instance moves for a tree that is REFIT, not rebuilt (test_refit_moves_cpu.py, test_refit_moves_gpu.py).

D4: closest hit = min over (t, id) of one ray-triangle routine, so a tree that keeps the topology of another pose may only
cost time.  Here six instances of a small mesh stand on the corners of a 2 x 2 x 2 lattice (spacing 1.5, centred: no
translation component is 0, so a zero-scaled instance is the same non-zero point three times and never mixes +0 / -0),
and a move replaces their transforms with ones the tree was not built for:

  stack       every instance takes instance 0's transform: six bitwise copies of every triangle, in six subtrees
  swap        instance i takes the transform of instance n-1-i: the tree's spatial order is wrong everywhere
  fling       the last instance + 1e5 on x: one 16-bit grid cell is ~1.5, more than an instance and than the lattice spacing
  collapse    instance 1 flattened onto a plane y = const, instance 2 onto a point
  mirror      determinants below zero: instance 0 mirrored in x, instance 3 rotated about z and mirrored in z
  scales      instance 0 x 1e-3 (smaller than the padding and than a grid cell), instance 1 x 1e3
  all_points  (small scenes) every instance a point: every (2q, 2q + 1) is a fan pair bit for bit, nothing can be hit
  home        the upload's transforms again

The rays of a case come from the moved (and, under a model matrix, posed) triangles of the oracle, instance by instance
(test_traversal_gpu.ray_families on each instance's own triangles; origins drawn from the whole scene's box would miss
everything once an instance is flung), plus `crossing` (fling: between the home cluster and the flung instance, 1e5 apart,
both ways) and `between` (stack, swap: from inside one instance's box at the vertices of the next).  The families that
are documented open D4 gaps (test_traversal_gpu.test_known_gaps) stay out: no in-plane rays, no axis rays on heightfields.

reference() traces a case once with the oracle's brute force and keeps it for every test of the session; its arrays are
read-only.  check_floors() is what keeps a case from passing by missing everything."""
from collections import namedtuple

import numpy as np

import test_traversal_gpu as T
from test_instances_gpu import _general_xforms

F32 = np.float32
SEED = 1
N_RAYS = 300          # per instance and family
N_INST = 6
SPACING = 1.5
FLING = 1.0e5
TMAX = 4.0e5          # cfg.ray_tmax of every context here, and the oracle's: the default 10 000 would cut `crossing` short
LARGE = ("heightfield", "soup", "sphere")
SMALL = ("small_pairs", "small_soup")
MOVES = ("stack", "swap", "fling", "collapse", "mirror", "scales", "home")
SMALL_MOVES = ("stack", "collapse", "all_points", "home")
ALL_MOVES = ("stack", "swap", "fling", "collapse", "mirror", "scales", "all_points", "home")
PAIRED = {"heightfield": True, "soup": False, "sphere": True, "small_pairs": True, "small_soup": False}
# share of a family's rays the oracle must hit (per mesh and move; `crossing`: must hit the instance aimed at)
FLOORS = {"aimed": 0.50, "on_surface": 0.25, "random": 0.05, "tiny_components": 0.05, "axis": 0.05, "crossing": 0.50,
          # `between` is `aimed` from other origins: a box of one instance at vertices of another (no floor of its own is set)
          "between": 0.50}

_meshes, _refs = {}, {}


def mesh(name):
    """(xyz, idx) of the base mesh, inside [-0.5, 0.5]^3 up to the soups' scatter"""
    if name not in _meshes:
        rng = np.random.default_rng([SEED, 11, (LARGE + SMALL).index(name)])
        _meshes[name] = {"heightfield": lambda: T._heightfield(12),           # 288 triangles, all fan pairs
                         "soup": lambda: T._soup(rng, 400, size=0.08),        # unpaired
                         "sphere": lambda: T._sphere(16, 8),                  # 256, paired, zero-area halves at the poles
                         "small_pairs": lambda: T._heightfield(2),            # 8 x 6 = 48: the brute-force route
                         # 10 x 6 = 60, unpaired at upload; large triangles about a small cube: ten sparse ones would be missed by most rays
                         "small_soup": lambda: T._soup(rng, 10, lo=-0.1, hi=0.1, size=0.2)}[name]()
        for a in _meshes[name]:
            a.setflags(write=False)
    return _meshes[name]


def moves_of(name):
    return SMALL_MOVES if name in SMALL else MOVES


def _rot3(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def x0():
    """the upload's transforms [6, 12] (rows of a 3 x 4, translation in columns 3, 7, 11).  Six of the lattice's eight
    corners; instances 0 and 1 share a line along x, the last one (the one `fling` moves) shares its line with instance 4
    only, so four of the five that stay home are seen from +x without another in front.  Instances 4 and 5 are rotated."""
    h = 0.5 * SPACING
    corners = [(-h, -h, -h), (h, -h, -h), (-h, h, -h), (h, -h, h), (-h, h, h), (h, h, h)]
    out = np.zeros((N_INST, 3, 4))
    for i, c in enumerate(corners):
        out[i, :, :3] = np.eye(3)
        out[i, :, 3] = c
    out[4, :, :3] = _rot3(0.4, -0.7, 0.2)
    out[5, :, :3] = _rot3(-1.1, 0.3, 0.9)
    return np.ascontiguousarray(out.astype(F32).reshape(N_INST, 12))


def _linear(x, i):
    return x[i].reshape(3, 4)[:, :3].astype(np.float64)


def _with_linear(x, i, m):
    r = x[i].reshape(3, 4).copy()
    r[:, :3] = np.asarray(m).astype(F32)
    x[i] = r.ravel()


def move(name):
    """the [6, 12] float32 transforms of a move, derived from x0()"""
    x = x0()
    if name == "home":
        pass
    elif name == "stack":
        x[:] = x[0]
    elif name == "swap":
        x = np.ascontiguousarray(x[::-1])
    elif name == "fling":
        x[-1, 3] += F32(FLING)
    elif name == "collapse":
        _with_linear(x, 1, np.diag([1.0, 0.0, 1.0]) @ _linear(x, 1))   # world y = the translation's, exactly
        _with_linear(x, 2, np.zeros((3, 3)))
    elif name == "mirror":
        _with_linear(x, 0, _linear(x, 0) @ np.diag([-1.0, 1.0, 1.0]))
        _with_linear(x, 3, _rot3(0.0, 0.0, 0.8) @ np.diag([1.0, 1.0, -1.0]))
    elif name == "scales":
        _with_linear(x, 0, _linear(x, 0) * 1e-3)
        _with_linear(x, 1, _linear(x, 1) * 1e3)
    elif name == "all_points":
        for i in range(N_INST):
            _with_linear(x, i, np.zeros((3, 3)))
    else:
        raise KeyError(name)
    x = np.ascontiguousarray(x, F32)
    x.setflags(write=False)
    return x


def model(name):
    """a column-major ubo.model: the identity, or rotation x shear x scale with irrational entries and a translation"""
    m = np.eye(4)
    if name == "general":
        m[:3, :4] = _general_xforms(1)[0].reshape(3, 4)
    else:
        assert name == "identity"
    return np.ascontiguousarray(m.astype(F32).T).ravel()


def posed(oracle, tris, model_name):
    """flattened triangles under ubo.model: the LUT's vertices (the device re-pose copies under the identity)"""
    if model_name == "identity":
        return tris
    return np.ascontiguousarray(oracle.lut(tris, model(model_name))[1:].reshape(-1, 3, 4)[:, :, :3].reshape(-1, 9))


def instance_of(ids, n_base):
    """instance index of 1-based winner ids (-1: no hit)"""
    ids = np.asarray(ids, np.int64)
    return np.where(ids > 0, (ids - 1) // n_base, -1)


# ------------------------------------------------------------------------------ rays
def _box(tris, rng, n):
    lo, hi, _ = T._bounds(tris)
    c, ext = 0.5 * (lo + hi), np.maximum(hi - lo, 1e-3)
    return rng.uniform(c - 0.75 * ext, c + 0.75 * ext, (n, 3)).astype(F32)


def _vertices(tris, rng, n):
    t = tris.reshape(-1, 3, 3)
    return t[rng.integers(0, len(t), n), rng.integers(0, 3, n)]


def _rays(mesh_name, move_name, tris, rng):
    """{family: rays [k, 6]} and {family: target instance [k]} (the instance a ray was generated on / aimed at)"""
    per = tris.reshape(N_INST, -1, 9)
    names = ["random", "aimed", "on_surface", "tiny_components"]
    if "heightfield" not in mesh_name and mesh_name != "small_pairs":   # small_pairs is a heightfield too
        names.append("axis")
    fams = {k: [] for k in names}
    for i in range(N_INST):
        f = T.ray_families(per[i], rng, n=N_RAYS, in_plane=False)
        for k in names:
            fams[k].append(f[k])
    fams = {k: np.concatenate(v) for k, v in fams.items()}
    inst = {k: np.repeat(np.arange(N_INST), N_RAYS) for k in fams}
    if move_name == "fling":
        home, far = per[:-1].reshape(-1, 9), per[-1]
        lo, hi, _ = T._bounds(home)
        n = 3 * N_RAYS
        there = T._aim(rng.uniform(lo, hi, (n, 3)).astype(F32), _vertices(far, rng, n))
        k = rng.integers(0, N_INST - 1, n)
        tgt = np.stack([_vertices(per[j], rng, 1)[0] for j in k])
        back = T._aim(_box(far, rng, n), tgt)
        fams["crossing"] = np.concatenate([there, back])
        inst["crossing"] = np.concatenate([np.full(n, N_INST - 1), k])
    if move_name in ("stack", "swap"):
        nxt = [(i + 1) % N_INST for i in range(N_INST)]
        fams["between"] = np.concatenate([T._aim(_box(per[i], rng, N_RAYS), _vertices(per[j], rng, N_RAYS)) for i, j in enumerate(nxt)])
        inst["between"] = np.repeat(np.array(nxt), N_RAYS)
    return fams, inst


Case = namedtuple("Case", "mesh move model n_base xf tris fams inst rays wid wts")


def reference(oracle, mesh_name, move_name, model_name="identity"):
    """the case (mesh, move, model) traced by the oracle's brute force, once per session"""
    key = (mesh_name, move_name, model_name)
    if key not in _refs:
        xyz, idx = mesh(mesh_name)
        xf = move(move_name)
        tris = posed(oracle, oracle.flatten(xyz, idx, xf), model_name)
        rng = np.random.default_rng([SEED, (LARGE + SMALL).index(mesh_name), ALL_MOVES.index(move_name), int(model_name != "identity")])
        fams, inst = _rays(mesh_name, move_name, tris, rng)
        rays = np.concatenate(list(fams.values()))
        wid, wts = oracle.trace_rays(tris, rays, tmax=TMAX)
        for a in (tris, rays, wid, wts, *fams.values(), *inst.values()):
            a.setflags(write=False)
        _refs[key] = Case(mesh_name, move_name, model_name, len(idx), xf, tris, fams, inst, rays, wid, wts)
    return _refs[key]


def by_family(case):
    """{family: (oracle ids, oracle t)}"""
    out, at = {}, 0
    for fam, r in case.fams.items():
        out[fam] = (case.wid[at:at + len(r)], case.wts[at:at + len(r)])
        at += len(r)
    return out


def hit_shares(case):
    """{family: share of the rays that count which the oracle hits}.  Rays generated on the instance `collapse` turns into
    a point (2, every family) or starting on the one it flattens (1, on_surface: most leave the plane at once) do not
    count; under all_points nothing can be hit and nothing counts."""
    out = {}
    for fam, (wid, _) in by_family(case).items():
        count = np.ones(len(wid), bool)
        if case.move == "collapse":
            count &= case.inst[fam] != 2
            if fam == "on_surface":
                count &= case.inst[fam] != 1
        if fam == "crossing":
            hit = instance_of(wid, case.n_base) == case.inst[fam]
        else:
            hit = wid > 0
        out[fam] = float(hit[count].mean())
    return out


def check_floors(case):
    if case.move == "all_points":
        return
    for fam, share in hit_shares(case).items():
        assert share >= FLOORS[fam], f"{case.mesh}/{case.move}/{case.model}: the oracle hits {share:.2f} of `{fam}` (floor {FLOORS[fam]})"
