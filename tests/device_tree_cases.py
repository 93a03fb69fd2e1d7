"""Meshes for the two device tree builders (csrc/bvh_build.hip, csrc/bvh_build_sah.hip), numpy only.

Every case is a function that returns (xyz, idx) — float32 vertices, uint32 triangle indices — and says in its docstring what
it is for.  LBVH_CASES and SAH_CASES name them: tag -> (function, arguments, upload flags).  What a case claims about itself
(which Morton cells its centres fall into, where the SAH tree takes the median, how a root splits) is asserted from the numpy
restatements in test_device_tree_cpu.py, not assumed; test_device_tree_gpu.py holds the device's trees to the restatements
(LBVH) and to the host builder's tree (SAH) array for array."""
import numpy as np

import test_traversal_gpu as T
from test_device_bvh_gpu import _chain_scene
from test_device_sah_cpu import deep_scene

F32 = np.float32
FORCE_BVH = 2  # RTPT_FLAG_FORCE_BVH
CELLS = 1 << 21  # Morton cells per axis
GRID_STRIDE_FIRST = 1024 * 256  # k_prim_centre runs at most 1,024 blocks of 256: ids from here on belong to a block's second stride


def _mesh(tri):
    tri = np.ascontiguousarray(tri, F32).reshape(-1, 3, 3)
    return tri.reshape(-1, 3), np.arange(3 * len(tri), dtype=np.uint32).reshape(-1, 3)


def tris_of(xyz, idx):
    """the flattened scene of a mesh without instances: [n, 9] float32"""
    return np.ascontiguousarray(np.asarray(xyz, F32)[np.asarray(idx, np.int64)].reshape(-1, 9))


def _about(c, h):
    """triangles whose box is c -+ h on every axis: with c -+ h exact in binary32 the centre 0.5 mn + 0.5 mx is c exactly"""
    c = np.asarray(c, np.float64).reshape(-1, 3)
    off = np.array([[-1, -1, -1], [1, 1, 1], [1, -1, 1]], np.float64) * h
    tri = c[:, None, :] + off[None, :, :]
    assert np.array_equal(tri.astype(F32).astype(np.float64), tri), "the vertices must be binary32 numbers"
    return tri.astype(F32)


# ------------------------------------------------------------------------------ LBVH
def count_soup(n):
    """n triangles of a random soup.  1 .. 5: the smallest trees (one primitive has no internal node; 2 .. 5 have every shape
    of Karras' search at the ends of the array); 255 .. 513: the last thread of a 256-block, the first of the next and the
    block without a neighbour, for k_morton, k_hierarchy (n - 1 threads), k_emit_* and k_heights (n threads)"""
    return T._soup(np.random.default_rng([606, n]), n, size=0.15 if n <= 64 else 0.06)


def count_pairs(n):
    """the first n quads of a non-planar height field, each a fan pair: n primitives of two triangles (w = 2) at the counts
    of count_soup — leaf references and leaf order carry the factor w"""
    xyz, idx = T._heightfield(24)
    assert 2 * n <= len(idx)
    return xyz, idx[:2 * n]


def copies(n):
    """n copies of one triangle: every Morton key is equal, so the tree is decided by the sorted position alone — which a
    stable sort makes the id — through the position half of the augmented key"""
    tri = np.array([[0.1, 0.2, 0.3], [0.4, 0.2, 0.35], [0.2, 0.5, 0.3]], F32)
    return _mesh(np.tile(tri, (n, 1, 1)))


def tie_runs(n=331):
    """a soup whose triangle i occurs 1 + (i mod 9) times, copy c of every triangle that has one before copy c + 1 of any:
    runs of 1 .. 9 equal keys inside a varied key set, the members of a run far apart by id.  The leaf order inside a run is
    the id order only if the sort is stable, and k_hierarchy has to find splits inside and at the ends of runs"""
    base = T._soup(np.random.default_rng(707), n)[0].reshape(n, 3, 3)
    ids = [i for c in range(9) for i in range(n) if c <= i % 9]
    return _mesh(base[np.array(ids)])


# descending, so neighbouring cells stand in the mesh against their key order: a key that cannot tell them apart (20 bits per
# axis) leaves them in id order, which is then the wrong one
CELL_PROBES = ((1 << 21) - 1, (1 << 21) - 2, 1 << 20, (1 << 20) - 1, 1, 0)
CELL_OTHER = 0.375  # the two axes a probe does not vary: 0.375 * 2^21 = 786432 exactly, the lower edge of that cell


def chosen_cells_expected():
    """the cells of chosen_cells' primitives, [n, 3]"""
    out = [[0, 0, 0], [CELLS - 1] * 3]
    for a in range(3):
        for i in CELL_PROBES:
            cell = [786432] * 3
            cell[a] = i
            out.append(cell)
    return np.array(out, np.int64)


def chosen_cells():
    """Centres placed in chosen Morton cells.  Two anchors with centres (0, 0, 0) and (1, 1, 1) fix the centre bounds at
    [0, 1]^3: the first lies exactly on the lower bound (cell 0), the second exactly on the upper one (quotient 2^21, the
    clamp to cell 2097151).  Then, for each axis in turn, centres at (i + 1/2) 2^-21 for i = 2^21 - 1, 2^21 - 2, 2^20, 2^20 - 1,
    1, 0 — both ends of the cell range and the carry into the top bit — with 0.375 (exactly the lower edge of cell 786432)
    on the two other axes.  Every vertex and centre is exact in binary32 and the extent is 1, so the quotient is exact: a key
    of 20 bits per axis, exchanged shifts or a clamp at another cell gives other keys, hence another tree"""
    c = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    for a in range(3):
        for i in CELL_PROBES:
            p = [CELL_OTHER] * 3
            p[a] = (i + 0.5) / CELLS
            c.append(p)
    return _mesh(_about(c, 2.0 ** -23))


def quotient_grid(n=4000):
    """Centres near 1e5 on a grid of binary32 neighbours (spacing 2^-7 there), extents 400, 397 and 389 spacings (about
    three units), so a Morton cell is 1.5e-6 wide and neighbouring centres lie some 5,000 cells apart.  c - lo and the extent
    are exact in either format; the quotient (c - lo) / ext * 2^21 rounded to binary32 has a spacing of up to 1/8 cell and
    falls into another cell than the binary64 one for more than 1 % of the centres (asserted): a builder that quantises in
    binary32 sorts them differently"""
    rng = np.random.default_rng(808)
    lo, h = 100000.0, 2.0 ** -7
    k = np.stack([rng.integers(0, m + 1, n) for m in (400, 397, 389)], 1)
    k[0], k[1] = (0, 0, 0), (400, 397, 389)
    return _mesh(_about(lo + k * h, h))


def cell_neighbours(n=1500):
    """A soup in which every triangle has a copy moved down one axis by less than one Morton cell (4e-7 here), the copy at
    the higher id.  Here binary32 numbers lie ten times closer than cells, c - lo rounds in binary32 but not in binary64,
    and whether a triangle and its copy share a cell decides their order: in one cell the lower id comes first, in two the
    copy does.  quotient_grid's centres are 5,000 cells apart, and there the binary32 quotient, though it moves 6 % of them
    by one cell, provably gives the same tree (test_device_tree_cpu.py); on this scene it gives another leaf order
    (asserted)"""
    rng = np.random.default_rng(1616)
    tri = T._soup(rng, n)[0].reshape(n, 3, 3)
    shift = np.zeros((n, 1, 3), F32)
    shift[np.arange(n), 0, np.arange(n) % 3] = (-rng.uniform(0.05, 0.95, n) * 0.8 / CELLS).astype(F32)
    return _mesh(np.concatenate([tri, (tri + shift).astype(F32)]))


def anisotropic(n=1500):
    """extent 1e13 on x, 1e-13 on y, none on z: the three axes of one scene at both ends of the range the binary64 quotient
    is there for, and the flat axis that must give cell 0"""
    xyz, idx = T._soup(np.random.default_rng(909), n)
    xyz = xyz.copy()
    xyz[:, 0] = (xyz[:, 0] * F32(1e13)).astype(F32)
    xyz[:, 1] = (xyz[:, 1] * F32(1e-13)).astype(F32)
    xyz[:, 2] = F32(0.25)
    return xyz, idx


def negative_zero(n=600):
    """a soup on a coarse grid (multiples of 1/8) whose zero coordinates are -0.0 or +0.0 at random: centres and centre
    bounds of either sign of zero, which the key must not tell apart, and many equal keys"""
    rng = np.random.default_rng(1010)
    v = np.round(rng.uniform(-0.5, 0.5, (n, 3, 3)) * 8) / 8
    v = v.astype(F32)
    zero = v == 0
    v[zero & (rng.random(v.shape) < 0.5)] = F32(-0.0)
    assert np.signbit(v[zero]).any() and not np.signbit(v[zero]).all()
    return _mesh(v)


def grid_stride():
    """262,144 + 257 triangles: k_prim_centre runs at most 1,024 blocks of 256 threads, so ids from 262,144 on are met in a
    block's SECOND stride only.  The two triangles whose centres are the lower and the upper centre bound on every axis sit
    at ids 262,144 + 3 and 262,144 + 250; a reduction that drops the second stride gets other bounds, and every key changes.
    The one large case.  Measured on an MI355X box: 0.8 s for the pre-order test (the restatement, one upload, the
    readbacks) and 1.1 s for the height-numbering one (upload, readbacks, the walk over both trees in Python)."""
    n = GRID_STRIDE_FIRST + 257
    xyz, idx = T._soup(np.random.default_rng(1111), n, size=0.01)
    tri = xyz.reshape(n, 3, 3).copy()
    small = np.array([[0, 0, 0], [0.01, 0, 0.005], [0, 0.01, 0.005]], F32)
    tri[GRID_STRIDE_FIRST + 3] = small - F32(1.0)
    tri[GRID_STRIDE_FIRST + 250] = small + F32(1.0)
    return _mesh(tri)


def chain_prefix(n):
    """the first n triangles of the chain scene (centres 2^-k along an axis: every Morton prefix splits one triangle off).
    48 of them give the deepest tree the device may keep (depth 47), 49 the first it must hand to the host builder
    (depth 48 = the traversal stack): the restatement's depth decides which, so a builder whose tree is deeper or
    shallower than the radix tree's falls back at another count"""
    xyz, idx = _chain_scene()
    return xyz[:3 * n], idx[:n]


# ------------------------------------------------------------------------------ SAH
K_SMALL = 1024  # bvh_build_sah.hip: a segment of more primitives is cut into chunks and handled by separate launches


def root_soup(n):
    """n triangles of a soup: a root of 1023 / 1024 (one workgroup, k_sah_small, its last thread's four slots part / all
    full) / 1025 (the first large segment: two chunks, the second of one primitive) / 2047 / 2048 / 2049 (two full chunks
    and the third)"""
    return T._soup(np.random.default_rng([1212, n]), n)


def root_pairs(n):
    """the first n quads of a 46 x 46 height field, row after row: n fan pairs at the root sizes of root_soup (counts in
    the bins are in triangles, sizes in primitives)"""
    xyz, idx = T._heightfield(46)
    assert 2 * n <= len(idx)
    return xyz, idx[:2 * n]


def two_clusters(n_low, n_high):
    """two soups far apart on x, n_low triangles at the low end: SAH splits the root between them, so the children are
    segments of exactly 1024 (small) and 1025 (large) primitives BELOW the root, in either order"""
    rng = np.random.default_rng([1313, n_low])
    a = T._soup(rng, n_low, lo=-0.2, hi=0.2, size=0.02)[0] + np.array([-3, 0, 0], F32)
    b = T._soup(rng, n_high, lo=-0.2, hi=0.2, size=0.02)[0] + np.array([3, 0, 0], F32)
    tri = np.concatenate([a, b]).astype(F32).reshape(-1, 3, 3)
    perm = rng.permutation(len(tri))  # ids of either cluster all over the mesh
    return _mesh(tri[perm])


CROSS_CHUNK_N = 5 * 1024 + 17


def cross_chunk_low(n=CROSS_CHUNK_N):
    return np.arange(n) % 3 == 0


def cross_chunk():
    """5 * 1024 + 17 primitives in two clusters far apart on x, triangle id in the low cluster when id % 3 == 0: the root is
    split by SAH between the clusters, and each of its six chunks of 1,024 positions holds members of both sides — the stable
    partition across chunks needs the left count of every chunk before (chunk_off) to place either side"""
    n = CROSS_CHUNK_N
    rng = np.random.default_rng(1414)
    tri = T._soup(rng, n, lo=-0.2, hi=0.2, size=0.02)[0].reshape(n, 3, 3)
    tri = tri + np.where(cross_chunk_low(n), F32(-3), F32(3))[:, None, None] * np.array([1, 0, 0], F32)
    return _mesh(tri)


def signed_zero_copies(n):
    """n copies of one triangle in the plane x = 0, the x of all three vertices +0.0 in the even copies and -0.0 in the odd
    ones: the centres are +0 and -0 on x and equal on y and z.  No centroid extent is positive, so there is no SAH split and
    the root takes the object median on the first widest axis, x, by (centre, id) — where -0 == +0, so the order is by id
    and the left half is the lower ids.  An integer key that keeps the sign of zero puts the odd copies first.  n = 200: the
    rank count of k_sah_small; n = 3000: the two radix sorts"""
    tri = np.tile(np.array([[0.0, 0.2, 0.3], [0.0, 0.6, 0.35], [0.0, 0.3, 0.7]], F32), (n, 1, 1))
    tri[1::2, :, 0] = F32(-0.0)
    assert np.signbit(tri[1::2, :, 0]).all() and not np.signbit(tri[0::2, :, 0]).any()
    return _mesh(tri)


DEEP_K = (-40, 106)  # exponents of the peeled triangles: centres 2^40 .. 2^-105
CLUSTER_SCALE = -120  # the cluster's centres: (1 + j) 2^-120, normal binary32 numbers


def large_median(n_cluster):
    """deep_scene's peeling triangles (c, c + e_y, c + e_z), c = 2^-k e_x, with the exponents cut to k = -40 .. 105, and a
    cluster of n_cluster such triangles at c = (1 + j) 2^-120 e_x, j in a shuffled order: distinct normal binary32
    centres far below the smallest peeled scale, and every difference of two of them normal as well.  SAH peels about six
    triangles per level and never separates the cluster (all of it lies in bin 0), so at depth 22 a range of more than
    1,024 primitives with DISTINCT centres takes the object median: the two radix sorts, ordered by centre and not by id.
    1,500: one such segment.  4,200: its halves (and theirs) are above 1,024 too — several large median segments in one
    level, which the second, stable sort by segment keeps apart"""
    k = np.arange(*DEEP_K)
    assert np.array_equal(deep_scene()[0][0::3, 0][:len(k)], np.ldexp(F32(1), -k).astype(F32))  # deep_scene's own, cut
    j = np.random.default_rng([1515, n_cluster]).permutation(n_cluster)
    x = np.concatenate([np.ldexp(1.0, -k), (1.0 + j) * 2.0 ** CLUSTER_SCALE])
    c = np.zeros((len(x), 3), F32)
    c[:, 0] = x.astype(F32)
    assert np.array_equal(c[:, 0].astype(np.float64), x) and (c[:, 0] >= np.finfo(F32).tiny).all()
    tri = np.stack([c, c + np.array([0, 1, 0], F32), c + np.array([0, 0, 1], F32)], 1).astype(F32)
    return _mesh(tri)


LBVH_COUNTS = (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513)

LBVH_CASES = {}
for _n in LBVH_COUNTS:
    LBVH_CASES[f"soup n={_n}"] = (count_soup, (_n,), FORCE_BVH)
    LBVH_CASES[f"pairs n={_n}"] = (count_pairs, (_n,), FORCE_BVH)
for _n in (1023, 1024, 1025, 3000):
    LBVH_CASES[f"copies n={_n}"] = (copies, (_n,), 0)
LBVH_CASES["tie runs"] = (tie_runs, (), 0)
LBVH_CASES["chosen cells"] = (chosen_cells, (), FORCE_BVH)
LBVH_CASES["quotient grid"] = (quotient_grid, (), 0)
LBVH_CASES["cell neighbours"] = (cell_neighbours, (), 0)
LBVH_CASES["anisotropic"] = (anisotropic, (), 0)
LBVH_CASES["negative zero"] = (negative_zero, (), 0)
LBVH_CASES["chain prefix 48"] = (chain_prefix, (48,), FORCE_BVH)
LBVH_CASES["grid stride"] = (grid_stride, (), 0)
# falls back to the host builder: the restatement's depth says so, there is no device tree to compare
LBVH_FALLBACK_CASES = {"chain prefix 49": (chain_prefix, (49,), FORCE_BVH), "chain": (_chain_scene, (), 0)}

SAH_CASES = {}
for _n in (1023, 1024, 1025, 2047, 2048, 2049):
    SAH_CASES[f"root soup n={_n}"] = (root_soup, (_n,), 0)
    SAH_CASES[f"root pairs n={_n}"] = (root_pairs, (_n,), 0)
SAH_CASES["clusters 1024|1025"] = (two_clusters, (1024, 1025), 0)
SAH_CASES["clusters 1025|1024"] = (two_clusters, (1025, 1024), 0)
SAH_CASES["cross chunk"] = (cross_chunk, (), 0)
SAH_CASES["signed zero n=200"] = (signed_zero_copies, (200,), 0)
SAH_CASES["signed zero n=3000"] = (signed_zero_copies, (3000,), 0)
SAH_CASES["large median 1500"] = (large_median, (1500,), 0)
SAH_CASES["large median 4200"] = (large_median, (4200,), 0)


def borrowed_lbvh_cases(cornell, lattice, scaled_soup):
    """tag -> (xyz, idx, xf, flags): test_device_bvh_gpu._structure_cases, the small lattice of fan pairs and the two scaled
    soups (the chain scene is in LBVH_FALLBACK_CASES)"""
    from test_device_bvh_gpu import _structure_cases
    cases = {f"structure: {tag}": (xyz, idx, None, flags) for tag, (xyz, idx, flags) in _structure_cases(cornell).items()}
    cases["lattice"] = tuple(lattice) + (0,)
    for scale in (1e-13, 1e13):
        cases[f"soup x {scale:g}"] = tuple(scaled_soup(scale)) + (None, 0)
    return cases


BORROWED_TAGS = list(borrowed_lbvh_cases((None, None), (None, None, None), lambda scale: (None, None)))


def make(cases, tag):
    fn, args, flags = cases[tag]
    xyz, idx = fn(*args)
    return np.ascontiguousarray(xyz, F32), np.ascontiguousarray(idx, np.uint32), flags
