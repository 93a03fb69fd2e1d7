"""What the device-tree tests (test_device_tree_gpu.py) rest on, checked without a GPU.

The LBVH builder is held there to scripts/lbvh_restate.py array for array, so the restatement itself is held here to the
DEFINITION of the tree it restates, by brute force over the ranges and from a second statement of the keys: the binary radix
tree over the augmented keys (Morton key, sorted position) of the primitives in stable key order — every node a contiguous
range of sorted positions, split where the highest bit in which its first and last augmented key differ flips, numbered
in pre-order, every primitive in one leaf.  The SAH builder is held on the device to the host builder's tree; here
scripts/sah_restate.py is held to the host builder on the new cases (nodes and depth, as test_device_sah_cpu.py does), because
it is the restatement that says which path a case takes.  And every precondition a case of device_tree_cases.py states
about itself is asserted."""
import os
import sys

import numpy as np
import pytest

import device_tree_cases as DC
import test_traversal_gpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import lbvh_restate  # noqa: E402
import sah_restate  # noqa: E402

F32 = np.float32
U64 = np.uint64
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF


# ------------------------------------------------------------------------------ a second statement of the keys
def centres(tris, w):
    v = np.ascontiguousarray(tris, F32).reshape(-1, 3 * w, 3)
    return (F32(0.5) * v.min(1) + F32(0.5) * v.max(1)).astype(F32)


def cells(tris, w, dtype=np.float64):
    """the Morton cell of every primitive per axis, the quotient evaluated in `dtype`"""
    c = centres(tris, w)
    lo, hi = c.min(0).astype(dtype), c.max(0).astype(dtype)
    ext = hi - lo
    with np.errstate(all="ignore"):
        x = (c.astype(dtype) - lo) / np.where(ext > 0, ext, dtype(1)) * dtype(2097152)
    x = np.where(ext > 0, x, dtype(0))
    return np.clip(np.floor(x.astype(np.float64)), 0, 2097151).astype(np.int64)


def interleave(q):
    """bit b of x, y, z at bits 3 b + 2, 3 b + 1, 3 b: one bit at a time"""
    key = np.zeros(len(q), U64)
    for b in range(21):
        for a, shift in ((0, 2), (1, 1), (2, 0)):
            key |= ((q[:, a].astype(U64) >> U64(b)) & U64(1)) << U64(3 * b + shift)
    return key


def deinterleave(key):
    q = np.zeros((len(key), 3), np.int64)
    for b in range(21):
        for a, shift in ((0, 2), (1, 1), (2, 0)):
            q[:, a] |= (((key >> U64(3 * b + shift)) & U64(1)) << U64(b)).astype(np.int64)
    return q


def _top_bit(x):
    """index of the highest set bit of every element of a uint64 array (all > 0)"""
    x = x.copy()
    r = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        m = (x >> U64(s)) != 0
        r += s * m
        x = np.where(m, x >> U64(s), x)
    return r


# ------------------------------------------------------------------------------ the definition
def assert_radix_tree(refs, leaf, keys, w, tag):
    """(refs, leaf) in the formats of rtpt_debug_bvh_topology are THE binary radix tree over `keys` (one per primitive, in
    primitive order), numbered in pre-order; returns its depth as rtpt_scene_build_info counts it"""
    n = len(keys)
    refs = np.asarray(refs, np.uint32).reshape(-1, 2).astype(np.int64)
    leaf = np.asarray(leaf, np.uint32).astype(np.int64)
    order = np.lexsort((np.arange(n), keys))  # by key, equal keys by id: what a stable sort leaves
    assert np.array_equal(leaf, (order[:, None] * w + np.arange(w)[None, :]).reshape(-1)), (tag, "leaf order")
    assert np.array_equal(np.sort(leaf), np.arange(n * w)), (tag, "every triangle in exactly one slot")
    if n == 1:
        assert refs.tolist() == [[LEAF | (w - 1), EMPTY]], (tag, refs)
        return 0
    m = n - 1
    assert refs.shape == (m, 2), (tag, refs.shape)
    is_leaf = (refs & LEAF) != 0
    assert ((refs[is_leaf] & 3) == w - 1).all(), (tag, "a leaf holds one primitive")
    pos = np.where(is_leaf, ((refs & 0x7FFFFFFF) >> 2) // w, -1)
    assert ((((refs & 0x7FFFFFFF) >> 2) % w)[is_leaf] == 0).all(), tag
    assert np.array_equal(np.sort(pos[is_leaf]), np.arange(n)), (tag, "every primitive in exactly one leaf")
    kid = np.where(is_leaf, -1, refs)
    own = np.arange(m)[:, None]
    assert ((kid > own) & (kid < m))[~is_leaf].all(), (tag, "every child behind its parent")
    first, last, inner = np.zeros(m, np.int64), np.zeros(m, np.int64), np.ones(m, np.int64)
    split = np.zeros(m, np.int64)  # the last sorted position of the left child
    for i in range(m - 1, -1, -1):
        (l, r), (pl, pr) = kid[i], pos[i]
        first[i] = pl if l < 0 else first[l]
        split[i] = pl if l < 0 else last[l]
        rfirst = pr if r < 0 else first[r]
        last[i] = pr if r < 0 else last[r]
        assert rfirst == split[i] + 1, (tag, i, "the children are neighbouring ranges")
        nl = 0 if l < 0 else inner[l]
        inner[i] += nl + (0 if r < 0 else inner[r])
        assert l < 0 or l == i + 1, (tag, i, "pre-order: the left child follows its parent")
        assert r < 0 or r == i + 1 + nl, (tag, i, "pre-order: the right child follows the left subtree")
    assert (first[0], last[0], inner[0]) == (0, n - 1, m), (tag, "the root covers everything")
    # the split of every node, by brute force over its range, level by level
    level = np.zeros(m, np.int64)
    for i in range(m):
        for c in kid[i]:
            if c >= 0:
                level[c] = level[i] + 1
    ks = keys[order].astype(U64)
    same = ks[first] == ks[last]
    top = np.where(same, _top_bit(np.where(same, (first ^ last).astype(U64), U64(1))), _top_bit(np.where(same, U64(1), ks[first] ^ ks[last])))
    for lv in range(int(level.max()) + 1):
        nodes = np.nonzero(level == lv)[0]
        length = last[nodes] - first[nodes] + 1
        start = np.cumsum(length) - length
        at = np.repeat(first[nodes] - start, length) + np.arange(int(length.sum()))  # every sorted position of every range
        t, use_pos = np.repeat(top[nodes], length).astype(U64), np.repeat(same[nodes], length)
        word = np.where(use_pos, at.astype(U64), ks[at])
        bit = (word >> t) & U64(1)
        above = np.where(use_pos, at.astype(U64) >> t >> U64(1), ks[at] >> t >> U64(1))
        ref_above = np.repeat(np.where(same[nodes], first[nodes].astype(U64) >> top[nodes].astype(U64) >> U64(1),
                                       ks[first[nodes]] >> top[nodes].astype(U64) >> U64(1)), length)
        assert np.array_equal(above, ref_above), (tag, lv, "the range shares everything above its highest differing bit")
        assert (ks[at] == np.repeat(ks[first[nodes]], length))[use_pos].all(), (tag, lv, "a range split by position holds one key")
        assert np.array_equal(bit.astype(bool), at > np.repeat(split[nodes], length)), (tag, lv, "split where that bit flips")
    return int(level.max()) + 1


def _tree(tris):
    tris = np.ascontiguousarray(tris, F32).reshape(-1, 9)
    tree = lbvh_restate.Tree(tris)
    assert tree.w == (2 if T._pair_ok(tris) else 1)
    keys = lbvh_restate.morton_keys(tris, tree.w)
    assert np.array_equal(keys, interleave(cells(tris, tree.w))), "the keys against their second statement"
    return tree, keys


def _hold_to_the_definition(tris, tag):
    tree, keys = _tree(tris)
    depth = assert_radix_tree(tree.child_refs(), tree.leaf_order(), keys, tree.w, tag)
    assert depth == tree.depth and tree.n_nodes() == max(len(keys) - 1, 1), (tag, depth, tree.depth, tree.n_nodes())
    return tree, keys


# ------------------------------------------------------------------------------ LBVH
@pytest.mark.parametrize("tag", list(DC.LBVH_CASES) + list(DC.LBVH_FALLBACK_CASES))
def test_lbvh_restatement_is_the_radix_tree(tag):
    xyz, idx, _ = DC.make({**DC.LBVH_CASES, **DC.LBVH_FALLBACK_CASES}, tag)
    tree, _ = _hold_to_the_definition(DC.tris_of(xyz, idx), tag)
    if tag in DC.LBVH_FALLBACK_CASES:
        assert tree.depth >= 48, (tag, tree.depth)
    else:
        assert tree.depth < 48, (tag, tree.depth)
    if tag.startswith("pairs"):
        assert tree.w == 2
    if tag.startswith("chain prefix"):
        assert tree.depth == {"chain prefix 48": 47, "chain prefix 49": 48}[tag]
    if tag == "chain":
        assert tree.depth == 65


def test_lbvh_restatement_is_the_radix_tree_on_the_borrowed_scenes(oracle, cornell):
    from test_device_sah_gpu import _scaled_soup, _small_lattice
    cases = DC.borrowed_lbvh_cases(cornell, _small_lattice(cornell), _scaled_soup)
    assert list(cases) == DC.BORROWED_TAGS
    for tag, (xyz, idx, xf, flags) in cases.items():
        tree, _ = _hold_to_the_definition(oracle.flatten(xyz, idx, xf), tag)
        assert tree.depth < 48, (tag, tree.depth)
        if tag == "lattice":
            assert tree.w == 2 and len(tree.order) > 64


def test_copies_have_one_key_and_tie_runs_have_runs():
    for n in (1023, 1024, 1025, 3000):
        tree, keys = _tree(DC.tris_of(*DC.copies(n)))
        assert len(np.unique(keys)) == 1 and np.array_equal(tree.order, np.arange(n))
    xyz, idx = DC.tie_runs()
    tree, keys = _tree(DC.tris_of(xyz, idx))
    _, counts = np.unique(keys, return_counts=True)
    assert sorted(set(counts.tolist())) == list(range(1, 10)), "runs of every length 1 .. 9"
    ks = keys[tree.order]
    run = np.nonzero(ks[1:] == ks[:-1])[0]
    assert (tree.order[run + 1] > tree.order[run]).all(), "inside a run the ids ascend"
    assert (tree.order[run + 1] - tree.order[run]).min() > 30, "and lie far apart: the members of a run are interleaved with the mesh"


def test_chosen_cells_are_the_cells_the_case_names():
    tris = DC.tris_of(*DC.chosen_cells())
    c = centres(tris, 1)
    assert np.array_equal(c.min(0), np.zeros(3, F32)) and np.array_equal(c.max(0), np.ones(3, F32)), "the anchors fix the bounds at [0, 1]^3"
    assert np.array_equal(c[0], np.zeros(3, F32)) and np.array_equal(c[1], np.ones(3, F32)), "one centre on either bound"
    want = DC.chosen_cells_expected()
    assert np.array_equal(deinterleave(lbvh_restate.morton_keys(tris, 1)), want)
    for a in range(3):
        assert set(DC.CELL_PROBES) <= set(want[:, a].tolist())
    assert (want[1] == 2097151).all() and (c[1].astype(np.float64) * 2097152 == 2097152).all(), "the clamp"
    # 20 bits per axis, or the y and z shifts exchanged, are other keys in another order
    k21 = interleave(want)
    assert not np.array_equal(np.argsort(interleave(want >> 1), kind="stable"), np.argsort(k21, kind="stable"))
    assert not np.array_equal(np.argsort(interleave(want[:, [0, 2, 1]]), kind="stable"), np.argsort(k21, kind="stable"))


def test_quotient_grid_tells_binary32_from_binary64():
    tris = DC.tris_of(*DC.quotient_grid())
    c = centres(tris, 1)
    assert (np.abs(c - 1e5) < 4).all() and ((c.max(0) - c.min(0)) < 4).all() and ((c.max(0) - c.min(0)) > 3).all()
    assert np.array_equal(c, (1e5 + np.round((c.astype(np.float64) - 1e5) * 128) / 128).astype(F32)), "a grid of binary32 neighbours"
    q64, q32 = cells(tris, 1), cells(tris, 1, F32)
    moved = (q64 != q32).any(1).mean()
    assert moved >= 0.01, moved
    # ... and yet the tree is the same.  The binary32 quotient is off by one cell at most, and where it is, x = k / K * 2^21
    # lies within 1/8 of the integer N it is rounded across; k / K is no closer than 1 / (K 2^m) to a fraction of denominator
    # 2^m, so with K < 512 no such N is a multiple of 2^7: the two cells agree above bit 6.  Distinct centres of this grid lie
    # at least 4,096 cells apart, so the highest bit in which two keys differ — all that a radix tree reads — is the same.
    assert np.abs(q64 - q32).max() == 1 and ((q64 ^ q32) < 128).all()
    t64, t32 = lbvh_restate.Tree(tris), lbvh_restate.Tree(tris, keys=interleave(q32))
    assert np.array_equal(t64.child_refs(), t32.child_refs()) and np.array_equal(t64.leaf_order(), t32.leaf_order())


def test_cell_neighbours_tell_binary32_from_binary64():
    tris = DC.tris_of(*DC.cell_neighbours())
    q64, q32 = cells(tris, 1), cells(tris, 1, F32)
    assert (q64 != q32).any(1).mean() >= 0.01
    n = len(tris) // 2
    assert (np.abs(q64[:n] - q64[n:]).max(1) <= 1).all(), "a triangle and its copy: one cell or neighbouring cells"
    t64, t32 = lbvh_restate.Tree(tris), lbvh_restate.Tree(tris, keys=interleave(q32))
    differ = int((t64.leaf_order() != t32.leaf_order()).sum())
    assert differ >= 20, differ


def test_anisotropic_negative_zero_and_grid_stride_are_what_they_say():
    c = centres(DC.tris_of(*DC.anisotropic()), 1)
    ext = c.max(0).astype(np.float64) - c.min(0)
    assert 5e12 < ext[0] < 2e13 and 5e-14 < ext[1] < 2e-13 and ext[2] == 0, ext
    xyz, _ = DC.negative_zero()
    assert (np.signbit(xyz) & (xyz == 0)).sum() > 50 and (~np.signbit(xyz) & (xyz == 0)).sum() > 50
    c = centres(DC.tris_of(*DC.negative_zero()), 1)
    assert (np.signbit(c) & (c == 0)).any() and (~np.signbit(c) & (c == 0)).any(), "centres of either zero"
    xyz, idx = DC.grid_stride()
    assert len(idx) == 262144 + 257
    c = centres(DC.tris_of(xyz, idx), 1)
    first = DC.GRID_STRIDE_FIRST
    for a in range(3):
        assert c[:first, a].min() > c[first:, a].min() and c[:first, a].max() < c[first:, a].max(), "only the second stride sees the bounds"
        assert int(np.argmin(c[:, a])) == first + 3 and int(np.argmax(c[:, a])) == first + 250


# ------------------------------------------------------------------------------ SAH
@pytest.mark.parametrize("tag", list(DC.SAH_CASES))
def test_sah_restatement_agrees_with_the_host_builder(hip_lib, tag):
    xyz, idx, _ = DC.make(DC.SAH_CASES, tag)
    tris = DC.tris_of(xyz, idx)
    pairs = T._pair_ok(tris)
    assert pairs == tag.startswith("root pairs")
    host = hip_lib.bvh_check(tris, pairs=pairs)
    assert host["bad_triangle_refs"] == 0 and host["bad_child_refs"] == 0 and host["loose_boxes"] == 0, (tag, host)
    tree = sah_restate.Tree(tris, pairs=pairs)
    assert (tree.n_nodes(), tree.depth) == (host["nodes"], host["max_depth"]), (tag, tree.n_nodes(), tree.depth, host)
    assert tree.depth < 48
    refs, leaf = tree.child_refs, tree.leaf_order
    assert np.array_equal(np.sort(leaf), np.arange(len(tris), dtype=np.uint32)), tag
    leaves = refs[(refs != EMPTY) & ((refs & LEAF) != 0)]
    assert int(((leaves & 3) + 1).sum()) == len(tris) and int(((leaves & 3) + 1).max()) <= 2, tag
    n = len(tris) // tree.w
    root_left = tree.last[1] + 1 if tree.n_nodes() > 1 and tree.first[1] == 0 else None  # node 1: the root's left child, when internal
    big = [m for m in tree.median_at if m[1] > DC.K_SMALL]
    if tag.startswith("root"):
        assert n == int(tag.split("=")[1]) and not tree.median_at, (tag, n)
    elif tag.startswith("clusters"):
        want = int(tag.split()[1].split("|")[0])
        assert n == 2049 and root_left == want and not tree.median_at, (tag, root_left)
    elif tag == "cross chunk":
        low = DC.cross_chunk_low()
        assert n == 5 * 1024 + 17 and root_left == int(low.sum()) and not tree.median_at, (tag, root_left)
        assert np.array_equal(np.sort(tree.perm[:root_left]), np.nonzero(low)[0]), "the root is split between the clusters"
        for lo in range(0, n, 1024):
            assert 0 < int(low[lo:lo + 1024].sum()) < len(low[lo:lo + 1024]), "every chunk holds both sides"
    elif tag.startswith("signed zero"):
        c = tree.c
        assert (c[:, 0] == 0).all() and np.signbit(c[1::2, 0]).all() and not np.signbit(c[0::2, 0]).any(), "centres +0 and -0"
        assert (c[:, 1:] == c[0, 1:]).all(), "no extent on y and z"
        assert tree.median_at[0] == (0, n), (tag, tree.median_at[:3])
        assert np.array_equal(np.sort(tree.perm[:n // 2]), np.arange(n // 2)), "the left half is the lower ids"
        assert bool(big) == (n > DC.K_SMALL)
    elif tag.startswith("large median"):
        assert big and all(d >= 22 for d, _ in big), (tag, big)
        cluster = int(tag.split()[-1])
        assert big[0][0] == 22 and cluster < big[0][1] < cluster + 40, (tag, big)
        x = tree.c[:, 0]
        assert len(np.unique(x)) == len(x) and (x >= np.finfo(F32).tiny).all(), "distinct normal centres"
        per_depth = np.bincount([d for d, _ in big])
        assert (per_depth.max() >= 2) == (cluster == 4200), (tag, big)
    else:
        raise AssertionError(f"no precondition written for {tag}")
