"""The two device tree builders held to their restatements, node for node.

LBVH (csrc/bvh_build.hip): any valid tree passes test_device_bvh_gpu.py — boxes only cull and order (D4) — so there a
wrong Morton key, an unstable sort, another tie split or another numbering costs traversal time and nothing else.  Here
the arrays rtpt_debug_bvh_topology reads back must equal scripts/lbvh_restate.py's in every element, and depth and node count
of the build info the restatement's, on the cases of device_tree_cases.py; test_device_tree_cpu.py holds that restatement
to the definition of the radix tree.  Under RTPT_LBVH_ORDER=height the same tree must come back in the other numbering.

SAH (csrc/bvh_build_sah.hip): the reference is the host builder's tree, as in test_device_sah_gpu.py, on the cases that
reach the branches its scenes leave alone: segments of 1023 / 1024 / 1025 primitives, the cross-chunk partition with both
sides in every chunk, the median over signed zeros and the two-sort median with distinct centres and several segments."""
import os
import sys

import numpy as np
import pytest

import device_tree_cases as DC
import test_traversal_gpu as T
from test_device_bvh_gpu import CLEAN, _upload
from test_device_sah_gpu import SAH, _assert_sah_info, _assert_sah_tree, _canonical, _scaled_soup, _small_lattice, _topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import lbvh_restate  # noqa: E402

pytestmark = pytest.mark.gpu

F32 = np.float32
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF
_borrowed = {}  # the scenes of the existing structure tests, made once
_restated = {}  # tag -> the scene and what the restatement says of it: computed once, shared by the tests, never changed


def _lbvh_case(tag, oracle, cornell):
    if tag not in _restated:
        if tag in DC.BORROWED_TAGS:
            if not _borrowed:
                _borrowed.update(DC.borrowed_lbvh_cases(cornell, _small_lattice(cornell), _scaled_soup))
            xyz, idx, xf, flags = _borrowed[tag]
            tris = oracle.flatten(xyz, idx, xf)
        else:
            xyz, idx, flags = DC.make({**DC.LBVH_CASES, **DC.LBVH_FALLBACK_CASES}, tag)
            xf, tris = None, DC.tris_of(xyz, idx)
        tree = lbvh_restate.Tree(tris)
        refs, leaf = tree.child_refs(), tree.leaf_order()
        refs.setflags(write=False), leaf.setflags(write=False)
        _restated[tag] = dict(mesh=(xyz, idx, xf), flags=flags, refs=refs, leaf=leaf, depth=tree.depth, n_nodes=tree.n_nodes(),
                              n_prims=len(tree.order), w=tree.w)
    return _restated[tag]


def _assert_device_lbvh(hip_lib, info, case, tag):
    assert info["builder"] == hip_lib.BVH_BUILDER_DEVICE_LBVH and info["fallback"] == hip_lib.BVH_FALLBACK_NONE, (tag, info)
    want = {"n_nodes": case["n_nodes"], "depth": case["depth"], "n_primitives": case["n_prims"], "leaf_pairs": case["w"] - 1}
    assert {k: info[k] for k in want} == want, (tag, info, want)


def _valid(st, info):
    return all(st[k] == 0 for k in CLEAN) and st["largest_leaf"] <= 2 and st["nodes"] == info["n_nodes"]


def _first_difference(got, want):
    if got.shape != want.shape:
        return f"shape {got.shape} for {want.shape}"
    bad = np.nonzero((got != want).reshape(len(got), -1).any(1))[0]
    return None if not len(bad) else f"{len(bad)} of {len(got)} rows differ, first {bad[0]}: {got[bad[0]].tolist()} for {want[bad[0]].tolist()}"


# ------------------------------------------------------------------------------ LBVH: pre-order
@pytest.mark.parametrize("tag", DC.BORROWED_TAGS + list(DC.LBVH_CASES))
def test_lbvh_tree_equals_the_restatement(hip_lib, oracle, cornell, tag):
    """One upload per case; every element of both arrays, the depth and the node count.  The one large case, `grid stride`
    (262,401 triangles), takes 0.8 s measured on an MI355X box, most of it the restatement; every other case under 0.2 s"""
    case = _lbvh_case(tag, oracle, cornell)
    xyz, idx, xf = case["mesh"]
    with _upload(hip_lib, xyz, idx, xf, case["flags"] | hip_lib.FLAG_DEVICE_BVH_BUILD) as ctx:
        info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
        refs, leaf = ctx.debug_bvh_topology()
    _assert_device_lbvh(hip_lib, info, case, tag)
    valid = "a valid tree" if _valid(st, info) else f"not even a valid tree: {st}"
    assert np.array_equal(leaf, case["leaf"]), (tag, "leaf order", _first_difference(leaf, case["leaf"]), valid)
    assert np.array_equal(refs, case["refs"]), (tag, "child references", _first_difference(refs, case["refs"]), valid)
    assert _valid(st, info), (tag, st, info)


@pytest.mark.parametrize("tag", list(DC.LBVH_FALLBACK_CASES))
def test_lbvh_falls_back_exactly_where_the_restated_depth_says(hip_lib, oracle, cornell, tag):
    """depth 48 and more is the host builder's: `chain prefix 48` (depth 47) is among the cases above and stays on the device"""
    case = _lbvh_case(tag, oracle, cornell)
    assert case["depth"] >= 48 and _lbvh_case("chain prefix 48", oracle, cornell)["depth"] == 47
    xyz, idx, xf = case["mesh"]
    with _upload(hip_lib, xyz, idx, xf, case["flags"] | hip_lib.FLAG_DEVICE_BVH_BUILD) as ctx:
        info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
    assert info["builder"] == hip_lib.BVH_BUILDER_HOST_SAH and info["fallback"] == hip_lib.BVH_FALLBACK_DEPTH, (tag, info)
    assert all(st[k] == 0 for k in CLEAN) and info["depth"] < 48, (tag, st, info)


# ------------------------------------------------------------------------------ LBVH: numbered by height
def _heights(refs):
    """height of every node (0: both children leaves) and the parent of every node, children behind their parents"""
    m = len(refs)
    h, parent = [0] * m, [-1] * m
    rows = refs.tolist()
    for i in range(m - 1, -1, -1):
        for c in rows[i]:
            if c != EMPTY and not c & LEAF:
                assert i < c < m and parent[c] < 0, (i, c, "a child lies behind its parent and has one parent")
                parent[c] = i
                h[i] = max(h[i], h[c] + 1)
    return np.array(h), np.array(parent)


@pytest.mark.parametrize("tag", DC.BORROWED_TAGS + list(DC.LBVH_CASES))
def test_lbvh_height_numbering_is_the_same_tree(hip_lib, oracle, cornell, monkeypatch, tag):
    """RTPT_LBVH_ORDER=height: the leaf order and the multiset of leaf references of the restatement, the numbering rule of
    bvh_build.hip (descending height, node 0 the root, every child behind its parent) — and, walked from the root side by
    side with the restatement, the same tree"""
    case = _lbvh_case(tag, oracle, cornell)
    xyz, idx, xf = case["mesh"]
    monkeypatch.setenv("RTPT_LBVH_ORDER", "height")
    with _upload(hip_lib, xyz, idx, xf, case["flags"] | hip_lib.FLAG_DEVICE_BVH_BUILD) as ctx:
        info, st = ctx.scene_build_info(), ctx.debug_bvh_check()
        refs, leaf = ctx.debug_bvh_topology()
    _assert_device_lbvh(hip_lib, info, case, tag)
    assert _valid(st, info), (tag, st, info)
    want = case["refs"]
    assert np.array_equal(leaf, case["leaf"]), (tag, "leaf order", _first_difference(leaf, case["leaf"]))
    assert refs.shape == want.shape, (tag, refs.shape)
    is_leaf = lambda r: ((r & LEAF) != 0) | (r == EMPTY)
    assert np.array_equal(np.sort(refs[is_leaf(refs)]), np.sort(want[is_leaf(want)])), (tag, "the leaf references")
    h, parent = _heights(refs)
    assert (parent[1:] >= 0).all() and parent[0] < 0, (tag, "node 0 is the root, every other node is some node's child")
    assert (np.diff(h) <= 0).all(), (tag, "descending height")
    assert h[0] == _heights(want)[0][0] and (len(h) == 1 or h[0] > h[1]), (tag, "the root alone is the highest")
    # the same tree: corresponding nodes have corresponding children
    twin = [-1] * len(want)  # pre-order index -> height-order index
    twin[0] = 0
    rows_want, rows_got = want.tolist(), refs.tolist()
    for i in range(len(want)):  # pre-order: a parent is met before its children
        assert twin[i] >= 0, (tag, i)
        for a, b in zip(rows_want[i], rows_got[twin[i]]):
            if a == EMPTY or a & LEAF:
                assert a == b, (tag, i, hex(a), hex(b))
            else:
                assert b != EMPTY and not b & LEAF, (tag, i, hex(b))
                twin[a] = b
    assert sorted(twin) == list(range(len(want))), tag


# ------------------------------------------------------------------------------ SAH: the host's tree
@pytest.mark.parametrize("tag", list(DC.SAH_CASES))
def test_sah_tree_equals_the_host_builders(hip_lib, tag):
    xyz, idx, flags = DC.make(DC.SAH_CASES, tag)
    seen = []
    for _ in range(2):
        with _upload(hip_lib, xyz, idx, None, flags | SAH) as ctx:
            seen.append((ctx.scene_build_info(), ctx.debug_bvh_check(), ctx.debug_bvh_topology()))
    info, st, raw = seen[0]
    _assert_sah_info(hip_lib, info, tag)
    assert np.array_equal(raw[0], seen[1][2][0]) and np.array_equal(raw[1], seen[1][2][1]), (tag, "the same scene built twice")
    with _upload(hip_lib, xyz, idx, None, flags) as ctx:
        hinfo, htopo = ctx.scene_build_info(), _topology(ctx)
    assert hinfo["builder"] == hip_lib.BVH_BUILDER_HOST_SAH and hinfo["fallback"] == hip_lib.BVH_FALLBACK_NONE, (tag, hinfo)
    valid = "a valid tree" if _valid(st, info) else f"not even a valid tree: {st}"
    for k in ("n_nodes", "depth", "n_primitives", "leaf_pairs"):
        assert info[k] == hinfo[k], (tag, k, info, hinfo, valid)
    assert info["leaf_pairs"] == int(tag.startswith("root pairs")), (tag, info)
    assert np.array_equal(raw[0], htopo[0]), (tag, "child references", _first_difference(raw[0], htopo[0]), valid)
    canon = _canonical(raw[0], raw[1])
    assert np.array_equal(canon, htopo[1]), (tag, "leaf order", _first_difference(canon, htopo[1]), valid)
    assert _valid(st, info), (tag, st, info)


# ------------------------------------------------------------------------------ SAH: closest hit on the new paths
@pytest.fixture
def sah_env(monkeypatch):
    monkeypatch.setenv("RTPT_DEVICE_BVH", "sah")
    return monkeypatch


@pytest.mark.parametrize("tag", ["signed zero n=200", "signed zero n=3000", "cross chunk"])
def test_sah_closest_hit(hip_lib, oracle, sah_env, tag):
    xyz, idx, _ = DC.make(DC.SAH_CASES, tag)
    _assert_sah_tree(hip_lib, xyz, idx, tag=tag)
    fams = T.ray_families(oracle.flatten(xyz, idx), np.random.default_rng(1717), n=1000)
    T.check_case(hip_lib, oracle, sah_env, tag, xyz, idx, {f: fams[f] for f in ("random", "aimed", "axis")}, floors={"aimed": 100})


def test_sah_closest_hit_large_median(hip_lib, oracle, sah_env):
    """rays along x from between two neighbouring peeled triangles, as test_closest_hit_on_the_median_paths sends them; the
    one below the smallest peeled triangle runs into the cluster, whose 1,500 hits tie on t and are decided by id"""
    tag = "large median 1500"
    xyz, idx, _ = DC.make(DC.SAH_CASES, tag)
    _assert_sah_tree(hip_lib, xyz, idx, tag=tag)
    rng = np.random.default_rng(1818)
    n = 1000
    k = rng.integers(DC.DEEP_K[0] + 1, DC.DEEP_K[1], n)
    yz = rng.uniform(0.05, 0.45, (n, 2))
    o = np.stack([0.75 * np.ldexp(1.0, -k), yz[:, 0], yz[:, 1]], 1)
    d = np.zeros((n, 3))
    d[:, 0] = rng.choice([-1.0, 1.0], n)
    rays = np.ascontiguousarray(np.concatenate([o, d], 1).astype(F32))
    out = T.check_case(hip_lib, oracle, sah_env, tag, xyz, idx, {"along_x": rays}, tmax=1e30, floors={"along_x": 900})
    ids = out["along_x"][0]
    assert len(np.unique(ids)) > 100, "the rays should end in many different leaves"
    assert (ids > DC.DEEP_K[1] - DC.DEEP_K[0]).any(), "and some in the cluster"
