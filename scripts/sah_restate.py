"""numpy restatement of the SAH builder — the host's (csrc/bvh.cpp: Builder::build) and the device's (csrc/bvh_build_sah.hip),
which are the same algorithm: 32 bins per axis over the centroid bounds, the cost scan in (axis, bin) order with a strict <,
the leaf decision of a group of at most two triangles, the object median by (centre, id) from depth 22 and wherever SAH
finds no split.  Every decision is taken from order-independent quantities in binary32, in the builders' operation
order, so the tree is a function of the triangle set.  Needs no GPU.  Used to predict node count and depth, and to explain
a mismatch between two trees: `child_refs` and `leaf_order` are the arrays rtpt_debug_bvh_topology reads back (leaf order up
to the order of the two triangles inside a two-triangle leaf).

    python scripts/sah_restate.py scene.bin        # n x 9 float32 world-space triangles: prints nodes, depth
"""
import sys

import numpy as np

F32 = np.float32
BINS, MIN_LEAF, MAX_LEAF, NODE_COST, MAX_DEPTH = 32, 1, 2, F32(1.5), 48
FLT_MAX = np.finfo(F32).max
EMPTY, LEAF = 0xFFFFFFFF, 0x80000000


def pair_ok(tris):
    t = tris.reshape(-1, 9).view(np.uint32)
    if len(t) < 2 or len(t) % 2:
        return False
    a, b = t[0::2], t[1::2]
    return bool((a[:, :3] == b[:, :3]).all() and (a[:, 6:9] == b[:, 3:6]).all())


def half_area(mn, mx):
    """Box::half_area, operation for operation, on rows of boxes"""
    with np.errstate(all="ignore"):
        d = (mx - mn).astype(F32)
        a = ((d[..., 0] * d[..., 1]).astype(F32) + (d[..., 1] * d[..., 2]).astype(F32)).astype(F32)
        a = (a + (d[..., 2] * d[..., 0]).astype(F32)).astype(F32)
    return np.where(d[..., 0] < 0, F32(0), a).astype(F32)


def bin_of(c, mn, scale):
    with np.errstate(all="ignore"):
        x = ((c - mn).astype(F32) * scale).astype(F32)
    return np.clip(np.nan_to_num(x, nan=0.0, posinf=BINS, neginf=0).astype(np.int64), 0, BINS - 1)


class Tree:
    """nodes in pre-order (the order in which the host allocates them): child_refs[i] = (left, right) reference of node i,
    leaf_order = triangle ids in leaf-slot order, depth = level of the deepest leaf (the root pair's children at 1),
    median_at = (depth, primitives) of every range that was split at the object median"""

    def __init__(self, tris, pairs=None):
        tris = np.ascontiguousarray(tris, F32).reshape(-1, 9)
        n = len(tris)
        self.w = w = 2 if ((pair_ok(tris) if pairs is None else pairs) and n >= 2 and n % 2 == 0) else 1
        v = tris.reshape(-1, 3 * w, 3)
        self.mn, self.mx = v.min(1), v.max(1)
        self.c = (F32(0.5) * (self.mn + self.mx).astype(F32)).astype(F32)
        self.perm = np.arange(n // w)
        self.refs, self.first, self.last = [], [], []
        self.depth = 0
        self.median_splits = 0
        self.median_at = []  # (depth, primitives) of every range split at the object median, in pre-order
        if n <= MAX_LEAF:
            self.refs.append([LEAF | (n - 1), EMPTY])
            self.first.append(0), self.last.append(n // w - 1)
            return
        # explicit stack instead of the host's recursion; the right subtree waits while the left one is numbered
        stack = [(0, n // w, 0, None, 0)]
        while stack:
            lo, hi, depth, parent, side = stack.pop()
            ref = self._build(lo, hi, depth, stack)
            if parent is not None:
                self.refs[parent][side] = ref

    def _leaf(self, lo, hi):
        return LEAF | ((lo * self.w) << 2) | ((hi - lo) * self.w - 1)

    def _build(self, lo, hi, depth, stack):
        self.depth = max(self.depth, depth)
        w, n = self.w, (hi - lo) * self.w
        if hi - lo == 1 or n <= MIN_LEAF:
            return self._leaf(lo, hi)
        may_leaf = n <= MAX_LEAF
        p = self.perm[lo:hi]
        c, mn, mx = self.c[p], self.mn[p], self.mx[p]
        cmn, cmx = c.min(0), c.max(0)
        bmn, bmx = mn.min(0), mx.max(0)
        median = depth >= MAX_DEPTH - 26
        if median and may_leaf:
            return self._leaf(lo, hi)
        mid = lo
        if not median:
            best_cost, best_axis, best_split = FLT_MAX, -1, -1
            for a in range(3):
                with np.errstate(all="ignore"):
                    ext = F32(cmx[a] - cmn[a])
                    if not ext > 0:
                        continue
                    scale = F32(F32(BINS) / ext)
                b = bin_of(c[:, a], cmn[a], scale)
                bin_mn = np.full((BINS, 3), FLT_MAX, F32)
                bin_mx = np.full((BINS, 3), -FLT_MAX, F32)
                np.minimum.at(bin_mn, b, mn)
                np.maximum.at(bin_mx, b, mx)
                cnt = np.bincount(b, minlength=BINS) * w
                # suffix from bin 31 down to 1, prefix from bin 0 up to 30
                r_mn, r_mx = np.minimum.accumulate(bin_mn[::-1], 0)[::-1], np.maximum.accumulate(bin_mx[::-1], 0)[::-1]
                l_mn, l_mx = np.minimum.accumulate(bin_mn, 0), np.maximum.accumulate(bin_mx, 0)
                r_cnt, l_cnt = np.cumsum(cnt[::-1])[::-1], np.cumsum(cnt)
                with np.errstate(all="ignore"):
                    cost = ((half_area(l_mn[:-1], l_mx[:-1]) * l_cnt[:-1].astype(F32)).astype(F32) +
                            (half_area(r_mn[1:], r_mx[1:]) * r_cnt[1:].astype(F32)).astype(F32)).astype(F32)
                ok = (l_cnt[:-1] > 0) & (r_cnt[1:] > 0)
                for s in np.nonzero(ok)[0]:  # strict <: the first minimum in (axis, bin) order
                    if cost[s] < best_cost:
                        best_cost, best_axis, best_split = cost[s], a, int(s)
            bbh = half_area(bmn, bmx)
            with np.errstate(all="ignore"):
                if may_leaf and (best_axis < 0 or F32(F32(NODE_COST * bbh) + best_cost) >= F32(F32(n) * bbh)):
                    return self._leaf(lo, hi)
            if best_axis >= 0:
                with np.errstate(all="ignore"):
                    scale = F32(F32(BINS) / F32(cmx[best_axis] - cmn[best_axis]))
                left = bin_of(c[:, best_axis], cmn[best_axis], scale) <= best_split
                self.perm[lo:hi] = np.concatenate([p[left], p[~left]])  # stable; only the two sets matter
                mid = lo + int(left.sum())
        if mid == lo or mid == hi:
            ext = (cmx - cmn).astype(F32)
            axis, best = 0, F32(-1)
            for a in range(3):
                if ext[a] > best:
                    best, axis = ext[a], a
            key = c[:, axis] + F32(0)  # -0 and +0 compare equal
            self.perm[lo:hi] = p[np.lexsort((p, key))]
            mid = lo + (hi - lo) // 2
            self.median_splits += 1
            self.median_at.append((depth, hi - lo))
        me = len(self.refs)
        self.refs.append([None, None])
        self.first.append(lo), self.last.append(hi - 1)
        stack.append((mid, hi, depth + 1, me, 1))
        stack.append((lo, mid, depth + 1, me, 0))
        return me

    def n_nodes(self):
        return len(self.refs)

    @property
    def child_refs(self):
        return np.array(self.refs, np.uint32).reshape(-1, 2)

    @property
    def leaf_order(self):
        return (self.perm[:, None] * self.w + np.arange(self.w)[None, :]).reshape(-1).astype(np.uint32)


def canonical_leaf_order(child_refs, leaf_order):
    """leaf_order with the ids inside every leaf sorted: what two equal trees agree on (the order inside a two-triangle
    leaf of a triangle-mode tree is the partition's, which is not part of the tree)"""
    out = np.array(leaf_order, np.uint32)
    refs = np.asarray(child_refs, np.uint32).reshape(-1)
    refs = refs[(refs != EMPTY) & ((refs & LEAF) != 0)]
    first, cnt = (refs & 0x7FFFFFFF) >> 2, (refs & 3) + 1
    for f in first[cnt == 2]:
        out[f:f + 2] = np.sort(out[f:f + 2])
    return out


if __name__ == "__main__":
    t = Tree(np.fromfile(sys.argv[1], F32).reshape(-1, 9))
    print(f"primitives {len(t.perm)} ({'fan pairs' if t.w == 2 else 'triangles'}), nodes {t.n_nodes()}, depth {t.depth}, "
          f"median splits {t.median_splits}")
