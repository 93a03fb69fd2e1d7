"""numpy restatement of the device LBVH builder (csrc/bvh_build.hip): primitive centres, 63-bit Morton keys, the stable
sort, the radix tree over the augmented keys (ties split by sorted position) and its pre-order numbering.  Needs no GPU.
Top-down splits where the device runs Karras' per-node searches: an independent statement, and the reference the device's
tree is held to array for array (tests/test_device_tree_gpu.py; tests/test_device_tree_cpu.py holds this file to the
definition of the radix tree).  Also used to predict depths (which scenes fall back to the host builder) and to explain
a traversal result: `path_to` gives the nodes above a triangle, `first_missed` the first of them whose padded box a ray
does not pass through.

    python scripts/lbvh_restate.py scene.bin        # n x 9 float32 world-space triangles: prints nodes, depth
"""
import sys

import numpy as np

F32 = np.float32
LEAF, EMPTY = 0x80000000, 0xFFFFFFFF


def pair_ok(tris):
    t = tris.reshape(-1, 9).view(np.uint32)
    if len(t) < 2 or len(t) % 2:
        return False
    a, b = t[0::2], t[1::2]
    return bool((a[:, :3] == b[:, :3]).all() and (a[:, 6:9] == b[:, 3:6]).all())


def morton_keys(tris, w):
    v = tris.reshape(-1, 3 * w, 3).astype(F32)
    mn, mx = v.min(1), v.max(1)
    c = (F32(0.5) * mn + F32(0.5) * mx).astype(F32)
    lo, hi = c.min(0).astype(np.float64), c.max(0).astype(np.float64)
    ext = hi - lo
    with np.errstate(all="ignore"):
        x = np.where(ext > 0, (c.astype(np.float64) - lo) / np.where(ext > 0, ext, 1.0) * 2097152.0, 0.0)
    x = np.where(x >= 0, x, 0.0)
    q = np.minimum(x, 2097151.0).astype(np.uint64)

    def spread(u):
        u = u & np.uint64(0x1FFFFF)
        for s, m in ((32, 0x001F00000000FFFF), (16, 0x001F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3),
                     (2, 0x1249249249249249)):
            u = (u | (u << np.uint64(s))) & np.uint64(m)
        return u

    return (spread(q[:, 0]) << np.uint64(2)) | (spread(q[:, 1]) << np.uint64(1)) | spread(q[:, 2])


class Tree:
    """nodes in pre-order: left / right = ("leaf", sorted position) or ("node", index); first / last = range of sorted positions.
    `child_refs()` and `leaf_order()` are the arrays rtpt_debug_bvh_topology reads back from a device-built tree, `depth` is
    the depth of rtpt_scene_build_info: the level of the deepest leaf, the root pair's children at 1 (0 for one primitive)"""

    def __init__(self, tris, pairs=None, keys=None):
        """`keys`: one 64-bit key per primitive instead of morton_keys' — the tree a builder with other keys would make"""
        tris = np.ascontiguousarray(tris, F32).reshape(-1, 9)
        self.tris = tris
        self.w = 2 if (pair_ok(tris) if pairs is None else pairs) else 1
        keys = morton_keys(tris, self.w) if keys is None else np.asarray(keys, np.uint64)
        self.order = np.argsort(keys, kind="stable")  # sorted position -> primitive
        k = [int(x) for x in keys[self.order]]
        n = len(k)
        self.left, self.right, self.first, self.last, self.level = [], [], [], [], []
        self.depth = 0
        if n == 1:
            self.left, self.right, self.first, self.last, self.level = [("leaf", 0)], [None], [0], [0], [0]
            return
        aug = [(k[i] << 32) | i for i in range(n)]  # the augmented key: unique
        stack = [(0, n - 1, None, 0, 0)]  # range, parent, side, level
        while stack:
            a, b, parent, side, lvl = stack.pop()
            me = len(self.left)
            self.left.append(None), self.right.append(None), self.first.append(a), self.last.append(b), self.level.append(lvl)
            self.depth = max(self.depth, lvl + 1)
            if parent is not None:
                (self.left if side == 0 else self.right)[parent] = ("node", me)
            top = (aug[a] ^ aug[b]).bit_length() - 1  # highest differing bit: the split is where it flips
            lo, hi = a, b
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if (aug[mid] >> top) & 1:
                    hi = mid
                else:
                    lo = mid
            g = lo  # last position with that bit clear
            # pre-order: the left subtree is numbered first — push right first
            if g + 1 == b:
                self.right[me] = ("leaf", b)
            else:
                stack.append((g + 1, b, me, 1, lvl + 1))
            if g == a:
                self.left[me] = ("leaf", a)
            else:
                stack.append((a, g, me, 0, lvl + 1))

    def n_nodes(self):
        return len(self.left)

    def child_refs(self):
        """[n_nodes, 2] uint32: an internal child is its pre-order index, a leaf bit 31 | (sorted position * w) << 2 | (w - 1);
        the absent right child of a one-primitive scene is 0xFFFFFFFF"""
        def ref(ch):
            if ch is None:
                return EMPTY
            return ch[1] if ch[0] == "node" else LEAF | ((ch[1] * self.w) << 2) | (self.w - 1)
        return np.array([[ref(l), ref(r)] for l, r in zip(self.left, self.right)], np.uint32).reshape(-1, 2)

    def leaf_order(self):
        """[n_triangles] uint32: slot sorted position * w + k holds triangle order[sorted position] * w + k"""
        return (self.order[:, None] * self.w + np.arange(self.w)[None, :]).reshape(-1).astype(np.uint32)

    def box(self, a, b):
        """unpadded binary32 box of sorted positions a..b"""
        prim = self.order[a:b + 1]
        v = self.tris.reshape(-1, 3 * self.w, 3)[prim].reshape(-1, 3)
        return v.min(0), v.max(0)

    def pad(self):
        v = self.tris.reshape(-1, 3)
        mn, mx = v.min(0), v.max(0)
        return F32(1e-5) * max(F32(np.sqrt(((mx - mn).astype(F32) ** 2).sum(dtype=F32))), np.abs(np.concatenate([mn, mx])).max())

    def path_to(self, tri):
        """[(node, side, (first, last) of that child)] from the root down to the leaf holding triangle `tri`"""
        pos = int(np.nonzero(self.order == tri // self.w)[0][0])
        out, node = [], 0
        while True:
            l = self.left[node]
            lrange = (l[1], l[1]) if l[0] == "leaf" else (self.first[l[1]], self.last[l[1]])
            side = 0 if lrange[0] <= pos <= lrange[1] else 1
            ch = self.right[node] if side else l
            rng = (ch[1], ch[1]) if ch[0] == "leaf" else (self.first[ch[1]], self.last[ch[1]])
            out.append((node, side, rng))
            if ch[0] == "leaf":
                return out
            node = ch[1]

    def first_missed(self, tri, o, d, t_hit):
        """the first child box above `tri` that the ray o + t d, 0 <= t <= t_hit, misses in exact arithmetic, with how far
        (in paddings) the ray stays outside it; None when it passes through all of them"""
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        pad = float(self.pad())
        for node, side, (a, b) in self.path_to(tri):
            mn, mx = (x.astype(np.float64) for x in self.box(a, b))
            t0, t1 = 0.0, float(t_hit)
            gap = 0.0
            for ax in range(3):
                if d[ax] == 0.0:
                    if not (mn[ax] - pad <= o[ax] <= mx[ax] + pad):
                        gap = max(gap, max(mn[ax] - o[ax], o[ax] - mx[ax]) / pad)
                        t1 = -1.0
                    continue
                ta, tb = (mn[ax] - pad - o[ax]) / d[ax], (mx[ax] + pad - o[ax]) / d[ax]
                t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
            if t0 > t1:
                p = o + d * float(t_hit)
                out = np.maximum(np.maximum(mn - p, p - mx), 0.0).max() / pad
                return dict(node=node, side="right" if side else "left", level=self.level[node], range=(a, b),
                            hit_point_outside_box_by_pads=float(max(out, gap)))
        return None


if __name__ == "__main__":
    t = Tree(np.fromfile(sys.argv[1], F32).reshape(-1, 9))
    print(f"primitives {len(t.order)} ({'fan pairs' if t.w == 2 else 'triangles'}), nodes {t.n_nodes()}, depth {t.depth}")
