"""Seeded generators of adversarial inputs for the a-trous filter kernels (numpy only; no fixture, no GPU): triangle soups
with degenerate members, id planes that read every entry of the id-pair table, colour / depth planes of six numeric
classes and the inputs of the final pass (world positions, an unrelated previous LUT, history, gradient, previous ids,
previous moments).  tests/test_filter_planes_cpu.py checks what is claimed here; tests/test_filter_planes_gpu.py feeds
the planes to the HIP kernels through rtpt_set_plane and to the oracle.

Every id a generator returns lies in [0, T] and the generators assert it: the kernels index their per-id tables
unguarded."""
from functools import lru_cache

import numpy as np

F32 = np.float32
T_VALUES = (1, 40, 63, 64, 100)
SHAPES = ((1, 1), (7, 3), (65, 7), (130, 33), (70, 37))      # (W, H)
CLASSES = ("bounded", "wide", "overflow", "subnormal", "planted", "flat")
ID_KINDS = ("random", "pairs_h", "pairs_v", "blocks")

# ids (triangle index + 1) of the special members of a soup with T >= 40
ID_TWO_EQUAL, ID_COLLINEAR, ID_POINT, ID_FRONT, ID_BACK, ID_TILT_A, ID_TILT_B = 1, 2, 3, 4, 5, 6, 7
# ids whose PREVIOUS triangle (lut_prev) is special, T >= 40
ID_PREV_HUGE_POS, ID_PREV_HUGE_NEG, ID_PREV_POINT, ID_PREV_TWO_EQUAL = 8, 9, 10, 11


def _rng(*key):
    return np.random.default_rng([int(k) if isinstance(k, (int, np.integer)) else _seed_of(str(k)) for k in key])


def _seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def check_ids(ids, T):
    ids = np.asarray(ids)
    assert ids.dtype == np.uint32 and ids.size and int(ids.max()) <= T, "an id above T must never reach a kernel"
    return ids


# ------------------------------------------------------------------------------------------ scenes
@lru_cache(maxsize=None)
def soup(T, seed=0):
    """[T, 9] float32 triangles.  With T >= 40 the first seven are (ids 1..7): two equal vertices (b == c: the cross
    product is the rounding residue of its fma form), three collinear vertices, three identical vertices (cross exactly
    0, normal NaN, self weight 0), two coplanar triangles of opposite winding (dot -1, clamped to 0) and two triangles
    whose normals differ by about 1e-4 rad (dot just under 1, where x^128 is steep)."""
    rng = _rng(11, T, seed)
    tris = rng.uniform(-2.0, 2.0, (T, 3, 3)).astype(F32)
    if T >= 40:
        a, b = tris[0, 0], tris[0, 1]
        tris[0] = np.stack([a, b, b])
        a, e = tris[1, 0], (tris[1, 1] * F32(0.37)).astype(F32)
        tris[1] = np.stack([a, (a + e).astype(F32), (a + F32(2) * e).astype(F32)])
        tris[2] = np.stack([tris[2, 0]] * 3)
        tris[4] = tris[3][[0, 2, 1]]
        a, b, c = tris[5].astype(np.float64)
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        foot = a + (b - a) * np.dot(c - a, b - a) / np.dot(b - a, b - a)
        tris[6] = np.stack([a, b, c + 1e-4 * np.linalg.norm(c - foot) * n]).astype(F32)   # c turned about the edge ab
    tris = np.ascontiguousarray(tris.reshape(T, 9))
    tris.setflags(write=False)
    return tris


# ids of a cone soup whose pair weight is not an ordinary one: rounding-residue or NaN normals, and the back face
CONE_ODD_IDS = (ID_TWO_EQUAL, ID_COLLINEAR, ID_POINT, ID_BACK)


@lru_cache(maxsize=None)
def cone_soup(T, seed=0):
    """[T, 9] float32 triangles for the pair-table planes: the degenerate members of soup() (ids 1..3), the back face of
    id 4 (id 5) — and every other normal inside a cone of 4 degrees about +z (id 0's normal), each with its own tilt
    (a sunflower spiral), so that max(0, n_p . n_q)^128 is a distinct weight between 0.2 and 1 for every pair: a wrong,
    unwritten or mis-staged table entry changes a pixel.  Ids 6 and 7 differ by about 1e-4 rad as in soup()."""
    assert T >= 40
    rng = _rng(17, T, seed)
    tris = np.array(soup(T, seed)).reshape(T, 3, 3).astype(np.float64)
    for t in range(T):
        if t + 1 in (ID_TWO_EQUAL, ID_COLLINEAR, ID_POINT):
            continue
        th = np.radians(4.0) * np.sqrt((t + 0.5) / T)
        ph = 2.399963229728653 * t
        if t + 1 == ID_TILT_B:
            th, ph = np.radians(4.0) * np.sqrt((ID_TILT_A - 0.5) / T) + 1e-4, 2.399963229728653 * (ID_TILT_A - 1)
        n = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
        u = np.cross(n, [0.0, 1.0, 0.0])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        a = rng.uniform(0.0, 2.0 * np.pi)
        e1 = rng.uniform(0.5, 1.5) * (np.cos(a) * u + np.sin(a) * v)
        e2 = rng.uniform(0.5, 1.5) * (-np.sin(a) * u + np.cos(a) * v)      # e1 x e2 is along +n (u x v = n ... checked on the CPU)
        c = rng.uniform(-1.0, 1.0, 3)
        tris[t] = np.stack([c, c + e1, c + e2])
    tris[ID_BACK - 1] = tris[ID_FRONT - 1][[0, 2, 1]]
    tris = np.ascontiguousarray(tris.reshape(T, 9), F32)
    tris.setflags(write=False)
    return tris


def pair_weights_numpy(tris):
    """[(T+1), (T+1)] float32: max(0, n_p . n_q)^128 from float32 normals, seven squarings (NaN normals weigh 0)"""
    n = normals_numpy(F32, tris)
    with np.errstate(invalid="ignore"):
        d = (n[:, None, :] * n[None, :, :]).sum(-1).astype(F32)
    w = np.where(d > 0, d, F32(0)).astype(F32)
    for _ in range(7):
        w = (w * w).astype(F32)
    return w


@lru_cache(maxsize=None)
def facing_grid(nx=10, ny=5, seed=0):
    """nx x ny quads (2 nx ny triangles, 100 by default) in front of a camera at the origin that looks down -z: every
    quad is tilted by its own small angles, so neighbouring pixels of different quads carry different normals"""
    rng = _rng(12, nx, ny, seed)
    tris = []
    xs = np.linspace(-1.0, 1.0, nx + 1)
    ys = np.linspace(-0.5, 0.5, ny + 1)
    for j in range(ny):
        for i in range(nx):
            tx, ty = rng.uniform(-0.3, 0.3, 2)
            def P(x, y):
                cx, cy = 0.5 * (xs[i] + xs[i + 1]), 0.5 * (ys[j] + ys[j + 1])
                return (x, y, -4.0 + tx * (x - cx) + ty * (y - cy))
            p00, p10, p11, p01 = P(xs[i], ys[j]), P(xs[i + 1], ys[j]), P(xs[i + 1], ys[j + 1]), P(xs[i], ys[j + 1])
            tris.append(p00 + p10 + p11)
            tris.append(p00 + p11 + p01)
    tris = np.ascontiguousarray(np.array(tris, F32))
    tris.setflags(write=False)
    return tris


def mesh_of(tris):
    """(xyz [3T, 3], idx [T, 3]) for rtpt_scene_upload: every triangle keeps its own three vertices, in order"""
    xyz = np.ascontiguousarray(np.asarray(tris, F32).reshape(-1, 3))
    idx = np.arange(len(xyz), dtype=np.uint32).reshape(-1, 3)
    return xyz, idx


# ------------------------------------------------------------------------------------------ id planes
def _pair_list(T):
    """every unordered pair {p, q} of ids in [0, T], p <= q: a tap reads the table at [centre][neighbour], so two
    adjacent pixels p, q read both [p][q] (centre p) and [q][p] (centre q)"""
    return [(p, q) for p in range(T + 1) for q in range(p, T + 1)]


@lru_cache(maxsize=None)
def id_plane(kind, T, W, H, seed=0):
    """[H, W] uint32.  random: per-pixel ids.  pairs_h / pairs_v: the pair list laid out as horizontally / vertically
    adjacent pixels (as many pairs as the frame holds, in list order, then random ids).  blocks: 4 x 5 pixel blocks."""
    rng = _rng(13, kind, T, W, H, seed)
    ids = rng.integers(0, T + 1, (H, W), dtype=np.uint32)
    if kind == "blocks":
        small = rng.integers(0, T + 1, ((H + 4) // 5, (W + 3) // 4), dtype=np.uint32)
        ids = np.ascontiguousarray(np.repeat(np.repeat(small, 5, 0), 4, 1)[:H, :W])
    elif kind in ("pairs_h", "pairs_v"):
        pairs = _pair_list(T)
        if kind == "pairs_h":
            slots = [(y, x) for y in range(H) for x in range(0, W - 1, 2)]
            for (p, q), (y, x) in zip(pairs, slots):
                ids[y, x], ids[y, x + 1] = p, q
        else:
            slots = [(y, x) for y in range(0, H - 1, 2) for x in range(W)]
            for (p, q), (y, x) in zip(pairs, slots):
                ids[y, x], ids[y + 1, x] = p, q
    else:
        assert kind == "random", kind
    ids = np.ascontiguousarray(ids, np.uint32)
    check_ids(ids, T)
    ids.setflags(write=False)
    return ids


def without_point(ids):
    """the plane with the ids of the all-identical-vertex triangle (every weight 0, the pixel 0 / 0 = NaN, and the NaN
    spreads by one stride per iteration) replaced by id 0: what the comparisons within a tolerance run on"""
    ids = np.array(ids, np.uint32)
    ids[ids == ID_POINT] = 0
    return ids


def pairs_read(ids, T, horizontal):
    """[(T+1), (T+1)] bool: entry [p][q] is read by some stride-1 tap of this plane along the given axis"""
    ids = np.asarray(ids).astype(np.int64)
    a, b = (ids[:, :-1], ids[:, 1:]) if horizontal else (ids[:-1, :], ids[1:, :])
    seen = np.zeros((T + 1, T + 1), bool)
    seen[a.ravel(), b.ravel()] = True
    seen[b.ravel(), a.ravel()] = True
    return seen


# ------------------------------------------------------------------------------------------ colour and depth
def planted_positions(ids, T):
    """where the planted class puts its non-finite pixels: a corner, the top and the left edge, the interior, and (when
    the plane has one) an interior pixel of the all-identical-vertex triangle.  [(y, x, value)]"""
    H, W = ids.shape
    pos = [(0, 0, np.nan), (H - 1, W - 1, np.inf), (0, W // 2, -np.inf), (H // 2, 0, np.nan),
           (H // 2, W // 2, np.inf), (H // 3, (2 * W) // 3, -np.inf), ((2 * H) // 3, W // 3, np.nan)]
    if T >= ID_POINT:
        ys, xs = np.nonzero(np.asarray(ids)[1:-1, 1:-1] == ID_POINT) if H > 2 and W > 2 else ((), ())
        if len(ys):
            pos.append((int(ys[0]) + 1, int(xs[0]) + 1, np.nan))
            pos.append((int(ys[-1]) + 1, int(xs[-1]) + 1, np.inf))
    return pos


def colour_depth(cls, ids, T, seed=0):
    """(image [H, W, 4] float32 with alpha 0, depth [H, W] float32) of one class"""
    H, W = ids.shape
    rng = _rng(14, _seed_of(cls), T, W, H, seed)
    img = np.zeros((H, W, 4), F32)
    if cls in ("bounded", "planted"):
        img[..., :3] = rng.uniform(0.0, 4.0, (H, W, 3))
        depth = rng.uniform(0.0, 8.0, (H, W))
    elif cls == "wide":
        img[..., :3] = 10.0 ** rng.uniform(-30.0, 18.0, (H, W, 3))
        depth = 10.0 ** rng.uniform(-6.0, 6.0, (H, W))          # steep: neighbours differ by orders of magnitude
    elif cls == "overflow":
        img[..., :3] = 10.0 ** rng.uniform(10.0, 26.0, (H, W, 3))    # dot(dc, dc) ~ 1e52 overflows binary32
        depth = 10.0 ** rng.uniform(0.0, 30.0, (H, W))
    elif cls == "subnormal":
        img[..., :3] = 1e-40 * rng.uniform(0.1, 10.0, (H, W, 3))
        depth = 1e-40 * rng.uniform(0.1, 10.0, (H, W))
    elif cls == "flat":
        img[..., :3] = np.array([0.7, 1.3, 2.1], F32)
        depth = np.full((H, W), 3.0)
    else:
        raise ValueError(cls)
    depth = np.ascontiguousarray(depth, F32)
    if cls == "planted":
        for n, (y, x, v) in enumerate(planted_positions(ids, T)):
            if n % 3 == 2:
                depth[y, x] = v                    # every third one in the depth plane
            else:
                img[y, x, n % 3] = v               # one channel: the others must turn NaN with it
    return img, depth


# ------------------------------------------------------------------------------------------ final-pass inputs
def prev_matrices():
    """(viewPrev, projPrev), column-major float32[16], chosen by the tests: a small turn about z plus a shift, and a
    projection with a perspective row (w = 1 + 0.1 z) — screen x, y in [-1, 1] cover about a third of where the
    reprojected points fall, so pixels land inside the frame and outside it on every side"""
    c, s = np.cos(0.05), np.sin(0.05)
    view = np.array([[c, -s, 0, 0.1], [s, c, 0, -0.05], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
    proj = np.array([[0.6, 0, 0, 0], [0, 0.7, 0, 0], [0, 0, 1, 0], [0, 0, 0.1, 1]], np.float64)
    return np.ascontiguousarray(view.T.ravel(), F32), np.ascontiguousarray(proj.T.ravel(), F32)


def final_inputs(ids, T, seed=0):
    """dict of the planes the final pass (and the extension modes) read besides colour, depth and ids.
    lut_prev [(T+1), 12] is unrelated to the scene; with T >= 40 the previous triangles of ids 8..11 are: huge and
    positive in x, y (1e9, w ~ 1e-5: the pixel saturates at INT_MAX), huge and negative (INT_MIN), a point (area exactly 0: barycentrics
    0/0, the pixel is f2i(NaN) = 0) and a needle (two equal vertices: the area is rounding residue)."""
    H, W = ids.shape
    rng = _rng(15, T, W, H, seed)
    lut_prev = np.zeros((T + 1, 3, 4), F32)
    lut_prev[1:, :, :3] = rng.uniform(-1.5, 1.5, (T, 3, 3))
    if T >= 40:
        big = rng.uniform(0.5, 1.5, (3, 3))
        big[:, :2] *= 1e9        # (areas ~1e18 and their squares stay finite in binary32)
        big[:, 2] = -9.9999      # w = 1 + 0.1 z ~ 1e-5: x / w ~ 1e14 saturates whatever the frame width
        lut_prev[ID_PREV_HUGE_POS, :, :3] = big
        big = big.copy()
        big[:, :2] *= -1.0
        lut_prev[ID_PREV_HUGE_NEG, :, :3] = big
        lut_prev[ID_PREV_POINT, :, :3] = lut_prev[ID_PREV_POINT, 0, :3]
        lut_prev[ID_PREV_TWO_EQUAL, 2, :3] = lut_prev[ID_PREV_TWO_EQUAL, 1, :3]
    worldpos = np.zeros((H, W, 4), F32)
    worldpos[..., :3] = rng.uniform(-1.5, 1.5, (H, W, 3))
    history = np.zeros((H, W, 4), F32)
    history[..., :3] = rng.uniform(0.0, 4.0, (H, W, 3))
    gradient = np.zeros((H, W, 4), F32)
    gradient[..., 0] = rng.choice(np.array([0.0, 1.0, -0.5, 2.5, np.nan, 0.25, 0.75], F32), (H, W))
    gradient[..., 1:3] = rng.uniform(0.0, 1.0, (H, W, 2))
    moments_prev = np.zeros((H, W, 4), F32)
    m1 = rng.uniform(0.0, 2.0, (H, W))
    moments_prev[..., 0] = m1
    moments_prev[..., 1] = m1 * m1 + rng.uniform(0.0, 1.0, (H, W))
    moments_prev[..., 2] = rng.choice(np.array([0, 1, 2, 3, 4, 5, 100, 253, 254, 255, 256, 300], F32), (H, W))
    moments_prev[..., 3] = rng.uniform(0.0, 1.0, (H, W))
    view_prev, proj_prev = prev_matrices()
    return dict(lut_prev=np.ascontiguousarray(lut_prev.reshape(T + 1, 12)), worldpos=worldpos, history=history, gradient=gradient,
                moments_prev=moments_prev, view_prev=view_prev, proj_prev=proj_prev)


def prev_ids(ids, T, prev_pixel, seed=0):
    """[H, W] uint32 previous-frame ids: random, but at the reprojected pixel of every second pixel that lands inside
    the frame the pixel's own id (so the disocclusion test and the moment history take both branches)"""
    H, W = ids.shape
    rng = _rng(16, T, W, H, seed)
    pv = rng.integers(0, T + 1, (H, W), dtype=np.uint32)
    px, py = prev_pixel[..., 0], prev_pixel[..., 1]
    inside = (px >= 0) & (px < W) & (py >= 0) & (py < H)
    take = inside & (rng.random((H, W)) < 0.5)
    pv[py[take], px[take]] = np.asarray(ids)[take]
    return check_ids(np.ascontiguousarray(pv), T)


def landing_classes(prev_pixel, W, H):
    """names of the landing classes a reprojected-pixel plane [H, W, 2] contains"""
    px, py = prev_pixel[..., 0].astype(np.int64), prev_pixel[..., 1].astype(np.int64)
    out = set()
    big = 1 << 30
    if ((px >= 0) & (px < W) & (py >= 0) & (py < H)).any():
        out.add("inside")
    if ((px < 0) & (px > -big)).any():
        out.add("left")
    if ((px >= W) & (px < big)).any():
        out.add("right")
    if ((py < 0) & (py > -big)).any():
        out.add("above")
    if ((py >= H) & (py < big)).any():
        out.add("below")
    if (px == -(1 << 31)).any() or (py == -(1 << 31)).any():
        out.add("int_min")
    if (px == (1 << 31) - 1).any() or (py == (1 << 31) - 1).any():
        out.add("int_max")
    return out


# ------------------------------------------------------------------------------------------ float64 restatement
def normals_numpy(dtype, tris):
    """[(T+1), 3] per-id unit normals normalize(cross(b - a, c - a)) at `dtype`; id 0: (0, 0, 1)"""
    v = np.asarray(tris, dtype).reshape(-1, 3, 3)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = (n / np.sqrt((n * n).sum(-1, keepdims=True))).astype(dtype)
    return np.concatenate([np.array([[0, 0, 1]], dtype), n])


def atrous_once_numpy(dtype, img, depth, ids, normals, stride, sigma_n=128, sigma_z=1.0, sigma_l=4.0):
    """one non-final iteration of the plain filter (temporalFiltering.comp.glsl:118-155) in numpy at `dtype`: 3 x 3 taps at
    `stride`, clamped to the frame, w = max(0, n_p . n_q)^sigma_n * exp(-|dz| / sigma_z) * exp(-|dc| / sigma_l), h = 1/9.
    normals: [(T+1), 3] per-id unit normals (id 0: (0, 0, 1)).  Returns [H, W, 3]."""
    H, W = ids.shape
    c = np.asarray(img[..., :3], dtype)
    d = np.asarray(depth, dtype)
    n = np.asarray(normals, dtype)[np.asarray(ids, np.int64)]
    num = np.zeros((H, W, 3), dtype)
    den = np.zeros((H, W), dtype)
    yy, xx = np.mgrid[0:H, 0:W]
    h = dtype(1) / dtype(9)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            qx = np.clip(xx + i * stride, 0, W - 1)
            qy = np.clip(yy + j * stride, 0, H - 1)
            cq, dq, nq = c[qy, qx], d[qy, qx], n[qy, qx]
            wn = np.maximum(dtype(0), (n * nq).sum(-1))
            assert sigma_n == 128
            for _ in range(7):                      # x^128 as seven squarings, the algorithm of the code under test
                wn = (wn * wn).astype(dtype)
            wd = np.exp(-np.abs(d - dq) / dtype(sigma_z))
            wl = np.exp(-np.sqrt(((c - cq) ** 2).sum(-1)) / dtype(sigma_l))
            hw = (h * ((wn * wd) * wl)).astype(dtype)
            num += hw[..., None] * cq
            den += hw
    return num / den[..., None]


# ------------------------------------------------------------------------------------------ comparison
def same_bits(got, want, tag):
    """NaN positions equal, every other value equal as bits; no pixel left out"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, tag
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), (tag, np.argwhere(got != want)[:4].tolist())
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (tag, "NaN positions", int(gn.sum()), int(wn.sum()), np.argwhere(gn != wn)[:4].tolist())
    g, w = np.where(gn, np.float32(0), got).view(np.uint32), np.where(wn, np.float32(0), want).view(np.uint32)
    bad = np.argwhere(g != w)
    assert not len(bad), (tag, len(bad), bad[:4].tolist(), [(float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]])
