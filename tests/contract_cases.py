"""Seeded operands for the numerics-contract functions, one generator per function of the table of include/rtpt.h
(rtpt_selftest_contract / oracle_contract_array), numpy only.

    words, cls = cases("dot", n)        # words [n, n_in] uint32 (raw bit patterns), cls [n] uint8 (index into CLASSES)

Every function gets the same classes of operand, in contiguous blocks whose sizes are fixed fractions of n (WEIGHTS):

    ordinary      magnitudes 2^-8 .. 2^8, either sign
    anybits       arbitrary 32-bit patterns
    scaled_small  ordinary operands, all scaled by one power of two in 2^-70 .. 2^-60 (squares and products land in or
                  below the subnormals)
    scaled_big    ... by 2^60 .. 2^66 (a dot product overflows)
    specials      ordinary operands with ONE position replaced by one of SPECIALS, every (position, special) in turn
    structural    what the shape of the function makes interesting: equal and nearly parallel vectors, degenerate triangles,
                  thresholds, every exponent
    onscreen      reproject_pixel only: a camera in front of the triangle, so that most items land inside the frame

Functions with a stated domain keep to it in every class (sincos2pi: [0, 1]; log_: positive finite) and integer operands
(powi's n, the RNG's words, reproject_pixel's W, H, id, x, y) have their own values; cases() says which.  The fractions are
chosen so that at most a quarter of a function's items have a NaN in the result (tests/test_contract_cpu.py asserts it on the
oracle): the barycentric functions, where overflow and underflow of an area both end in 0/0 or inf/inf, get more ordinary
items for that reason."""
import numpy as np

F32 = np.float32
U32 = np.uint32

FNS = ("dot", "cross", "length", "normalize", "powi", "f2i", "minmax", "rng_seed", "rng_next_skip", "sincos2pi", "log", "exp",
       "mat_row_point", "div", "div2", "tri_area", "bary_coords", "bary_coords_at", "bary_mix", "reproject_pixel",
       "ray_hits_light", "sky_color", "hit_barycentrics")
WORDS = ((6, 1), (6, 3), (3, 1), (3, 3), (2, 1), (1, 1), (2, 2), (4, 1), (1, 3), (1, 2), (1, 1), (1, 1), (19, 4), (2, 1), (3, 2),
         (9, 1), (12, 3), (13, 3), (12, 3), (36, 2), (10, 1), (3, 3), (3, 6))
# which output words are floats (compared with the NaN rule); the others are integers and always exact
FLOAT_OUT = {"f2i": (), "rng_seed": (), "rng_next_skip": (1,), "reproject_pixel": (), "ray_hits_light": ()}
CLASSES = ("ordinary", "anybits", "scaled_small", "scaled_big", "specials", "structural", "onscreen")
ORDINARY, ANYBITS, SCALED_SMALL, SCALED_BIG, SPECIALS_CLS, STRUCTURAL, ONSCREEN = range(7)

# +0, -0, +inf, -inf, NaN, 2^-149, the largest finite
SPECIALS = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x00000001, 0x7f7fffff], U32)
POWI_N = (1, 2, 3, 5, 127, 128, 255)
REPROJECT_WH = (1, 7, 65, 3840)

_DEFAULT_W = (0.40, 0.12, 0.08, 0.08, 0.16, 0.16, 0.0)
_BARY_W = (0.64, 0.06, 0.03, 0.03, 0.09, 0.15, 0.0)
WEIGHTS = {fn: _DEFAULT_W for fn in FNS}
for _fn in ("bary_coords", "bary_coords_at"):
    WEIGHTS[_fn] = _BARY_W
WEIGHTS["reproject_pixel"] = (0.20, 0.06, 0.03, 0.03, 0.13, 0.25, 0.30)


def fn_index(fn):
    return FNS.index(fn)


def float_out_words(fn):
    return FLOAT_OUT.get(fn, tuple(range(WORDS[fn_index(fn)][1])))


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def floats(w):
    return np.ascontiguousarray(w, U32).view(F32)


def is_nan_bits(w):
    return (np.asarray(w, U32) & U32(0x7fffffff)) > U32(0x7f800000)


def is_finite_bits(w):
    return (np.asarray(w, U32) & U32(0x7f800000)) != U32(0x7f800000)


def _ordinary(rng, shape, positive=False):
    m = np.exp2(rng.uniform(-8.0, 8.0, shape)).astype(F32)
    if not positive:
        m = np.where(rng.integers(0, 2, shape) == 1, -m, m).astype(F32)
    return m


def _anybits(rng, shape):
    return rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(U32)


def _scale(rng, x, lo, hi):
    """every operand of an item times ONE power of two 2^k, lo <= k <= hi (exact: a power of two and no overflow here)"""
    k = rng.integers(lo, hi + 1, (len(x),) + (1,) * (x.ndim - 1))
    return (x.astype(np.float64) * np.exp2(k.astype(np.float64))).astype(F32)


def _split(n, weights):
    counts = [int(n * w) for w in weights]
    counts[0] += n - sum(counts)
    return counts


def _cycle(rows, m):
    """m rows out of a list of structural rows, every one in turn"""
    rows = np.asarray(rows)
    return rows[np.arange(m) % len(rows)]


def _nextafter(x, up):
    x = F32(x)
    return np.nextafter(x, F32(np.inf) if up else F32(-np.inf), dtype=F32)


# ---------------------------------------------------------------------------------------------- float-operand functions
def _float_cases(rng, n, k, weights, structural, positive=False):
    """the six classes for a function of k float operands; structural(rng, m) -> [m, k] float32 or uint32 bits"""
    c = _split(n, weights)
    parts, cls = [], []
    parts.append(bits(_ordinary(rng, (c[0], k), positive)))
    any_ = _anybits(rng, (c[1], k))
    if positive:  # the positive finite patterns 1 .. 0x7f7fffff
        any_ = (any_ % U32(0x7f7fffff)) + U32(1)
    parts.append(any_)
    parts.append(bits(_scale(rng, _ordinary(rng, (c[2], k), positive), -70, -60)))
    parts.append(bits(_scale(rng, _ordinary(rng, (c[3], k), positive), 60, 66)))
    sp = bits(_ordinary(rng, (c[4], k), positive)).copy()
    j = np.arange(c[4])
    pool = SPECIALS if not positive else np.array([0x00000001, 0x7f7fffff, 0x00800000, 0x007fffff, 0x00800001, 0x3f800000, 0x3f800001], U32)
    sp[j, j % k] = pool[(j // k) % len(pool)]
    parts.append(sp)
    st = structural(rng, c[5])
    parts.append(st if st.dtype == U32 else bits(st))
    for i, p in enumerate(parts):
        cls.append(np.full(len(p), i, np.uint8))
    return np.concatenate(parts).astype(U32), np.concatenate(cls)


def _vec_pairs(rng, m):
    a = _ordinary(rng, (m, 3))
    near = (a * F32(1.0 + 2.0 ** -12)).astype(F32)
    z = np.zeros((m, 3), F32)
    rows = np.stack([np.hstack([a, a]), np.hstack([a, near]), np.hstack([near, a]), np.hstack([z, a]), np.hstack([a, z]),
                     np.hstack([z, z]), np.hstack([a, -a]), np.hstack([-z, a])], 1)  # [m, 8, 6]
    return rows[np.arange(m), np.arange(m) % 8].astype(F32)


def _vec_single(rng, m):
    a = _ordinary(rng, (m, 3))
    z = np.zeros((m, 3), F32)
    one = a.copy()
    one[:, 1:] = 0
    tiny = _scale(rng, a, -75, -75)
    sub = _scale(rng, a, -140, -135)
    huge = _scale(rng, a, 64, 64)
    edge = _scale(rng, a, 55, 56)  # squares around 2^127: some dot products overflow, some do not
    rows = np.stack([z, -z, one, tiny, sub, huge, edge, a], 1)
    return rows[np.arange(m), np.arange(m) % 8].astype(F32)


def _div_pairs(rng, m):
    a = _ordinary(rng, (m,))
    b = _ordinary(rng, (m,))
    z = np.zeros(m, F32)
    # the window of the short sequence is the exponent fields 65 .. 188: operands right at its ends
    ef = rng.choice(np.array([1, 63, 64, 65, 66, 187, 188, 189, 190, 253, 254], np.int64), (m, 2))
    man = _anybits(rng, (m, 2)) & U32(0x807fffff)
    edge = floats(man | (ef.astype(U32) << U32(23)))
    rows = np.stack([np.stack([a, a], 1), np.stack([a, (a * F32(1 + 2.0 ** -12)).astype(F32)], 1), np.stack([z, z], 1),
                     np.stack([a, z], 1), np.stack([a, -z], 1), np.stack([z, b], 1), edge, np.stack([edge[:, 0], b], 1),
                     np.stack([a, edge[:, 1]], 1)], 1)
    return rows[np.arange(m), np.arange(m) % 9].astype(F32)


def _div2_triples(rng, m):
    p = _div_pairs(rng, m)
    q = _div_pairs(rng, m)
    third = np.where((np.arange(m) % 2) == 0, q[:, 0], p[:, 0])
    return np.stack([p[:, 0], third, p[:, 1]], 1).astype(F32)


def _int_points(rng, shape, span=64):
    return rng.integers(-span, span + 1, shape).astype(F32)


def _degenerate_triangles(rng, m):
    """[m, 9]: two equal vertices, exactly collinear vertices (small integers: the arithmetic is exact), a point"""
    a = _int_points(rng, (m, 3))
    d = _int_points(rng, (m, 3), 8)
    s = rng.integers(-4, 5, (m, 1)).astype(F32)
    b = a + d
    eq_ab = np.hstack([a, a, b])
    eq_bc = np.hstack([a, b, b])
    eq_ac = np.hstack([a, b, a])
    col = np.hstack([a, b, a + s * d])
    pt = np.hstack([a, a, a])
    rows = np.stack([eq_ab, eq_bc, eq_ac, col, pt], 1)
    return rows[np.arange(m), np.arange(m) % 5].astype(F32)


def _tri_area_struct(rng, m):
    t = _degenerate_triangles(rng, m)
    o = _ordinary(rng, (m, 9))
    o[:, 3:6] = o[:, 0:3] * F32(1 + 2.0 ** -12)  # a sliver: b next to a
    return np.where((np.arange(m) % 4 == 3)[:, None], o, t).astype(F32)


def _np_area(a, b, c):
    n = np.cross((b - a).astype(np.float64), (c - a).astype(np.float64))
    return (np.sqrt((n * n).sum(-1)) * 0.5).astype(F32)


def _points_of_triangle(rng, a, b, c):
    """[m, 3] p for the barycentric functions: on a vertex, on an edge, inside, off the plane"""
    m = len(a)
    w = rng.dirichlet((1.0, 1.0, 1.0), m).astype(F32)
    inside = (w[:, :1] * a + w[:, 1:2] * b + w[:, 2:] * c).astype(F32)
    edge = ((a + b) * F32(0.5)).astype(F32)
    nrm = np.cross(b - a, c - a).astype(F32)
    off = (inside + nrm * F32(0.25)).astype(F32)
    rows = np.stack([a, b, c, edge, ((b + c) * F32(0.5)).astype(F32), inside, off, (a + (a - b)).astype(F32)], 1)
    return rows[np.arange(m), np.arange(m) % 8].astype(F32)


def _bary_struct(rng, m, with_area=False):
    tri = _ordinary(rng, (m, 9))
    ints = _int_points(rng, (m, 9), 16)  # integer triangles: p on a vertex or an edge midpoint is exact
    tri = np.where((np.arange(m) % 2 == 0)[:, None], tri, ints).astype(F32)
    deg = _degenerate_triangles(rng, m)
    use_deg = (np.arange(m) % 4 == 3)[:, None]  # a quarter of the structural items: area 0, so 0/0 and x/0
    tri = np.where(use_deg, deg, tri).astype(F32)
    a, b, c = tri[:, 0:3], tri[:, 3:6], tri[:, 6:9]
    p = _points_of_triangle(rng, a, b, c)
    cols = [p, tri]
    if with_area:
        cols.append(_np_area(a, b, c)[:, None])
    return np.hstack(cols).astype(F32)


def _bary_ordinary_fix(words, cls, with_area):
    """ordinary items: half keep an arbitrary p, half take a p in the triangle's plane; bary_coords_at gets the triangle's area"""
    f = floats(words).copy()
    o = np.nonzero(cls == ORDINARY)[0]
    a, b, c = f[o, 3:6], f[o, 6:9], f[o, 9:12]
    half = o[::2]
    f[half, 0:3] = ((a[::2] + b[::2] + c[::2]) * F32(1.0 / 3.0)).astype(F32)
    if with_area:
        f[o, 12] = np.maximum(_np_area(a, b, c), F32(2.0 ** -20))
    return bits(f)


def _bary_mix_struct(rng, m):
    tri = _ordinary(rng, (m, 9))
    e = np.eye(3, dtype=F32)
    bc = np.stack([np.tile(e[0], (m, 1)), np.tile(e[1], (m, 1)), np.tile(e[2], (m, 1)), np.full((m, 3), F32(1.0 / 3.0)),
                   np.zeros((m, 3), F32), rng.dirichlet((1, 1, 1), m).astype(F32), -np.zeros((m, 3), F32)], 1)
    return np.hstack([bc[np.arange(m), np.arange(m) % 7], tri]).astype(F32)


def _mat_struct(rng, m):
    M = _ordinary(rng, (m, 16))
    p = _ordinary(rng, (m, 3))
    eye = np.tile(np.eye(4, dtype=F32).ravel(), (m, 1))
    zero = np.zeros((m, 16), F32)
    k = np.arange(m) % 5
    Ms = np.stack([eye, zero, M, M, -zero], 1)[np.arange(m), k]
    ps = np.stack([p, p, np.zeros((m, 3), F32), -np.zeros((m, 3), F32), p], 1)[np.arange(m), k]
    cancel = Ms.copy()  # the translation cancels the rotated point: the last addition is exact zero or a rounding error
    return np.hstack([cancel, ps]).astype(F32)


def _sky_struct(rng, m):
    d = _ordinary(rng, (m, 3))
    ys = np.array([0.0, -0.0, 2.0 ** -149, 1.0, _nextafter(1, True), _nextafter(1, False), 0.5, 2.0, np.nan, np.inf, -np.inf, -1.0,
                   2.0 ** 24, 3.0e38, 2.0 ** -126], F32)
    d[:, 1] = ys[np.arange(m) % len(ys)]
    d[: m // 2, 1] = rng.uniform(0, 1, m // 2).astype(F32)  # the unit directions of a frame
    return d


def _hitbary_struct(rng, m):
    ad = _ordinary(rng, (m,))
    w = rng.dirichlet((1, 1, 1), m).astype(F32)
    u = (-w[:, 1] * ad).astype(F32)  # HitRec::u is negated
    v = (w[:, 2] * ad).astype(F32)
    z = np.zeros(m, F32)
    rows = np.stack([np.stack([u, v, ad], 1), np.stack([z, z, ad], 1), np.stack([-ad, z, ad], 1), np.stack([z, ad, ad], 1),
                     np.stack([u, v, z], 1), np.stack([z, z, z], 1), np.stack([-z, -z, ad], 1), np.stack([u, (ad + u).astype(F32), ad], 1)], 1)
    return rows[np.arange(m), np.arange(m) % 8].astype(F32)


def _light_struct(rng, m):
    """o, d, c, radius: inside the sphere, on its centre, aimed at it, away from it, tangent, radius 0, d = 0"""
    o = _ordinary(rng, (m, 3))
    c = _ordinary(rng, (m, 3))
    r = _ordinary(rng, (m, 1), positive=True)
    aimed = (c - o).astype(F32)
    z3 = np.zeros((m, 3), F32)
    side = rng.integers(1, 9, (m, 1)).astype(F32)
    tang_o = np.hstack([z3[:, :2], -side])  # o = (0, 0, -s), c = (0, r, 0), d = (0, 0, 1): the ray grazes the sphere
    tang_c = np.hstack([z3[:, :1], r, z3[:, :1]])
    tang_d = np.tile(np.array([0, 0, 1], F32), (m, 1))
    rows = np.stack([
        np.hstack([o, _ordinary(rng, (m, 3)), o, r]),                       # the camera in the centre
        np.hstack([o, aimed, c, r]),                                        # aimed at the centre
        np.hstack([o, -aimed, c, r]),                                       # the sphere behind the ray (or around its origin)
        np.hstack([o, aimed, c, np.zeros((m, 1), F32)]),                    # radius 0
        np.hstack([o, z3, c, r]),                                           # no direction: a == 0
        np.hstack([tang_o, tang_d, tang_c, r]),                             # tangent: the discriminant is exactly 0
        np.hstack([tang_o, tang_d, tang_c, _nextafter_arr(r, True)]),       # ... and just inside
        np.hstack([tang_o, tang_d, tang_c, _nextafter_arr(r, False)]),      # ... and just outside
        np.hstack([o, (aimed * F32(2.0 ** -40)).astype(F32), c, r]),        # a short direction: 2a small
    ], 1)
    return rows[np.arange(m), np.arange(m) % 9].astype(F32)


def _nextafter_arr(x, up):
    return np.nextafter(x.astype(F32), F32(np.inf) if up else F32(-np.inf)).astype(F32)


def _light_ordinary_fix(rng, words, cls):
    """ordinary items: every second ray is aimed near the sphere (random directions of ordinary magnitude seldom meet it)"""
    f = floats(words).copy()
    o = np.nonzero(cls == ORDINARY)[0][::2]
    to_c = (f[o, 6:9] - f[o, 0:3]).astype(F32)
    dist = np.sqrt((to_c.astype(np.float64) ** 2).sum(-1, keepdims=True))
    jitter = rng.normal(0, 1, (len(o), 3)) * dist * 0.02 + rng.normal(0, 1, (len(o), 3)) * f[o, 9:10] * 0.7
    f[o, 3:6] = (to_c + jitter).astype(F32)
    return bits(f)


# ---------------------------------------------------------------------------------------------- functions with a domain
def _sincos_cases(rng, n):
    c = _split(n, _DEFAULT_W)
    one = U32(0x3f800000)
    parts = [bits(rng.uniform(0, 1, c[0]).astype(F32)),
             (_anybits(rng, c[1]) % (one + U32(1))),
             bits(_scale(rng, _ordinary(rng, (c[2],), positive=True), -70, -60)),
             bits((F32(1) - _scale(rng, _ordinary(rng, (c[3],), positive=True), -24, -9)).astype(F32)),  # no big u: up against 1
             np.array([0x00000000, 0x80000000, 0x00000001, 0x3f800000, 0x3f7fffff, 0x00800000, 0x007fffff], U32)[np.arange(c[4]) % 7]]
    # every exponent of [0, 1] with a few significands, and k/8 +- 1 ulp
    ex = (np.arange(0, 127, dtype=np.uint32)[:, None] << U32(23)) | np.array([0, 1, 0x400000, 0x555555, 0x7fffff], U32)[None, :]
    k8 = bits(np.arange(0, 9, dtype=F32) / F32(8))
    st = np.concatenate([ex.ravel(), k8, k8[1:] - U32(1), k8[:-1] + U32(1), np.array([0x3f800000], U32)])
    parts.append(_cycle(st, c[5]))
    cls = np.concatenate([np.full(len(p), i, np.uint8) for i, p in enumerate(parts)])
    w = np.concatenate(parts).astype(U32)
    assert (w <= one).all() or ((w[w > one] == U32(0x80000000)).all())
    return w[:, None], cls


def _log_struct(rng, m):
    ex = (np.arange(0, 255, dtype=np.uint32)[:, None] << U32(23)) | np.array([0, 1, 0x3504f3, 0x3504f4, 0x400000, 0x7fffff], U32)[None, :]
    ex = ex.ravel()
    ex = ex[ex != 0]
    return _cycle(ex, m)[:, None].astype(U32)


def _exp_struct(rng, m):
    th = np.array([-87.0, 88.0], F32)
    edge = np.concatenate([th, _nextafter_arr(th, True), _nextafter_arr(th, False),
                           np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** -149, -2.0 ** -149, 1.0, -1.0], F32)])
    k = np.arange(m) % 4
    x = np.where(k == 1, rng.uniform(0, 88, m), np.where(k == 2, rng.uniform(-87, 0, m), rng.uniform(-100, 100, m))).astype(F32)
    x[k == 0] = edge[(np.arange(m) // 4) % len(edge)][k == 0]
    return x[:, None]


def _f2i_struct(rng, m):
    p31 = F32(2.0 ** 31)
    edge = np.array([p31, -p31, _nextafter(p31, True), _nextafter(p31, False), _nextafter(-p31, True), _nextafter(-p31, False),
                     0.99999994, -0.99999994, 0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 1.5, -1.5, 2.0 ** 24, 2.0 ** 24 + 2, -2.0 ** 24,
                     8388607.5, -8388607.5, 2.0 ** 30, -2.0 ** 30, 2.0 ** -149, -2.0 ** -149, 3.4e38, -3.4e38, 2.0 ** 32, 2.0 ** 63], F32)
    mid = (np.exp2(rng.uniform(0, 33, m)) * rng.choice([-1.0, 1.0], m)).astype(F32)  # the whole range of int and a little beyond
    return np.where(np.arange(m) % 2 == 0, edge[(np.arange(m) // 2) % len(edge)], mid).astype(F32)[:, None]


def _minmax_struct(rng, m):
    pairs = np.array([(a, b) for a in SPECIALS for b in SPECIALS], U32)  # all 49 ordered pairs
    x = bits(_ordinary(rng, (m,)))
    more = np.stack([np.stack([x, x], 1), np.stack([x, x + U32(1)], 1), np.stack([x + U32(1), x], 1), np.stack([x, x ^ U32(0x80000000)], 1)], 1)
    more = more[np.arange(m), np.arange(m) % 4]
    out = np.where((np.arange(m) < len(pairs) * 4)[:, None], _cycle(pairs, m), more)
    return out.astype(U32)


def _powi_cases(rng, n):
    def structural(rng, m):
        xs = np.array([0.0, -0.0, 1.0, _nextafter(1, True), _nextafter(1, False), -1.0, -1.5, -0.99, -2.0, 2.0 ** -20, 2.0 ** -75, 1e-30,
                       -2.0 ** -75, 0.5, 2.0, 1.0000119, 0.9999, np.inf, -np.inf, np.nan, 2.0 ** -149, 3.4e38, 1.4142135, -1.4142135], F32)
        return _cycle(xs, m)[:, None]
    w, cls = _float_cases(rng, n, 1, _DEFAULT_W, structural)
    ns = np.array(POWI_N, U32)
    nn = ns[rng.integers(0, len(ns), len(w))]
    s = np.nonzero(cls == STRUCTURAL)[0]
    nn[s] = ns[(np.arange(len(s)) // 24) % len(ns)]  # every x of the list with every n
    # ordinary x within 2^-8 .. 2^8 overflows under n = 127 and up: that is the scaled classes' business; keep the ordinary class's
    # results finite by drawing its bases from 2^-0.45 .. 2^0.45 for the long exponents
    o = np.nonzero((cls == ORDINARY) & (nn >= U32(127)))[0]
    f = floats(w).copy()
    f[o, 0] = (np.sign(f[o, 0]) * np.exp2(rng.uniform(-0.45, 0.45, len(o)))).astype(F32)
    return np.hstack([bits(f), nn[:, None]]).astype(U32), cls


def _rng_cases(rng, n, k):
    c = _split(n, (0.3, 0.5, 0, 0, 0.2, 0, 0))
    small = np.stack([rng.integers(0, 3840, c[0]), rng.integers(0, 2160, c[0]), rng.integers(0, 1000, c[0]), rng.integers(0, 4, c[0])], 1).astype(U32)
    pool = np.array([0, 1, 0xffffffff, 0x80000000, 0x7fffffff, 0xfffffffe], U32)
    sp = _anybits(rng, (c[4], k))
    j = np.arange(c[4])
    sp[j, j % k] = pool[(j // k) % len(pool)]
    parts = [small[:, :k] if k == 4 else (small[:, 0] * U32(3266489917) + small[:, 1] * U32(668265263))[:, None], _anybits(rng, (c[1], k)), sp]
    cls = np.concatenate([np.full(len(parts[0]), ORDINARY, np.uint8), np.full(len(parts[1]), ANYBITS, np.uint8), np.full(len(parts[2]), SPECIALS_CLS, np.uint8)])
    return np.concatenate(parts).astype(U32), cls


# ---------------------------------------------------------------------------------------------- reproject_pixel
# words: W, H, PVprev[16] (2..17), id (18), wp (19..21), three cells of four floats (22..33), x (34), y (35)
_RP_FLOATS = list(range(2, 18)) + list(range(19, 34))


def _rp_frame(rng, m):
    wh = np.array(REPROJECT_WH, np.int64)
    W = wh[rng.integers(0, 4, m)]
    H = wh[rng.integers(0, 4, m)]
    x = (rng.integers(0, 2 ** 31, m) % W).astype(np.int64)
    y = (rng.integers(0, 2 ** 31, m) % H).astype(np.int64)
    return W, H, x, y


def _rp_pack(W, H, M, idv, wp, tri, x, y, cell_w=None):
    m = len(W)
    w = np.zeros((m, 36), U32)
    w[:, 0] = W.astype(np.int64).astype(U32)
    w[:, 1] = H.astype(np.int64).astype(U32)
    w[:, 2:18] = bits(M)
    w[:, 18] = idv.astype(U32)
    w[:, 19:22] = bits(wp)
    for k in range(3):
        w[:, 22 + 4 * k:25 + 4 * k] = bits(tri[:, 3 * k:3 * k + 3])
        if cell_w is not None:
            w[:, 25 + 4 * k] = cell_w[:, k]
    w[:, 34] = (x.astype(np.int64) & 0xffffffff).astype(U32)
    w[:, 35] = (y.astype(np.int64) & 0xffffffff).astype(U32)
    return w


def _rp_onscreen(rng, m):
    """a triangle of coordinates below 2, a point inside it, a previous camera whose clip w stays in 1.5 .. 6.5 and whose clip x
    and y stay mostly inside +-w: most items land in the frame"""
    W, H, x, y = _rp_frame(rng, m)
    tri = (_ordinary(rng, (m, 9)) * F32(2.0 ** -7)).astype(F32)
    wgt = rng.dirichlet((1, 1, 1), m).astype(F32)
    wp = (wgt[:, :1] * tri[:, 0:3] + wgt[:, 1:2] * tri[:, 3:6] + wgt[:, 2:] * tri[:, 6:9]).astype(F32)
    M = rng.uniform(-0.25, 0.25, (m, 16)).astype(F32)
    M[:, 12:14] = rng.uniform(-0.5, 0.5, (m, 2)).astype(F32)
    M[:, 15] = rng.uniform(3, 5, m).astype(F32)
    return _rp_pack(W, H, M, rng.integers(1, 4, m), wp, tri, x, y)


def _rp_structural(rng, m):
    """id 0; clip w zero, tiny, negative, NaN; screen coordinates within an ulp of an integer, of 0, of W and H; beyond +-2^31;
    degenerate triangles.  The camera of the screen-coordinate items maps every point to ndc = (M[12], M[13]) with w = 1."""
    W, H, x, y = _rp_frame(rng, m)
    tri = _int_points(rng, (m, 9), 8)
    deg = _degenerate_triangles(rng, m)
    wgt = rng.dirichlet((1, 1, 1), m).astype(F32)
    kind = np.arange(m) % 8
    tri = np.where((kind == 7)[:, None], deg, tri).astype(F32)
    wp = (wgt[:, :1] * tri[:, 0:3] + wgt[:, 1:2] * tri[:, 3:6] + wgt[:, 2:] * tri[:, 6:9]).astype(F32)
    M = np.zeros((m, 16), F32)
    M[:, 15] = 1
    # the target screen coordinate s (pixels) gives ndc = 2 s / W - 1, then moved by -2 .. 2 ulps
    def ndc_for(size):
        tgt = np.stack([np.zeros(m), size.astype(np.float64), rng.integers(0, 1 << 12, m) % (size + 1), size - 1.0, np.ones(m)], 1)
        s = tgt[np.arange(m), rng.integers(0, 5, m)]
        v = (2.0 * s / size - 1.0).astype(F32)
        return floats((bits(v).astype(np.int64) + rng.integers(-2, 3, m)).astype(U32))
    M[:, 12] = ndc_for(W)
    M[:, 13] = ndc_for(H)
    far = np.array([2.0 ** 31, -2.0 ** 31, 2.0 ** 32, -2.0 ** 32, 3e38, -3e38, np.inf, -np.inf, np.nan, 2.0 ** 30, 4.3e9, -4.3e9], F32)
    k2 = kind == 2  # beyond +-2^31: ndc * 0.5 + 0.5 times W is the far value itself with W == 1, and larger otherwise
    M[k2, 12] = _cycle(far, m)[k2]
    M[k2, 13] = _cycle(far[::-1], m)[k2]
    clw = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, -2.0 ** -126, -1.0, np.nan, -2.0 ** -100, 2.0 ** -100, np.inf, -np.inf], F32)
    k3 = kind == 3
    M[k3, 15] = _cycle(clw, m)[k3]
    M[k3, 12] = rng.uniform(-1, 1, int(k3.sum())).astype(F32)
    k4 = kind == 4  # a general camera whose w row cancels at the point: clip w is a rounding error or exactly zero
    M[k4] = rng.uniform(-1, 1, (int(k4.sum()), 16)).astype(F32)
    M[k4, 15] = -(M[k4, 3] * wp[k4, 0] + M[k4, 7] * wp[k4, 1] + M[k4, 11] * wp[k4, 2]).astype(F32)
    idv = rng.integers(1, 4, m)
    idv[kind == 0] = 0  # nothing to reproject: the pixel itself, whatever the other words hold
    x = np.where(kind == 0, rng.integers(-2 ** 31, 2 ** 31, m), x)
    y = np.where(kind == 0, rng.integers(-2 ** 31, 2 ** 31, m), y)
    return _rp_pack(W, H, M, idv, wp, tri, x, y)


def _reproject_cases(rng, n):
    c = _split(n, WEIGHTS["reproject_pixel"])
    parts, cls = [], []

    def generic(m, make):
        W, H, x, y = _rp_frame(rng, m)
        f = make(m)
        return _rp_pack(W, H, f[:, 0:16], rng.integers(0, 4, m), f[:, 16:19], f[:, 19:28], x, y, cell_w=bits(f[:, 28:31]))

    parts.append(generic(c[0], lambda m: _ordinary(rng, (m, 31))))
    a = generic(c[1], lambda m: floats(_anybits(rng, (m, 31))))
    a[:, 34:36] = _anybits(rng, (c[1], 2))
    parts.append(a)
    parts.append(generic(c[2], lambda m: _scale(rng, _ordinary(rng, (m, 31)), -70, -60)))
    parts.append(generic(c[3], lambda m: _scale(rng, _ordinary(rng, (m, 31)), 60, 66)))
    sp = _rp_onscreen(rng, c[4])
    j = np.arange(c[4])
    pos = np.array(_RP_FLOATS)[j % len(_RP_FLOATS)]
    sp[j, pos] = SPECIALS[(j // len(_RP_FLOATS)) % len(SPECIALS)]
    parts.append(sp)
    parts.append(_rp_structural(rng, c[5]))
    parts.append(_rp_onscreen(rng, c[6]))
    for i, p in enumerate(parts):
        cls.append(np.full(len(p), i, np.uint8))
    return np.concatenate(parts).astype(U32), np.concatenate(cls)


# ---------------------------------------------------------------------------------------------- the table
def cases(fn, n, seed=20240521):
    """(words [n, n_in] uint32, cls [n] uint8) for the function named fn"""
    idx = fn_index(fn)
    rng = np.random.default_rng([seed, idx])
    k = WORDS[idx][0]
    wts = WEIGHTS[fn]
    if fn in ("dot", "cross"):
        w, cls = _float_cases(rng, n, 6, wts, _vec_pairs)
    elif fn in ("length", "normalize"):
        w, cls = _float_cases(rng, n, 3, wts, _vec_single)
    elif fn == "powi":
        w, cls = _powi_cases(rng, n)
    elif fn == "f2i":
        w, cls = _float_cases(rng, n, 1, wts, _f2i_struct)
    elif fn == "minmax":
        w, cls = _float_cases(rng, n, 2, wts, _minmax_struct)
    elif fn == "rng_seed":
        w, cls = _rng_cases(rng, n, 4)
    elif fn == "rng_next_skip":
        w, cls = _rng_cases(rng, n, 1)
    elif fn == "sincos2pi":
        w, cls = _sincos_cases(rng, n)
    elif fn == "log":
        w, cls = _float_cases(rng, n, 1, wts, _log_struct, positive=True)
    elif fn == "exp":
        w, cls = _float_cases(rng, n, 1, wts, _exp_struct)
    elif fn == "mat_row_point":
        w, cls = _float_cases(rng, n, 19, wts, _mat_struct)
    elif fn == "div":
        w, cls = _float_cases(rng, n, 2, wts, _div_pairs)
    elif fn == "div2":
        w, cls = _float_cases(rng, n, 3, wts, _div2_triples)
    elif fn == "tri_area":
        w, cls = _float_cases(rng, n, 9, wts, _tri_area_struct)
    elif fn == "bary_coords":
        w, cls = _float_cases(rng, n, 12, wts, lambda r, m: _bary_struct(r, m))
        w = _bary_ordinary_fix(w, cls, False)
    elif fn == "bary_coords_at":
        w, cls = _float_cases(rng, n, 13, wts, lambda r, m: _bary_struct(r, m, True))
        w = _bary_ordinary_fix(w, cls, True)
    elif fn == "bary_mix":
        w, cls = _float_cases(rng, n, 12, wts, _bary_mix_struct)
    elif fn == "reproject_pixel":
        w, cls = _reproject_cases(rng, n)
    elif fn == "ray_hits_light":
        w, cls = _float_cases(rng, n, 10, wts, _light_struct)
        w = _light_ordinary_fix(rng, w, cls)
    elif fn == "sky_color":
        w, cls = _float_cases(rng, n, 3, wts, _sky_struct)
    elif fn == "hit_barycentrics":
        w, cls = _float_cases(rng, n, 3, wts, _hitbary_struct)
    else:
        raise ValueError(fn)
    assert w.shape == (n, k) and w.dtype == U32 and cls.shape == (n,), (fn, w.shape, n, k)
    return np.ascontiguousarray(w), cls
