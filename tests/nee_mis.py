"""Multiple importance sampling of next-event estimation (RTPT_FLAG_EXT_NEE_MIS; csrc/light_sample.hpp states the rules) restated
in numpy for test_nee_mis_*.py: the two weights of the power heuristic, the light sample's weight function at a point a bounce
hit, the search for a hit emitter's entry of the light list, operands and the scene with a close emitter.

Everything the device fixes is one correctly rounded float32 operation at a time (numpy's products, sums and divisions, the
contract's dot, cross, normalize and fused multiply-add through dielectric_scenes) or integer arithmetic, so numpy gives the same
bits.  find() is the binary search of csrc/light_list_host.hpp, step for step on arrays of queries; test_nee_mis_cpu.py holds it to
np.searchsorted.  tests/path_walker.py walks the paths with the three rules where `mis` (and the list has entries): the sample's g
becomes g * m(g), a diffuse hit that goes on records the cosine cb of its new direction, and an emissive triangle met with the
sampled bit set ends the path with (T * Ke) * wb(g_hit) instead of 0.  With `mis` off it weighs nothing, which test_nee_mis_cpu.py
asks for bit by bit against the recorded frames of the walker without the flag."""
import numpy as np

import nee_power as PW
import nee_scenes as N
import pathtrace_scenes as P
from dielectric_scenes import dot, fma, normalize

F32, U32, U64 = np.float32, np.uint32, np.uint64
ONE = F32(1.0)
INF = F32(np.inf)


# ------------------------------------------------------------------------------------------ the weights
def m_light(g):
    """m(g) = 1 / (1 + g * g), float32: the light side of the power heuristic"""
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        g2 = (g * g).astype(F32)
        return (ONE / (ONE + g2).astype(F32)).astype(F32)


def wb(g):
    """wb(g) = g2 / (1 + g2) where g2 = g * g < +inf, else 1 (a NaN fails the comparison), float32: the bounce side"""
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        g2 = (g * g).astype(F32)
        return np.where(g2 < INF, (g2 / (ONE + g2).astype(F32)).astype(F32), ONE).astype(F32)


def gm(g):
    """g * m(g): the light sample's weight, one multiply behind sample()'s division"""
    g = np.asarray(g, F32)
    with np.errstate(all="ignore"):
        return (g * m_light(g)).astype(F32)


def weights64(g):
    """(wb, gm) in float64 from the float32 g as it is"""
    g = np.asarray(g, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        g2 = g * g
        return g2 / (1 + g2), g / (1 + g2)


def g_hit(O, v0, v1, v2, o, d, b1, b2, cb, inv_p):
    """light::hit_weight, operation by operation: the light sample's weight function at the point with barycentrics (b1, b2) of
    the emitter (v0, v1, v2) that the ray (o, d) hit; the emitter's unit normal as its shade record's, b0 as hit_barycentrics"""
    v0, v1, v2, o, d = (np.asarray(a, F32).reshape(-1, 3) for a in (v0, v1, v2, o, d))
    b1, b2, cb, inv_p = (np.asarray(a, F32).ravel() for a in (b1, b2, cb, inv_p))
    with np.errstate(all="ignore"):
        b0 = ((ONE - b1).astype(F32) - b2).astype(F32)
        e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
        cr = N.cross(O, e1, e2)
        nl = normalize(O, cr)                                                                          # raytrace.comp.glsl:150
        y = fma(O, v2, b2[:, None], fma(O, v1, b1[:, None], (v0 * b0[:, None]).astype(F32)))           # bary_point
        w = (y - o).astype(F32)
        r2 = dot(O, w, w)
        cl = np.abs(dot(O, nl, d))
        a2 = np.sqrt(dot(O, cr, cr)).astype(F32)
        return (((cb * cl).astype(F32) * (a2 * inv_p).astype(F32)).astype(F32) / (N.K2PI * r2).astype(F32)).astype(F32)


def cases_of(v0, v1, v2, o, d, b1, b2, cb, inv_p):
    """[n, 20] float32 of rtpt_selftest_mis_weight's input (word 19 is not read: 0)"""
    n = len(np.asarray(o).reshape(-1, 3))
    f = np.concatenate([np.broadcast_to(np.asarray(a, F32), (n, 3)) for a in (v0, v1, v2, o, d)] +
                       [np.broadcast_to(np.asarray(a, F32), (n,))[:, None] for a in (b1, b2, cb, inv_p, 0.0)], 1).astype(F32)
    return np.ascontiguousarray(f)


def mis_weight32(O, cases):
    """[n, 3] float32 (g_hit, wb(g_hit), g_hit * m(g_hit)) of cases [n, 20]: what rtpt_selftest_mis_weight returns"""
    c = np.ascontiguousarray(cases, F32).reshape(-1, 20)
    g = g_hit(O, c[:, 0:3], c[:, 3:6], c[:, 6:9], c[:, 9:12], c[:, 12:15], c[:, 15], c[:, 16], c[:, 17], c[:, 18])
    return np.stack([g, wb(g), gm(g)], 1).astype(F32)


# ------------------------------------------------------------------------------------------ the search
def find(ids, queries):
    """uint32 [k]: rtpt_light::find of every query on the ascending list ids [n] — the index of the entry, n where the list does
    not hold the id.  The device's loop, step for step, on all queries at once; every index read lies in [0, n)"""
    ids = np.ascontiguousarray(ids, U32).ravel()
    q = np.ascontiguousarray(queries, U32).ravel()
    n = len(ids)
    lo, hi = np.zeros(len(q), np.int64), np.full(len(q), n, np.int64)
    while True:
        go = lo < hi
        if not go.any():
            break
        mid = lo + ((hi - lo) >> 1)
        assert n > 0 and mid[go].min() >= 0 and mid[go].max() < n
        less = np.zeros(len(q), bool)
        less[go] = ids[mid[go]] < q[go]
        lo = np.where(go & less, mid + 1, lo)
        hi = np.where(go & ~less, mid, hi)
    found = lo < n
    found[found] = ids[lo[found]] == q[found]
    return np.where(found, lo, n).astype(U32)


def hit_inv_p(lights, cdf, id1):
    """(reached bool [k], inv_p float32 [k]) for the emitters id1 [k] a bounce hit: float(L) for the uniform pick (cdf None); for
    the weighted pick float(S) / float(q_i) of the emitter's entry, not reached where q_i == 0 or the list does not hold the id"""
    L = len(lights)
    id1 = np.asarray(id1, U32).ravel()
    if cdf is None:
        return np.ones(len(id1), bool), np.full(len(id1), F32(L), F32)
    cdf = np.asarray(cdf, U64)
    i = find(lights, id1).astype(np.int64)
    held = i < L
    ic = np.minimum(i, L - 1)
    q = cdf[ic] - np.where(ic > 0, cdf[np.maximum(ic - 1, 0)], U64(0))
    reached = held & (q > 0)
    with np.errstate(all="ignore"):
        inv_p = (np.full(len(id1), cdf[-1], U64).astype(F32) / q.astype(F32)).astype(F32)
    return reached, np.where(reached, inv_p, F32(0)).astype(F32)


# ------------------------------------------------------------------------------------------ operands
G_HOSTILE = np.array([0.0, 1e-45, 1e-40, 1.17549435e-38, 1e-20, 0.5, 1.0, 2.0, 2.0 ** 63, 2.0 ** 64, 2.0 ** 64 * 1.5, 1e30, 3.4028235e38,
                      np.inf, np.nan, -1.0, -np.inf], np.float64).astype(F32)
G_HOSTILE.setflags(write=False)


def seeded_g(n=4096, seed=67):
    """n weights over twelve decades around 1, log-uniform"""
    g = (10.0 ** np.random.default_rng(seed).uniform(-6, 6, n)).astype(F32)
    g.setflags(write=False)
    return g


def seeded_cases(n=4096, seed=71):
    """[n, 20]: emitters of random vertices in [-1, 1]^3, a hit point of random barycentrics on each, the ray's origin at a distance
    log-uniform in [0.01, 4] along a random direction, cb uniform in (0, 1], inv_p log-uniform in [1, 2^20]"""
    r = np.random.default_rng(seed)
    v = r.uniform(-1, 1, (n, 3, 3)).astype(F32)
    su, ub = np.sqrt(r.random(n)), r.random(n)
    b1, b2 = (su * (1 - ub)).astype(F32), (su * ub).astype(F32)
    y = v[:, 0] * (1 - b1 - b2)[:, None] + v[:, 1] * b1[:, None] + v[:, 2] * b2[:, None]
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = 10.0 ** r.uniform(-2, np.log10(4.0), n)
    o = y - dist[:, None] * d
    out = cases_of(v[:, 0], v[:, 1], v[:, 2], o, d, b1, b2, 1.0 - r.random(n), 2.0 ** r.uniform(0, 20, n))
    out.setflags(write=False)
    return out


def hostile_cases():
    """[n, 20]: on one emitter — cl = 0 (the ray in the emitter's plane), cb = 0, inv_p = inf (q_i = 0 by the formula) with cb * cl
    positive and zero, inv_p = NaN and 0, r2 = 0 (the origin on the hit point), r2 subnormal, a degenerate emitter (a2 = 0), huge
    and tiny operands (g2 overflows, g underflows), cb negative and NaN, barycentrics outside the triangle"""
    v0, v1, v2 = F32([0, 0, 0]), F32([1, 0, 0]), F32([0, 0, 1])                       # in the plane y = 0, normal (0, -1, 0)
    down, o = F32([0, -1, 0]), F32([0.25, 1, 0.25])
    rows = [
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.5, 2.0),                            # an ordinary hit
        cases_of(v0, v1, v2, F32([-1, 0, 0.25]), F32([1, 0, 0]), 0.25, 0.25, 0.5, 2.0),  # cl = 0
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.0, 2.0),                            # cb = 0
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.5, np.inf),                         # q_i = 0: inv_p = inf
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.0, np.inf),                         # ... times 0: NaN
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.5, np.nan),
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, 0.5, 0.0),
        cases_of(v0, v1, v2, F32([0.25, 0, 0.25]), down, 0.25, 0.25, 0.5, 2.0),         # r2 = 0
        cases_of(v0, v1, v2, F32([0.25, 2.0 ** -70, 0.25]), down, 0.25, 0.25, 0.5, 2.0),  # r2 = 2^-140
        cases_of(v0, v1, v1, o, down, 0.25, 0.25, 0.5, 2.0),                            # a2 = 0
        cases_of(v0, v1, v2, F32([0.25, 2.0 ** -20, 0.25]), down, 0.25, 0.25, 1.0, 2.0 ** 30),   # g2 overflows
        cases_of(v0, v1, v2, F32([0.25, 2.0 ** -40, 0.25]), down, 0.25, 0.25, 1.0, 2.0 ** 60),   # g overflows
        cases_of(v0, v1, v2, F32([0.25, 2.0 ** 40, 0.25]), down, 0.25, 0.25, 2.0 ** -40, 1.0),   # g underflows
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, -0.5, 2.0),                           # cb < 0 (no bounce leaves with one)
        cases_of(v0, v1, v2, o, down, 0.25, 0.25, np.nan, 2.0),
        cases_of(v0, v1, v2, o, down, 3.0, -2.5, 0.5, 2.0),                             # barycentrics outside
        cases_of(v0 * F32(1e18), v1 * F32(1e18), v2 * F32(1e18), o, down, 0.25, 0.25, 0.5, 2.0),   # the cross product overflows
    ]
    out = np.concatenate(rows)
    out.setflags(write=False)
    return out


FIND_SIZES = (1, 2, 3, 1000, (1 << 20) + 1025)


def find_case(n, seed=73):
    """(ids [n] ascending with gaps of 1 to 5 between neighbours, queries): both ends, every entry and every gap (of a list up to
    1,000 entries; of a longer one 4,096 seeded places), ids below, above and between the entries"""
    r = np.random.default_rng(seed + n)
    ids = (2 + np.cumsum(r.integers(1, 6, n))).astype(U32)
    at = np.arange(n) if n <= 1000 else np.unique(np.concatenate([[0, n - 1], r.integers(0, n, 4096)]))
    e = ids[at].astype(np.int64)
    q = np.concatenate([e, e + 1, e - 1, e + 2, [0, 1, 2, int(ids[0]) - 1, int(ids[-1]) + 1, 2 ** 32 - 1, 2 ** 31]])
    return ids, np.clip(q, 0, 2 ** 32 - 1).astype(U32)


# ------------------------------------------------------------------------------------------ scenes
WALL_LAMP = np.array([(-2.2, 1.6, 0.02), (2.2, 1.6, 0.02), (2.2, 1.6, 1.0), (-2.2, 1.6, 1.0)], np.float64)


def wall_lamp():
    """nee_power's receiver quad with an emissive wall standing on it, just outside the view of nee_scenes.receiver()'s camera: the
    hit points next to the wall are where the area sample's weight is unbounded.  Materials: 0 the receiver, 1 the wall"""
    quads = np.array([PW.RECEIVER_QUAD, WALL_LAMP], np.float64)
    tris, mat = P._with_form("small", quads, np.array([0, 1]))
    materials = P._materials((N.RECEIVER_KD,), (N.RECEIVER_KE,))
    return P.Scene("nee_wall_lamp", "small", tris, N.RECEIVER_CAM, N.RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)
