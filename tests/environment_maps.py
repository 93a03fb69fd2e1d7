"""The environment map (rtpt_set_environment; csrc/env.hpp, include/rtpt.h: rules E1 to E6) for test_environment_*.py: the numpy
float32 restatement of the lookup, the double-precision decode and lat-long conversion (csrc/env_host.hpp), the maps and the
hostile directions, and the seam that puts the restatement where tests/path_walker.py reaches the sky.

color32 follows the rules one float32 operation per device operation: every dot and every fused multiply-add through the oracle's
statement of the numerics contract (dielectric_scenes.dot / fma), the sums, products, differences and the two divisions in numpy
float32 (all correctly rounded, like the device's).

path_walker reaches the sky through its module-level name `_contract` with the function name "sky_color", once per segment of a
sample's paths.  environment(O, env) replaces that name for the duration of a walk(): every other contract function is forwarded
untouched, "sky_color" is answered with color32, and the directions of every call are recorded — the paths that ended in
the environment at that segment.  (`_primary`, the walker's primary-ray generation, is wrapped as a pure pass-through that marks
where a sample starts, so that the calls of samples_per_pixel > 1 can be told apart.)  path_walker.py itself is not edited."""
from collections import namedtuple
from contextlib import contextmanager

import numpy as np

from dielectric_scenes import dot, fma

F32, U32 = np.float32, np.uint32
NEAREST = 0x1                                    # RTPT_TEX_NEAREST
MAX_SIZE = 4096
SIZES = (1, 2, 3, 8, 64)

# texels [n, n, 4] float32 (row j holds V in [j / n, (j + 1) / n)), flags, rotation [3, 3] row-major, scale [3]
Env = namedtuple("Env", "texels flags rotation scale")


def make_env(texels, flags=0, rotation=None, scale=None):
    tx = np.ascontiguousarray(texels, F32)
    assert tx.ndim == 3 and tx.shape[0] == tx.shape[1] and tx.shape[2] == 4
    rot = np.eye(3, dtype=F32) if rotation is None else np.ascontiguousarray(rotation, F32).reshape(3, 3)
    sc = np.ones(3, F32) if scale is None else np.ascontiguousarray(scale, F32).reshape(3)
    return Env(tx, int(flags), rot, sc)


# ------------------------------------------------------------------------------------------ E1 to E6 in float32
def octahedral32(O, env, d):
    """(U [k], V [k], ok [k]) of directions d [k, 3]: E1 to E5's first line.  U and V are 0 where E2 refuses"""
    d = np.ascontiguousarray(d, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = np.stack([dot(O, np.broadcast_to(env.rotation[i], d.shape), d) for i in range(3)], 1)        # E1
        s = ((np.abs(e[:, 0]) + np.abs(e[:, 1])).astype(F32) + np.abs(e[:, 2])).astype(F32)               # E2
        ok = (s > 0) & ~np.isinf(s)
        safe = np.where(ok, s, F32(1.0)).astype(F32)
        ex, ey, ez = (np.where(ok, e[:, i], F32(0.0)).astype(F32) for i in range(3))
        p, q = (ex / safe).astype(F32), (ez / safe).astype(F32)                                           # E3
        upper = ey >= 0
        u = np.where(upper, p, np.copysign((F32(1.0) - np.abs(q)).astype(F32), p)).astype(F32)            # E4
        v = np.where(upper, q, np.copysign((F32(1.0) - np.abs(p)).astype(F32), q)).astype(F32)
        U, V = fma(O, u, F32(0.5), F32(0.5)), fma(O, v, F32(0.5), F32(0.5))                               # E5
    return U, V, ok


def _taps(s, n):
    x = ((s * F32(n)).astype(F32) - F32(0.5)).astype(F32)
    x0 = np.floor(x).astype(F32)
    f = (x - x0).astype(F32)
    k = x0.astype(np.int64)
    return np.clip(k, 0, n - 1), np.clip(k + 1, 0, n - 1), f


def _lerp(a, b, f):
    return (a + (f[:, None] * (b - a).astype(F32)).astype(F32)).astype(F32)


def color32(O, env, d):
    """[k, 3] float32: env::color of directions d [k, 3], bit for bit"""
    U, V, ok = octahedral32(O, env, d)
    tx, n = env.texels, env.texels.shape[0]
    with np.errstate(all="ignore"):
        if env.flags & NEAREST:
            i = np.clip(np.floor((U * F32(n)).astype(F32)).astype(np.int64), 0, n - 1)
            j = np.clip(np.floor((V * F32(n)).astype(F32)).astype(np.int64), 0, n - 1)
            t = tx[j, i]
        else:
            i0, i1, fx = _taps(U, n)
            j0, j1, fy = _taps(V, n)
            t = _lerp(_lerp(tx[j0, i0], tx[j0, i1], fx), _lerp(tx[j1, i0], tx[j1, i1], fx), fy)
        out = (t[:, :3] * env.scale[None, :]).astype(F32)                                                  # E6
    out[~ok] = 0
    return out


# ------------------------------------------------------------------------------------------ the decode and the conversion in double
def decode64(U, V):
    """[..., 3] float64 unit directions (map frame) of the points (U, V) of the square: E5, E4 and E3 inverted"""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    u, v = 2.0 * U - 1.0, 2.0 * V - 1.0
    y = 1.0 - np.abs(u) - np.abs(v)
    lower = y < 0.0
    p = np.where(lower, np.copysign(1.0 - np.abs(v), u), u)
    q = np.where(lower, np.copysign(1.0 - np.abs(u), v), v)
    y = np.where(lower, -(1.0 - np.abs(p) - np.abs(q)), y)
    e = np.stack([p, y, q], -1)
    return e / np.sqrt(p * p + y * y + q * q)[..., None]


def centres64(n):
    """[n, n, 3]: the directions of the texel centres, [j, i]"""
    c = (np.arange(n) + 0.5) / n
    return decode64(c[None, :], c[:, None])


def from_latlong64(rgb, n):
    """[n, n, 4] float64, the conversion before its rounding to binary32: one bilinear sample of the lat-long image rgb [h, w, 3] at
    the direction of every texel centre (column fraction atan2(d.x, -d.z) / (2 pi) + 0.5, row fraction acos(d.y) / pi; wrapped
    horizontally, clamped vertically); alpha 1"""
    rgb = np.asarray(rgb, np.float32).astype(np.float64)
    h, w = rgb.shape[:2]
    d = centres64(n)
    cf = np.arctan2(d[..., 0], -d[..., 2]) / (2.0 * np.pi) + 0.5
    rf = np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / np.pi
    x, y = cf * w - 0.5, rf * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]
    i0 = np.mod(x0.astype(np.int64), w)
    i1 = np.mod(i0 + 1, w)
    j0 = np.clip(y0.astype(np.int64), 0, h - 1)
    j1 = np.clip(y0.astype(np.int64) + 1, 0, h - 1)
    top = rgb[j0, i0] + fx * (rgb[j0, i1] - rgb[j0, i0])
    bot = rgb[j1, i0] + fx * (rgb[j1, i1] - rgb[j1, i0])
    return np.concatenate([top + fy * (bot - top), np.ones((n, n, 1))], -1)


# ------------------------------------------------------------------------------------------ maps
def distinct_map(n, seed=0):
    """[n, n, 4] float32 whose texels are pairwise distinct in every colour channel, a few of them HDR (1e4 and above)"""
    rng = np.random.default_rng(1000 * n + seed)
    k = n * n
    tx = np.zeros((k, 4), F32)
    for c in range(3):
        tx[:, c] = (rng.permutation(k) + 1 + c * k).astype(np.float64) / (3.0 * k + 1.0) * (0.5 + c)
    hdr = rng.choice(k, size=max(1, k // 16), replace=False)
    tx[hdr, :3] = (1e4 * (1.0 + np.arange(len(hdr))[:, None] * 0.25 + np.arange(3)[None, :] * 0.0625)).astype(F32)
    tx[:, 3] = 0.5
    for c in range(3):
        assert len(np.unique(tx[:, c])) == k, (n, c)
    tx = tx.reshape(n, n, 4)
    tx.setflags(write=False)
    return tx


def direction_map(n):
    """[n, n, 4] float32: every texel holds its own centre's direction"""
    return np.concatenate([centres64(n), np.ones((n, n, 1))], -1).astype(F32)


def rotation(yaw_deg=30.0, tilt_deg=-20.0):
    """a proper rotation, float32 entries: yaw about y, then a tilt about x"""
    a, b = np.deg2rad(yaw_deg), np.deg2rad(tilt_deg)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (rx @ ry).astype(F32)


SCALE = (0.5, 1.25, 3.0)


def envs():
    """every generated map, bilinear and nearest, with and without a rotation and a scale: [(tag, Env)]"""
    out = []
    for n in SIZES:
        for flags in (0, NEAREST):
            for posed in (False, True):
                out.append(((n, flags, posed), make_env(distinct_map(n), flags, rotation() if posed else None, SCALE if posed else None)))
    return out


# ------------------------------------------------------------------------------------------ directions
def hostile_directions(seed=11, random=256):
    """[k, 3] float32: the six axes, +-0 components, each fold (|p| = 1, |q| = 1, e.y = +-0), directions that land exactly on texel
    centres and texel borders of the generated sizes on both sheets, denormals, one huge finite component, infinities, NaN, the zero
    vector, and seeded directions of both hemispheres, unit length and not"""
    z, inf, nan = 0.0, np.inf, np.nan
    rows = []
    for a in range(3):
        for sgn in (1.0, -1.0):
            v = [z, z, z]
            v[a] = sgn
            rows.append(v)
            rows.append([(-z if i != a else x) for i, x in enumerate(v)])                  # the other components -0
    rows += [[z, 1.0, -z], [-z, -1.0, z], [-z, -z, 1.0], [1.0, -z, z], [-z, z, -z], [z, z, z], [-z, -z, -z]]
    for y in (z, -z):                                                                       # the folds: e.y = +-0 ...
        rows += [[1.0, y, z], [-1.0, y, -z], [z, y, 1.0], [-z, y, -1.0]]                    # ... with |p| = 1 or |q| = 1
        rows += [[0.25, y, -0.75], [-0.5, y, 0.5], [0.125, y, 0.875], [-0.625, y, -0.375]]
    for n in (2, 8, 64, 3):                                                                 # texel centres and borders, exact for n = 2^k
        for a in range(2 * n + 1):
            for b in range(2 * n + 1):
                if n == 64 and (a % 16 not in (0, 1, 15) or b % 16 not in (0, 1, 15)):
                    continue
                u, v = a / n - 1.0, b / n - 1.0                                             # even a, b: borders; odd: centres
                if abs(u) + abs(v) <= 1.0:
                    rows.append([u, 1.0 - abs(u) - abs(v), v])
                    rows.append([u, -(1.0 - abs(u) - abs(v)), v])
                    rows.append([3.0 * u, -3.0 * (1.0 - abs(u) - abs(v)), 3.0 * v])         # not unit length
    rows += [[1e-45, z, z], [1e-40, -1e-41, 1e-42], [-1e-45, -1e-45, -1e-45], [z, -1e-45, z], [1e-38, 1e-45, -1e-38]]
    rows += [[3e38, 1.0, 1.0], [1.0, -3e38, 0.5], [3e38, 3e38, z], [-2e38, -2e38, 2e38], [1e30, -1e30, 1e30]]
    rows += [[inf, z, z], [1.0, -inf, z], [inf, inf, inf], [-inf, 1.0, 1.0], [z, z, -inf]]
    rows += [[nan, z, 1.0], [z, nan, z], [1.0, 1.0, nan], [nan, nan, nan], [inf, nan, -inf]]
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((random, 3))
    g /= np.linalg.norm(g, axis=1)[:, None]
    g[random // 2:] *= rng.uniform(0.01, 100.0, (random - random // 2, 1))
    out = np.concatenate([np.array(rows, np.float64), g]).astype(F32)
    out.setflags(write=False)
    return out


def finite_nonzero(d):
    d = np.asarray(d, F32)
    with np.errstate(all="ignore"):
        s = np.abs(d.astype(np.float64)).sum(1)
    return np.isfinite(d).all(1) & (s > 0) & (s < 3.0e38)


# ------------------------------------------------------------------------------------------ the walker's sky seam
@contextmanager
def environment(O, env):
    """while active, path_walker.walk() multiplies a path that meets nothing by color32(env, d) and not by the sky.  Yields the
    list of samples walked, each the list of the direction arrays [k, 3] of its "sky_color" calls, one per segment in order: the
    paths of that sample that ended in the environment at that segment.  env None: the walker's own sky, recorded the same way"""
    import path_walker as WK
    real_contract, real_primary = WK._contract, WK._primary
    samples = []

    def seam(O_, fn, *cols):
        if fn != "sky_color":
            return real_contract(O_, fn, *cols)
        d = np.asarray(cols[0], F32).reshape(-1, 3)
        samples[-1].append(d.copy())
        return color32(O_, env, d) if env is not None else real_contract(O_, fn, *cols)

    def primary(*a, **k):
        samples.append([])
        return real_primary(*a, **k)

    WK._contract, WK._primary = seam, primary
    try:
        yield samples
    finally:
        WK._contract, WK._primary = real_contract, real_primary


def shares(samples, paths_per_sample):
    """(share of all paths that ended in the environment at segment 0, at later segments)"""
    total = float(paths_per_sample * len(samples))
    return sum(len(s[0]) for s in samples if s) / total, sum(sum(len(c) for c in s[1:]) for s in samples) / total


def ended_behind(samples, hits, flags=("mirror", "glass")):
    """how many paths ended in the environment at a segment >= 1 right behind a hit with one of `flags` (path_walker.hit_table's
    columns): the directions of the later "sky_color" calls that are, bit for bit, the direction such a hit left with"""
    sel = np.zeros(len(hits["seg"]), bool)
    for f in flags:
        sel |= hits[f]
    left = {r.tobytes() for r in np.ascontiguousarray(hits["dn"][sel & hits["bounced"]], F32)}
    return sum(r.tobytes() in left for s in samples for c in s[1:] for r in np.ascontiguousarray(c, F32))
