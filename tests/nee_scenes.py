"""Operands and the numpy restatement of the light sample of next-event estimation (csrc/light_sample.hpp) for test_nee_*.py.

sample32 follows light_sample.hpp one float32 operation per device operation, through the pieces of dielectric_scenes (the
contract's dot, cross, normalize and fused multiply-add; numpy's square root, products and division, all correctly rounded): it
is what tests/test_nee_gpu.py holds the device function to, bit for bit.  sample64 is the same estimator in float64 from the
float32 operands as they are.  form_factor is Lambert's closed form for the irradiance of a polygon, in float64: what the mean
of the weight g estimates."""
from functools import lru_cache

import numpy as np

import pathtrace_scenes as P
from dielectric_scenes import _contract, dot, fma, normalize

F32 = np.float32
U32 = np.uint32
K2PI = F32(6.28318548202514648)
MAX_LIGHTS = 1 << 24
SIZES = ((64, 48), (70, 10), (64, 12))


# ------------------------------------------------------------------------------------------ the sample in float32 and float64
def cross(O, a, b):
    return _contract(O, "cross", a, b)


def pick(u_l, L):
    """min(uint32(u_l * float(L)), L - 1)"""
    L = np.asarray(L, np.int64)
    i = (np.asarray(u_l, F32) * L.astype(F32)).astype(F32).astype(np.int64)
    return np.minimum(i, L - 1).astype(U32)


def cases_of(v0, v1, v2, x, nf, u_l, u_a, u_b, L):
    """[n, 19] uint32 words of rtpt_selftest_light_sample's input"""
    n = len(np.asarray(x).reshape(-1, 3))
    f = np.concatenate([np.broadcast_to(np.asarray(a, F32), (n, 3)) for a in (v0, v1, v2, x, nf)] +
                       [np.broadcast_to(np.asarray(a, F32), (n,))[:, None] for a in (u_l, u_a, u_b)], 1).astype(F32)
    return np.ascontiguousarray(np.concatenate([f.view(U32), np.broadcast_to(np.asarray(L, U32), (n,))[:, None]], 1))


def sample32(O, cases, nl=None):
    """[n, 9] uint32 words (y, wd, g, valid as 1.0 / 0.0, the picked entry) of cases [n, 19]: light::pick and light::sample,
    operation by operation.  nl: the light's unit normal where the caller has it; else as its shade record's"""
    c = np.ascontiguousarray(cases, U32).reshape(-1, 19)
    f = c[:, :18].view(F32)
    v0, v1, v2, x, nf = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12:15]
    u_l, u_a, u_b, L = f[:, 15], f[:, 16], f[:, 17], c[:, 18]
    with np.errstate(all="ignore"):
        e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
        cr = cross(O, e1, e2)
        if nl is None:
            nl = normalize(O, cr)                                                                   # raytrace.comp.glsl:150
        su = np.sqrt(u_a).astype(F32)
        b0 = (F32(1.0) - su).astype(F32)
        b1 = (su * (F32(1.0) - u_b).astype(F32)).astype(F32)
        b2 = (su * u_b).astype(F32)
        y = fma(O, v2, b2[:, None], fma(O, v1, b1[:, None], (v0 * b0[:, None]).astype(F32)))
        w = (y - x).astype(F32)
        r2 = dot(O, w, w)
        wd = normalize(O, w)
        cs = dot(O, nf, wd)
        cl = np.abs(dot(O, nl, wd))
        a2 = np.sqrt(dot(O, cr, cr)).astype(F32)
        valid = (cs > 0) & (cl > 0) & (r2 > 0) & (a2 > 0)
        g = (((cs * cl).astype(F32) * (a2 * L.astype(F32)).astype(F32)).astype(F32) / (K2PI * r2).astype(F32)).astype(F32)
    out = np.concatenate([y, wd, g[:, None], valid[:, None].astype(F32)], 1).astype(F32).view(U32)
    return np.ascontiguousarray(np.concatenate([out, pick(u_l, L)[:, None]], 1))


def sample64(cases):
    """the same in float64 from the float32 operands: dict of y, wd, g, valid, cs, cl, pick"""
    c = np.ascontiguousarray(cases, U32).reshape(-1, 19)
    f = c[:, :18].view(F32).astype(np.float64)
    v0, v1, v2, x, nf = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12:15]
    u_a, u_b, L = f[:, 16], f[:, 17], c[:, 18].astype(np.float64)
    with np.errstate(all="ignore"):
        cr = np.cross(v1 - v0, v2 - v0)
        a2 = np.linalg.norm(cr, axis=1)
        nl = cr / a2[:, None]
        su = np.sqrt(u_a)
        y = v0 * (1 - su)[:, None] + v1 * (su * (1 - u_b))[:, None] + v2 * (su * u_b)[:, None]
        w = y - x
        r2 = (w * w).sum(1)
        wd = w / np.sqrt(r2)[:, None]
        cs, cl = (nf * wd).sum(1), np.abs((nl * wd).sum(1))
        valid = (cs > 0) & (cl > 0) & (r2 > 0) & (a2 > 0)
        g = cs * cl * a2 * L / (2 * np.pi * r2)
    return dict(y=y, wd=wd, g=g, valid=valid, cs=cs, cl=cl, pick=np.minimum(np.floor(f[:, 15] * L), L - 1))


def form_factor(polygon, x, n):
    """Lambert's formula: (1 / 2 pi) sum over the edges of angle(v_i - x, v_i+1 - x) * dot(n, unit(cross(v_i - x, v_i+1 - x))),
    float64, |.| of the sum (either winding) — the integral of cos cos' / (pi r^2) over a polygon wholly above x's horizon.
    polygon [m, 3], x and n [k, 3] -> [k]"""
    poly = np.asarray(polygon, np.float64)
    x, n = np.asarray(x, np.float64).reshape(-1, 3), np.asarray(n, np.float64).reshape(-1, 3)
    total = np.zeros(len(x))
    for i in range(len(poly)):
        a, b = poly[i] - x, poly[(i + 1) % len(poly)] - x
        a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
        c = np.cross(a, b)
        s = np.linalg.norm(c, axis=1)
        gamma = np.arctan2(s, (a * b).sum(1))
        total += gamma * (n * (c / s[:, None])).sum(1)
    return np.abs(total) / (2 * np.pi)


def _draw(k):
    return (np.asarray(k, np.float64) * 2.0 ** -24).astype(F32)


# ------------------------------------------------------------------------------------------ operands
TRAPEZOID_Y2 = np.array([(-0.9, 2.0, -0.6), (1.0, 2.0, -0.8), (0.6, 2.0, 0.7), (-0.5, 2.0, 0.4)], np.float64)


def fan(quad):
    """the two triangles (a, b, c), (a, c, d) of a quad, float32 [2, 3, 3]"""
    q = np.asarray(quad, F32)
    return np.stack([q[[0, 1, 2]], q[[0, 2, 3]]])


@lru_cache(maxsize=None)
def seeded_cases(n=4096, seed=41):
    """points uniform in [-1, 1] x [0, 1.2] x [-1, 1] under a trapezoid lamp of two unequal triangles at y = 2, normals within 60
    degrees of up and uniform in solid angle there (the cosine of the tilt uniform in [1/2, 1], the azimuth uniform), draws as
    exact::rng_next returns them, L = 2: [n, 19] words and the index of the triangle each case samples.  With this distribution
    3.8 % of the cases are not valid (the sampled point lies below the tilted surface's horizon) and 1.7 % more have a cosine
    under 1/16; a tilt ANGLE drawn uniformly in [0, 60] degrees tilts less on average and leaves 2.4 % and 1.0 %"""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-1, 1, n), rng.uniform(0, 1.2, n), rng.uniform(-1, 1, n)], 1)
    ct = rng.uniform(0.5, 1.0, n)
    ph = rng.uniform(0, 2 * np.pi, n)
    st = np.sqrt(1 - ct * ct)
    nf = np.stack([st * np.cos(ph), ct, st * np.sin(ph)], 1).astype(F32)
    u = _draw(rng.integers(0, 2 ** 24, (n, 3)))
    tri = fan(TRAPEZOID_Y2)
    which = pick(u[:, 0], np.full(n, 2))
    t = tri[which]
    out = cases_of(t[:, 0], t[:, 1], t[:, 2], x, nf, u[:, 0], u[:, 1], u[:, 2], 2)
    out.setflags(write=False)
    return out, which


@lru_cache(maxsize=None)
def hostile_cases():
    """a degenerate light, x on the light's plane, x behind the surface (the light below the horizon), u_a on 0 and 1 - 2^-24, u_l
    next to 1 with L in {1, 3, 2^24}, r2 at the smallest normal: [n, 19] words"""
    tri = fan(TRAPEZOID_Y2)[0]
    up = F32([0, 1, 0])
    x0 = F32([0.1, 0.2, -0.1])
    rows = []
    us = _draw([0, 1, 2 ** 23, 2 ** 24 - 1])
    for L in (1, 3, MAX_LIGHTS):
        for u_l in us:
            for u_a in us:
                rows.append(cases_of(tri[0], tri[1], tri[2], x0, up, u_l, u_a, _draw(11184811), L))
    ax = (F32([0, 2, 0]), F32([1, 2, 0]), F32([0.5, 2, 0]))                            # along an axis, so that the cross product is 0
    for a, b, c in ((tri[0], tri[0], tri[0]), (ax[0], ax[1], ax[1]), ax):             # exactly (fused, cross(e, e) need not be)
        rows.append(cases_of(a, b, c, x0, up, 0.5, 0.25, 0.75, 1))                     # no area: a point, an edge, three on a line
    rows.append(cases_of(tri[0], tri[1], tri[1], x0, up, 0.5, 0.25, 0.75, 1))          # an edge whose cross product is a rounding's residue
    rows.append(cases_of(tri[0], tri[1], tri[2], F32([0.0, 2.0, 0.0]), up, 0.5, 0.25, 0.75, 1))    # on the light's plane
    rows.append(cases_of(tri[0], tri[1], tri[2], F32([3.0, 2.0, 3.0]), up, 0.5, 0.25, 0.75, 1))    # ... beside the light
    rows.append(cases_of(tri[0], tri[1], tri[2], x0, -up, 0.5, 0.25, 0.75, 1))                     # behind the surface
    rows.append(cases_of(tri[0], tri[1], tri[2], F32([0.0, 3.0, 0.0]), up, 0.5, 0.25, 0.75, 1))    # above the light, facing away
    tiny = F32(2.0 ** -63)                                                                         # r2 = 2^-126 at u_a = 0: y = v0
    unit = (F32([0, 0, 0]), F32([1, 0, 0]), F32([0, 0, 1]))
    rows.append(cases_of(*unit, F32([0, -tiny, 0]), up, 0.5, 0.0, 0.75, 1))
    small = (F32([0, 0, 0]), F32([2.0 ** -40, 0, 0]), F32([0, 0, 2.0 ** -40]))                     # a light of area 2^-81
    rows.append(cases_of(*small, F32([0, -2.0 ** -63, 0]), up, 0.5, 0.0, 0.75, 1))
    rows.append(cases_of(tri[0], tri[1], tri[2], tri[0], up, 0.5, 0.0, 0.75, 1))                   # x on the sampled point: r2 = 0
    out = np.concatenate(rows)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------ the receiver
RECEIVER_CAM = (0.0, 0.0, 3.0)
RECEIVER_SLOPE = 0.5
RECEIVER_KD = (0.5, 0.25, 0.75)
RECEIVER_LAMP = np.array([(0.9, 0.7, 2.0), (2.0, 0.6, 2.0), (1.8, 1.6, 2.0), (1.2, 1.4, 2.0)], np.float64)
RECEIVER_KE = (4.0, 2.0, 8.0)


@lru_cache(maxsize=None)
def receiver():
    """a diffuse quad in the plane z = 0 that fills the frame of a camera at z = 3 (K2's camera looks down -z), lit by an emissive
    trapezoid of two unequal triangles in the plane z = 2, beside the view frustum; pixel_jitter 0, so a pixel's hit point is the
    same in every frame.  Materials: 0 the receiver, 1 the lamp.  Its pixels' hit points are where test_nee_cpu.py takes the mean
    of the weight"""
    quads = [[(-2.3, -1.8, 0.0), (2.3, -1.8, 0.0), (2.3, 1.8, 0.0), (-2.3, 1.8, 0.0)], RECEIVER_LAMP]
    tris, mat = P._with_form("small", np.array(quads, np.float64), np.array([0, 1]))
    materials = P._materials((RECEIVER_KD,), (RECEIVER_KE,))
    return P.Scene("receiver", "small", tris, RECEIVER_CAM, RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)
