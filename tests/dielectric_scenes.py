"""Operands, scenes, material records, the contract functions on arrays and the numpy restatement of the dielectric interface
(csrc/dielectric.hpp) for test_dielectric_*.py; the path walker that uses them is tests/path_walker.py.

refract32 follows the arithmetic as dielectric.hpp states it, one float32 operation per device operation: dot and normalize
through the oracle's statement of the numerics contract (oracle.contract_array), every fused multiply-add through the contract's
dot as well (fma below: exact, where texture_scenes.fma32 rounds twice), the square root, the products, the differences and the
two divisions of the record in numpy float32 (all correctly rounded, like the device's).  refract64 is the same interface in
float64 libm from the float32 operands as they are.

_rng_next and _primary are the walker's random stream and primary-ray generation (csrc/pathtrace_tile.hpp).  The oracle knows no
dielectric, so path_walker.walk is the reference of the dielectric frames — after tests/test_dielectric_cpu.py has held it to
oracle.raytrace_ext on scenes without one, IMAGE and HIT_ID bit for bit."""
import os
from functools import lru_cache

import numpy as np

import contract_cases as CC
import pathtrace_scenes as P
import specular_scenes as S
from gbuffer_scenes import fill_push_constants

F32 = np.float32
SIZES = S.SIZES
GLASS_IOR = 1.5
GLASS_COLOUR = (1.0, 0.5, 0.25)


# ------------------------------------------------------------------------------------------ contract functions on arrays
def _contract(O, fn, *cols):
    n = len(np.asarray(cols[0]))
    if n == 0:
        return np.zeros((0, O.contract_words(CC.fn_index(fn))[1]), F32)
    w = np.ascontiguousarray(np.concatenate([np.asarray(c, F32).reshape(n, -1) for c in cols], 1)).view(np.uint32)
    return O.contract_array(CC.fn_index(fn), w).view(F32)


def dot(O, a, b):
    return _contract(O, "dot", a, b)[:, 0]


def normalize(O, v):
    return _contract(O, "normalize", v)


def fma(O, a, b, c):
    """fmaf(a, b, c) per element, one rounding: the contract's dot((c, a, 0), (1, b, -0)) = fma(0, -0, fma(a, b, c * 1)) — c * 1 is
    c, and adding the product -0 changes no value and no zero's sign"""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    shape = a.shape
    a, b, c = a.ravel(), b.ravel(), c.ravel()
    zero = np.zeros_like(a)
    left = np.stack([c, a, zero], 1)
    right = np.stack([np.ones_like(a), b, -zero], 1)
    return dot(O, left, right).reshape(shape)


# ------------------------------------------------------------------------------------------ the interface in float32 and float64
def record_values(ior):
    """(inv, R0) as the host computes them for the record, binary32"""
    ior = np.asarray(ior, F32)
    with np.errstate(all="ignore"):
        inv = (F32(1.0) / ior).astype(F32)
        q = ((ior - F32(1.0)).astype(F32) / (ior + F32(1.0)).astype(F32)).astype(F32)
        return inv, (q * q).astype(F32)


def interface32(O, n, d, u1, ior, inv, r0):
    """diel::interface after the side is taken from the STORED normal n: (d' [k, 3], transmitted [k] bool, F [k], nf [k, 3])"""
    with np.errstate(all="ignore"):
        entering = dot(O, n, d) < 0
        nf = np.where(entering[:, None], n, -n).astype(F32)
        eta = np.where(entering, inv, ior).astype(F32)
        ci = (-dot(O, nf, d)).astype(F32)
        s2 = ((eta * eta).astype(F32) * fma(O, -ci, ci, F32(1.0))).astype(F32)
        k = (F32(1.0) - s2).astype(F32)
        tir = ~(k > 0)
        ct = np.sqrt(np.where(tir, F32(0.0), k)).astype(F32)
        x = (F32(1.0) - np.where(entering, ci, ct)).astype(F32)
        x2 = (x * x).astype(F32)
        x5 = ((x2 * x2).astype(F32) * x).astype(F32)
        fres = np.where(tir, F32(1.0), fma(O, (F32(1.0) - r0).astype(F32), x5, r0)).astype(F32)
        reflect = tir | (u1 < fres)
        refl = fma(O, ((F32(2.0) * ci).astype(F32))[:, None], nf, d)
        a = fma(O, eta, ci, -ct)
        trans = fma(O, a[:, None], nf, (eta[:, None] * d).astype(F32))
        dn = normalize(O, np.where(reflect[:, None], refl, trans).astype(F32))
    return dn, ~reflect, fres, nf


def refract32(O, cases):
    """[n, 5] float32 (d', 1.0 if transmitted else 0.0, F) of cases [n, 9] = d, n, u1, u2, ior: diel::refract, operation by operation"""
    c = np.ascontiguousarray(cases, F32).reshape(-1, 9)
    inv, r0 = record_values(c[:, 8])
    dn, transmitted, fres, _ = interface32(O, c[:, 3:6], c[:, 0:3], c[:, 6], c[:, 8], inv, r0)
    return np.concatenate([dn, transmitted[:, None].astype(F32), fres[:, None]], 1).astype(F32)


def refract64(cases):
    """the same interface in float64 from the float32 operands as they are: dict of d' [n, 3], transmitted [n], F [n], k [n]
    (1 - eta^2 sin^2: <= 0 is total internal reflection) and u1 - F [n]"""
    c = np.asarray(cases, np.float64).reshape(-1, 9)
    d, n, u1, ior = c[:, 0:3], c[:, 3:6], c[:, 6], c[:, 8]
    with np.errstate(all="ignore"):
        entering = (n * d).sum(1) < 0
        nf = np.where(entering[:, None], n, -n)
        eta = np.where(entering, 1.0 / ior, ior)
        ci = -(nf * d).sum(1)
        k = 1.0 - eta * eta * (1.0 - ci * ci)
        tir = ~(k > 0)
        ct = np.sqrt(np.where(tir, 0.0, k))
        r0 = ((ior - 1.0) / (ior + 1.0)) ** 2
        fres = np.where(tir, 1.0, r0 + (1.0 - r0) * (1.0 - np.where(entering, ci, ct)) ** 5)
        reflect = tir | (u1 < fres)
        v = np.where(reflect[:, None], d + 2.0 * ci[:, None] * nf, eta[:, None] * d + (eta * ci - ct)[:, None] * nf)
        dn = v / np.linalg.norm(v, axis=1, keepdims=True)
    return dict(d=dn, transmitted=~reflect, F=fres, k=k, margin=u1 - fres)


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def _draw(k):
    return (np.asarray(k, np.float64) * 2.0 ** -24).astype(F32)


HOSTILE_IOR = (1.0, 1.0 + 2.0 ** -23, 1.5, 2.4170000553131104, 1e6, 1e18)
HUGE_IOR = 1e3
# the sine of the angle of incidence relative to the critical one's: at it, at its two float32 neighbours' distance from it (k
# stays within the tests' bar of 0, where total reflection is a rounding's choice) and a quarter to either side, where float64
# decides.  In between, k = 1 - eta^2 sin^2 carries the cosine's roundings scaled by 2 eta^2, ct = sqrt(k) those divided by 2 ct,
# and F five times ct's: binary32's F is then further from float64's than the bar of 2^-20 (measured: 1.5e-6 at ior 2.417, ct =
# 0.18), so a row with u1 at F there compares two roundings of F, not the choice.  The seeded set samples that range.
CRITICAL_SIDES = (0.0, 2.0 ** -23, -2.0 ** -23, 0.25, -0.25)


def _frames():
    """unit normals with a tangent each"""
    out = []
    for n in ((0, 0, 1), (0, 1, 0), (1, 2, 3), (-0.3, 0.9, 0.1)):
        n64 = np.asarray(n, np.float64) / np.linalg.norm(n)
        t = np.cross(n64, (0.3, -0.5, 0.8))
        out.append((n64, t / np.linalg.norm(t)))
    return out


@lru_cache(maxsize=None)
def _hostile_geometry():
    """(d, n, ior) rows: normal incidence from either side, grazing incidence, n . d = 0 exactly, from inside at, next to and on
    either side of the critical angle, for ior 1, 1 + ulp, glass, diamond and two huge ones whose square is still finite.
    From inside, k = 1 - ior^2 sin^2 carries the roundings of the cosine scaled by ior^2: within a cone of about 1 / ior around the
    normal the last bits of the float32 operands (unit vectors to 2^-24) decide between transmission and total reflection in any
    precision.  A huge ior therefore meets the interface along the normal only where that is exact in every format (an
    axis-aligned normal: sin^2 = 0) and otherwise far outside that cone, and has no row at its critical angle of 1 / ior radians."""
    rows = []
    for n64, t in _frames():
        n = n64.astype(F32)
        for ior in HOSTILE_IOR:
            for side in (-1.0, 1.0):                                   # -1: the ray meets the front (entering), +1: the back
                if ior < HUGE_IOR or np.count_nonzero(n) == 1:
                    rows.append((_unit(side * n64), n, ior))           # normal incidence
                for eps in (2.0 ** -20, 2.0 ** -12, 2.0 ** -4, 0.5):   # |n . d| is about eps: grazing and on the way there
                    rows.append((_unit(t * np.sqrt(1 - eps * eps) + side * eps * n64), n, ior))
            if 1.0 < ior < HUGE_IOR:                                    # from inside: sin(critical) = 1 / ior
                for rel in CRITICAL_SIDES:
                    s = min(1.0, (1.0 / ior) * (1.0 + rel))
                    rows.append((_unit(t * s + np.sqrt(max(0.0, 1 - s * s)) * n64), n, ior))
    rows.append((F32([1, 0, 0]), F32([0, 0, 1]), 1.5))                 # n . d = 0 in every format
    rows.append((F32([0, -1, 0]), F32([0, 1, 0]), 1.5))
    rows.append((F32([0, 1, 0]), F32([0, 1, 0]), 1.5))
    return rows


def hostile_cases(O):
    """the hostile geometry with u1 on 0, 1 ulp, the middle, just below 1 and 1, and then — F taken from refract32 — with u1
    equal to F and to its two float32 neighbours"""
    geo = _hostile_geometry()
    u1s = _draw([0, 1, 2 ** 23, 2 ** 24 - 1, 2 ** 24])
    rows = [np.concatenate([d, n, [a, b, ior]]) for d, n, ior in geo for a in u1s for b in _draw([0, 11184811])]
    base = np.array([np.concatenate([d, n, [0.5, 0.25, ior]]) for d, n, ior in geo], F32)
    fres = refract32(O, base)[:, 4]
    for u in (fres, np.nextafter(fres, F32(-1.0)), np.nextafter(fres, F32(2.0))):
        at = base.copy()
        at[:, 6] = u
        rows += list(at)
    out = np.array(rows, F32)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def seeded_cases(n=4096, seed=37):
    """random unit normals and directions (half of them meet the back: from inside), draws as exact::rng_next returns them, ior
    from glass-like values, 1 and uniform ones in [1, 3]"""
    rng = np.random.default_rng(seed)
    nn = _unit(rng.normal(size=(n, 3)))
    dd = _unit(rng.normal(size=(n, 3)))
    u = _draw(rng.integers(0, 2 ** 24, (n, 2)))
    ior = np.where(rng.random(n) < 0.5, rng.choice(F32([1.0, 1.33, 1.5, 2.417]), n), (1.0 + 2.0 * rng.random(n)).astype(F32)).astype(F32)
    out = np.concatenate([dd, nn, u, ior[:, None]], 1).astype(F32)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------ material records
def records(scene, specular=None, dielectric=None):
    """[t, 8] float32, the device's per-triangle records (material_host.hpp pack_records_mode): (Kd, 0)(Ke, emissive), (Ks, -g)(0 0 0
    0), (colour, ior)(1 / ior, R0, 0, 0)"""
    mats = np.asarray(scene.materials, F32).reshape(-1, 6)
    rec = np.zeros((len(mats), 8), F32)
    rec[:, 0:3], rec[:, 4:7] = mats[:, 0:3], mats[:, 3:6]
    rec[:, 7] = (mats[:, 3:6] != 0).any(1)
    for m, (ks, g) in (specular or {}).items():
        rec[m] = (*F32(ks), -F32(g), 0, 0, 0, 0)
    for m, (colour, ior) in (dielectric or {}).items():
        inv, r0 = record_values(F32(ior))
        rec[m] = (*F32(colour), F32(ior), inv, r0, 0, 0)
    return rec[np.asarray(scene.tri_material, np.int64)]


# ------------------------------------------------------------------------------------------ the walker's stream and primary rays
def _rng_next(O, state):
    """(new state [k] uint32, float [k]) of exact::rng_next"""
    w = O.contract_array(CC.fn_index("rng_next_skip"), np.ascontiguousarray(state, np.uint32).reshape(-1, 1))
    return w[:, 0].copy(), w[:, 1].copy().view(F32)


def _primary(O, cfg, rng, xs, ys):
    """(rng state after the jitter's two draws [k] uint32, primary direction [k, 3]) of pixels (xs, ys) whose stream stands at
    `rng`: raytrace.comp.glsl:314-320"""
    k = len(xs)
    slope, jitter, fw, fh = F32(cfg.fov_slope), F32(cfg.pixel_jitter), F32(cfg.width), F32(cfg.height)
    rng, g1 = _rng_next(O, rng)
    rng, g2 = _rng_next(O, rng)
    g1 = _contract(O, "minmax", np.full(k, 1e-38, F32), g1)[:, 1]
    r = np.sqrt((F32(-2.0) * _contract(O, "log", g1)[:, 0]).astype(F32)).astype(F32)
    sc = _contract(O, "sincos2pi", g2)
    gx, gy = (r * sc[:, 1]).astype(F32), (r * sc[:, 0]).astype(F32)
    cx = fma(O, jitter, gx, (xs.astype(F32) + F32(0.5)).astype(F32))
    cy = fma(O, jitter, gy, (ys.astype(F32) + F32(0.5)).astype(F32))
    ux = (fma(O, F32(2.0), cx, -fw) / fh).astype(F32)
    uy = (-(fma(O, F32(2.0), cy, -fh) / fh)).astype(F32)
    d = normalize(O, np.stack([(slope * ux).astype(F32), (slope * uy).astype(F32), np.full(k, -1.0, F32)], 1))
    return rng, d


def primary_rays(O, scene, W, H, frame=0):
    """(rng state behind the jitter [H, W] uint32, direction [H, W, 3]) of every pixel's primary ray, as path_walker.walk forms them"""
    cfg = P.configure(O.config_default(W, H), scene, 1, 1)
    pc = fill_push_constants(O.PushConstants(), P.push_constants(scene), frame)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xs, ys = xs.ravel().astype(np.uint32), ys.ravel().astype(np.uint32)
    seeds = np.stack([xs, ys, np.full(W * H, pc.frameNumber, np.uint32), np.full(W * H, pc.sample_batch, np.uint32)], 1)
    rng = O.contract_array(CC.fn_index("rng_seed"), np.ascontiguousarray(seeds, np.uint32))[:, 0].copy()
    rng, d = _primary(O, cfg, rng, xs, ys)
    return rng.reshape(H, W), d.reshape(H, W, 3)


def stored_normals(O, tris):
    """[t, 3]: the unit normal the device stores per triangle, normalize(cross(v1 - v0, v2 - v0)) (:150)"""
    tri = np.asarray(tris, F32).reshape(-1, 9)
    return normalize(O, _contract(O, "cross", (tri[:, 3:6] - tri[:, 0:3]).astype(F32), (tri[:, 6:9] - tri[:, 0:3]).astype(F32)))


def oracle_ext_frame(O, scene, W, H, segments, specular=None, frame=0, rows=None, spp=1):
    """oracle.raytrace_ext of a scene whose materials are diffuse or specular: IMAGE, HIT_ID, rays"""
    cfg = P.configure(O.config_default(W, H), scene, segments, spp)
    pc = fill_push_constants(O.PushConstants(), P.push_constants(scene), frame)
    y0, y1 = rows or (0, H)
    r = O.raytrace_ext(cfg, pc, scene.tris, O.material_records_ext(scene.tri_material, scene.materials, specular), y0=y0, y1=y1,
                       specular=True, records=False, dump=False)
    return dict(IMAGE=r["IMAGE"], HIT_ID=r["HIT_ID"], rays=r["rays"])


# ------------------------------------------------------------------------------------------ scenes
@lru_cache(maxsize=None)
def glass_quad():
    """specular_scenes.mirror_quad's geometry as glass, ior 1.5, colour (1, 1/2, 1/4): (scene, {material: (colour, ior)})"""
    sc, _ = S.mirror_quad()
    return sc._replace(name="glass_quad"), {0: (GLASS_COLOUR, GLASS_IOR)}


BEHIND_CAM = (-6.5, 1.0, 6.0)
BEHIND_SIZE = (64, 12)


@lru_cache(maxsize=None)
def glass_quad_from_behind():
    """the same quad with its winding reversed, so that its stored normal points away from the camera — the camera is inside the
    medium and meets the interface from behind — seen from far to the left in a frame of BEHIND_SIZE, seven times wider than
    tall: K2's camera looks down -z, so only rays of the frame's right part meet the quad, more than 38 degrees off the axis,
    and the quad's tilt of 30 degrees about x leaves every one of them beyond the critical angle of 41.8 degrees (asserted on
    float64's k where this scene is used)"""
    sc, glass = glass_quad()
    tris = P._frozen(np.asarray(sc.tris)[:, [0, 1, 2, 6, 7, 8, 3, 4, 5]])
    return sc._replace(name="glass_quad_behind", tris=tris, cam=BEHIND_CAM), glass


BOX_LO, BOX_HI = (-0.9, -1.0 + 0.05, -2.4), (0.3, 0.1, -1.2)
LAMP_KE = (6.0, 5.0, 4.0)


@lru_cache(maxsize=None)
def glass_room(form="small"):
    """pathtrace_scenes' closed room (six diffuse walls, the camera inside) with a closed glass box standing in it, its faces'
    normals pointing outwards, and a lamp quad under the ceiling: (scene, {material: (colour, ior)}).  Materials 0..5 the walls, 6
    the glass, 7 the lamp.  small: 6 + 6 + 1 quads = 26 triangles; pairs: every quad 3 x 3 = 234 triangles, all fan pairs"""
    walls = P._box_quads(*P.ROOM)
    box = P._box_quads(BOX_LO, BOX_HI)               # _box_quads winds every face so that its normal points out of the box
    lamp = np.array([[(0.4, 0.99, -1.4), (1.2, 0.99, -1.4), (1.2, 0.99, -0.6), (0.4, 0.99, -0.6)]], np.float64)
    quads = np.concatenate([walls, box, lamp])
    qmat = np.array([0, 1, 2, 3, 4, 5] + [6] * 6 + [7])
    if form != "small":
        quads, src = P._tessellate(quads, 3)
        qmat = qmat[src]
    tris, mat = P._with_form(form, quads, qmat)
    materials = P._materials(P.WALL_KD + ((0.5, 0.5, 0.5),), (LAMP_KE,))
    sc = P.Scene("glass_room", form, tris, P.ROOM_CAM, P.REF_SLOPE, 0.375, P.LIGHT_FAR, 0.2, mat, materials)
    return sc, {6: ((0.75, 0.875, 1.0), GLASS_IOR)}


def with_far_glass_pair(scene):
    """specular_scenes.with_far_pair, the pair's material to be made glass: (scene, material index)"""
    return S.with_far_pair(scene)


# ------------------------------------------------------------------------------------------ files for the loader / hosts
MTL_NI = """\
newmtl glass4
Ks 0.9 0.8 0.7
Ni 1.5
illum 4
newmtl glass6
Ks 0.5 0.5 0.5
Ns 100
Ni 1.33
illum 6
newmtl glass7tf
Ks 0.9 0.8 0.7
Tf 0.25 0.5 0.75
Ni 2.417
illum 7
newmtl glass9
Ks 1 1 1
Ni 1
illum 9
newmtl mirror4
Ks 0.9 0.8 0.7
illum 4
newmtl mirror6
Ks 0.5 0.5 0.5
Ns 100
illum 6
newmtl mirror7
Ks 0.9 0.8 0.7
Tf 0.25 0.5 0.75
illum 7
newmtl mirror9
Ks 1 1 1
illum 9
newmtl mirror3ni
Ks 0.9 0.8 0.7
Ni 1.5
illum 3
newmtl thin
Ks 0.9 0.8 0.7
Ni 0.5
illum 7
newmtl tfblack
Ks 0.9 0.8 0.7
Tf 0 0 0
Ni 1.5
illum 7
newmtl tfonly
Tf 0.25 0.5 0.75
Ni 1.5
illum 7
newmtl lamp
Ks 0.9 0.8 0.7
Ke 4 3 2
Ni 1.5
illum 7
newmtl broken
Ks 0.9 0.8 0.7
Tf 0.25 0.5
Ni
Ni x
illum 7
newmtl brokenni
Ks 0.9 0.8 0.7
Ni nan
illum 7
newmtl diffuse2
Kd 0.1 0.2 0.3
Ni 1.5
illum 2
"""
OBJ_NI = "mtllib lib.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3\nusemtl glass4\nf 1 2 3 4\nusemtl glass7tf\nf 1 2 3\n" \
         "usemtl nobody\nf 1 2 3\nusemtl lamp\nf 2 3 4\n"


def write_glass_room(directory):
    """room.obj + room.mtl in `directory`: specular_scenes.write_specular_room's room with its satin panel made a glass pane
    (illum 7, Ni 1.5, Tf) in front of the back wall, both faces' worth of one quad.  Returns the OBJ's path"""
    with open(os.path.join(directory, "room.mtl"), "w") as f:
        f.write("newmtl wall\nKd 0.8 0.7 0.6\n"
                "newmtl floor\nKd 0.6 0.6 0.7\n"
                "newmtl mirror\nKd 0.1 0.1 0.1\nKs 0.9 0.9 0.95\nillum 3\n"
                "newmtl gloss\nKd 0.1 0.1 0.1\nKs 0.7 0.5 0.3\nNs 40\nillum 3\n"
                "newmtl pane\nKd 0.2 0.6 0.3\nKs 1 1 1\nTf 0.9 0.95 1.0\nNi 1.5\nillum 7\n"
                "newmtl lamp\nKd 0 0 0\nKe 4 3 2\n")
    with open(os.path.join(directory, "room.obj"), "w") as f:
        f.write("mtllib room.mtl\n"
                "v -2 -0.2 -1\nv 2 -0.2 -1\nv 2 2.4 -1\nv -2 2.4 -1\n"
                "v -2 -0.2 3\nv 2 -0.2 3\n"
                "v -1.6 0.2 0.6\nv -0.2 0.1 0.1\nv -0.1 1.5 -0.3\nv -1.5 1.6 0.2\n"
                "v 0.3 -0.19 0.2\nv 1.7 -0.19 0.2\nv 1.7 -0.19 2.4\nv 0.3 -0.19 2.4\n"
                "v 0.4 0.4 0.3\nv 1.4 0.3 0.1\nv 1.5 1.3 -0.1\nv 0.5 1.4 0.2\n"
                "v 1.0 1.8 -0.9\nv 1.5 1.8 -0.9\nv 1.5 2.2 -0.9\nv 1.0 2.2 -0.9\n"
                "usemtl wall\nf 1 2 3 4\n"
                "usemtl floor\nf 5 6 2 1\n"
                "usemtl mirror\nf 7 8 9 10\n"
                "usemtl gloss\nf 11 14 13 12\n"
                "usemtl pane\nf 15 16 17 18\n"
                "usemtl lamp\nf 19 20 21 22\n")
    return os.path.join(directory, "room.obj")
