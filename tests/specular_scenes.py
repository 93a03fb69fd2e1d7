"""Scenes, operands and the numpy restatement of the specular bounce (csrc/specular.hpp) for test_specular_*.py.

The restatement follows the arithmetic as specular.hpp states it, one float32 operation per device operation: the fused
multiply-adds through fma32 of tests/texture_scenes.py, dot / normalize / sincos2pi through the oracle's statement of the
numerics contract (oracle.contract_array, the way tests/test_contract_gpu.py reaches them), the square root and the plain
products in numpy float32 (both correctly rounded, like the device's).

The scenes reuse tests/pathtrace_scenes.py: the closed room with mirror walls (closed form: every path lives to the bound and
its colour is a power of two), a mirror quad under the sky (the direction, end to end), the closed room and the trench with
diffuse and specular surfaces side by side (paths absorbed at different segments: schedule independence)."""
from functools import lru_cache

import numpy as np

import contract_cases as CC
import pathtrace_scenes as P
from texture_scenes import fma32

F32 = np.float32
SIZES = ((64, 48), (70, 10))


# ------------------------------------------------------------------------------------------ the bounce in numpy float32
def _contract(O, fn, *cols):
    w = np.ascontiguousarray(np.concatenate([np.asarray(c, F32).reshape(len(cols[0]), -1) for c in cols], 1)).view(np.uint32)
    return O.contract_array(CC.fn_index(fn), w).view(F32)


def dot32(O, a, b):
    return _contract(O, "dot", a, b)[:, 0]


def bounce32(O, cases):
    """[n, 4] float32 (d', 1.0 if absorbed else 0.0) of cases [n, 9] = d, n, u1, u2, g: spec::bounce, operation by operation"""
    cases = np.ascontiguousarray(cases, F32).reshape(-1, 9)
    d, n, u1, u2, g = cases[:, 0:3], cases[:, 3:6], cases[:, 6], cases[:, 7], cases[:, 8]
    flip = ~(dot32(O, n, d) < 0)                                   # faceforward
    n = np.where(flip[:, None], -n, n)
    c2 = (F32(-2.0) * dot32(O, n, d)).astype(F32)
    r = fma32(c2[:, None], n, d)                                   # the mirror direction
    sc = _contract(O, "sincos2pi", u1)
    sn, cs = sc[:, 0], sc[:, 1]
    u = fma32(F32(2.0), u2, F32(-1.0))
    rho = np.sqrt(fma32(-u, u, F32(1.0))).astype(F32)
    s = np.stack([(rho * cs).astype(F32), (rho * sn).astype(F32), u], 1)
    dn = _contract(O, "normalize", fma32(g[:, None], s, r))
    absorbed = ~(dot32(O, n, dn) > 0)
    return np.concatenate([dn, absorbed[:, None].astype(F32)], 1).astype(F32)


def bounce64(cases):
    """the same bounce in float64 from the float32 operands as they are: (d' [n, 3], n . d' [n], |r + g s| [n])"""
    c = np.asarray(cases, np.float64).reshape(-1, 9)
    d, n, u1, u2, g = c[:, 0:3], c[:, 3:6], c[:, 6], c[:, 7], c[:, 8]
    nd = (n * d).sum(1)
    n = np.where((~(nd < 0))[:, None], -n, n)
    r = d - 2.0 * (n * d).sum(1)[:, None] * n
    u = 2.0 * u2 - 1.0
    rho = np.sqrt(np.maximum(1.0 - u * u, 0.0))
    s = np.stack([rho * np.cos(2 * np.pi * u1), rho * np.sin(2 * np.pi * u1), u], 1)
    v = r + g[:, None] * s
    ln = np.linalg.norm(v, axis=1)
    dn = v / np.maximum(ln, 1e-300)[:, None]
    return dn, (n * dn).sum(1), ln


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def _draw(k):
    """an RNG float: a multiple of 2^-24 in [0, 1], as exact::rng_next returns them (1.0 itself only as a hostile operand)"""
    return (np.asarray(k, np.float64) * 2.0 ** -24).astype(F32)


HOSTILE_G = (0.0, 2.0 ** -24, 1.0)


@lru_cache(maxsize=None)
def hostile_cases():
    """grazing d, n . d = 0 exactly, n . d > 0 (the back of the triangle), axis-aligned and oblique normals; u2 at 0 and 1 (u = -1, +1:
    the sphere's poles, rho = 0), u1 on the quarter turns and next to them; g in {0, 2^-24, 1}"""
    ns = [_unit(v) for v in ((0, 0, 1), (0, 1, 0), (1, 0, 0), (1, 2, 3), (-0.3, 0.9, 0.1))]
    pairs = []
    for n in ns:
        n64 = n.astype(np.float64)
        t = np.cross(n64, (0.3, -0.5, 0.8))
        t /= np.linalg.norm(t)
        b = np.cross(n64, t)
        for eps in (0.0, 2.0 ** -20, -2.0 ** -20, 2.0 ** -12, -2.0 ** -12, 0.5, -0.5, 1.0, -1.0):      # n . d is about -eps
            for w in (t, b, 0.6 * t - 0.8 * b):
                pairs.append((_unit(w * np.sqrt(max(0.0, 1 - eps * eps)) - eps * n64), n))
    pairs.append((F32([1, 0, 0]), F32([0, 0, 1])))      # n . d = 0 in every format
    pairs.append((F32([0, -1, 0]), F32([0, 1, 0])))     # straight down onto the surface
    pairs.append((F32([0, 1, 0]), F32([0, 1, 0])))      # ... and onto its back
    u1s = _draw([0, 1, 2 ** 22, 2 ** 22 + 1, 2 ** 23, 3 * 2 ** 22 - 1, 2 ** 24 - 1, 5592405])
    u2s = _draw([0, 1, 2 ** 23, 2 ** 24 - 1, 2 ** 24, 11184811])
    rows = [np.concatenate([d, n, [a, b, g]]) for d, n in pairs for a in u1s for b in u2s for g in HOSTILE_G]
    out = np.array(rows, F32)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def seeded_cases(n=4096, seed=31):
    rng = np.random.default_rng(seed)
    nn = _unit(rng.normal(size=(n, 3)))
    dd = _unit(rng.normal(size=(n, 3)))
    u = _draw(rng.integers(0, 2 ** 24, (n, 2)))
    g = np.where(rng.random(n) < 0.25, rng.choice(F32(HOSTILE_G), n), rng.random(n).astype(F32)).astype(F32)
    out = np.concatenate([dd, nn, u, g[:, None]], 1).astype(F32)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------ scenes: (scene, {material: (Ks, g)})
MIRROR_KS = (0.5, 0.25, 0.125)


@lru_cache(maxsize=None)
def mirror_room(form="small"):
    """the closed room of pathtrace_scenes, every wall a perfect mirror with Ks = (1/2, 1/4, 1/8): (scene, {material: (Ks, g)})"""
    sc = P.closed_room(form)
    return sc._replace(name="mirror_room"), {m: (MIRROR_KS, 0.0) for m in range(len(sc.materials))}


MIXED_G = {1: 0.0, 3: 0.3, 5: 1.0}      # walls +x, +y, +z are specular; -x, -y, -z stay diffuse


@lru_cache(maxsize=None)
def mixed_room(form="small"):
    """the closed room with walls alternating diffuse and specular (Ks = the wall's Kd, powers of two)"""
    sc = P.closed_room(form)
    return sc._replace(name="mixed_room"), {m: (P.WALL_KD[m], g) for m, g in MIXED_G.items()}


@lru_cache(maxsize=None)
def glossy_trench(form="small"):
    """three_ends with its floor (material 0) specular, g = 0.3, Ks = its Kd"""
    sc = P.three_ends(form)
    return sc._replace(name="glossy_trench"), {0: (tuple(sc.materials[0, :3]), 0.3)}


def with_far_pair(scene):
    """the scene plus one tiny fan pair behind the camera (the camera looks down -z), three scene extents away: outside the closed
    rooms, where no path can reach it; seen from an open scene under a solid angle of about 1e-8 steradians.  Its material is
    a new last row of the table: (scene with the two triangles, index of that row)"""
    cam = np.asarray(scene.cam, np.float64)
    extent = float(np.abs(np.asarray(scene.tris, np.float64).reshape(-1, 3) - cam).max())
    c, h = cam + (0.0, 0.0, 3.0 * extent), 1e-4 * extent
    quad = [c + (-h, -h, 0), c + (h, -h, 0), c + (h, h, 0), c + (-h, h, 0)]
    tris = np.concatenate([scene.tris, P._quad_tris([quad])])
    m = len(scene.materials)
    mat = np.concatenate([scene.tri_material, np.array([m, m], np.uint32)])
    materials = np.concatenate([scene.materials, F32([[0.5, 0.5, 0.5, 0, 0, 0]])])
    return scene._replace(tris=P._frozen(tris), tri_material=P._frozen(mat, np.uint32), materials=P._frozen(materials)), m


# ------------------------------------------------------------------------------------------ the mirror quad under the sky
QUAD_CAM = (0.0, 1.0, 6.0)
QUAD_KS = (1.0, 0.5, 0.25)
QUAD_TILT = np.deg2rad(30.0)                  # the normal is (0, sin, cos): reflected rays of the frame go up
QUAD_LIGHT = (0.0, -5000.0, 0.0)              # straight below: no primary ray and no reflected ray points there
QUAD_HALF = (1.37, 0.91)                      # odd extents: no pixel centre's ray meets an edge


def quad_frame():
    """centre, the unit axes a (along x) and b (up the slope), the unit normal"""
    return np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, np.cos(QUAD_TILT), -np.sin(QUAD_TILT)]), \
        np.array([0.0, np.sin(QUAD_TILT), np.cos(QUAD_TILT)])


@lru_cache(maxsize=None)
def mirror_quad():
    c, a, b, _ = quad_frame()
    ha, hb = QUAD_HALF
    quad = [c - ha * a - hb * b, c + ha * a - hb * b, c + ha * a + hb * b, c - ha * a + hb * b]
    tris = P._frozen(P._quad_tris([quad]))
    sc = P.Scene("mirror_quad", "small", tris, QUAD_CAM, P.REF_SLOPE, 0.0, QUAD_LIGHT, 0.2, P._frozen([0, 0], np.uint32),
                 P._frozen(F32([[0.7, 0.7, 0.7, 0, 0, 0]])))
    return sc, {0: (QUAD_KS, 0.0)}


def sky64(d):
    """sky_color (raytrace.comp.glsl:95-107) in float64"""
    t = d[..., 1:2]
    up = np.concatenate([0.25 * t + (1 - t), 0.5 * t + (1 - t), t + (1 - t)], -1)
    return np.where(t > 0, up, 0.03)


def mirror_quad_expectation(W, H):
    """float64 restatement of K2's jitter-free ray through every pixel centre (raytrace.comp.glsl:314-320), met with the quad's
    plane and reflected: (on [H, W] bool: the ray meets the quad; colour [H, W, 3] = Ks * sky(reflect(d)) there)"""
    c, a, b, n = quad_frame()
    cam = np.asarray(QUAD_CAM, np.float64)
    cx, cy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    ux, uy = (2 * cx - W) / H, -(2 * cy - H) / H
    d = np.stack([P.REF_SLOPE * ux, P.REF_SLOPE * uy, -np.ones_like(ux)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    t = ((c - cam) @ n) / (d @ n)
    p = cam + t[..., None] * d - c
    on = (t > 0) & (np.abs(p @ a) < QUAD_HALF[0]) & (np.abs(p @ b) < QUAD_HALF[1])
    r = d - 2.0 * (d @ n)[..., None] * n
    assert (r[on][:, 1] > 0.3).all(), "reflected rays go up, well clear of the horizon"
    return on, np.asarray(QUAD_KS, np.float64) * sky64(r)


# ------------------------------------------------------------------------------------------ what the device measured
# pixels of MAIN_SHAPE whose path ends absorbed (IMAGE exactly 0, ALBEDO != 0) at 33 segments, frame 0, single launch, measured on
# an MI355X (tests/test_specular_gpu.py asserts at least half of each)
ABSORBED = {("mixed_room", "small"): 2342, ("glossy_trench", "small"): 227}


# ------------------------------------------------------------------------------------------ files for the loader / hosts
MTL_RULE = """\
newmtl diffuse2
Kd 0.1 0.2 0.3
Ks 0.5 0.5 0.5
Ns 1000
illum 2
newmtl mirror3
Kd 0.4 0.4 0.4
Ks 0.9 0.8 0.7
illum 3
newmtl rough5
Ks 0.5 0.25 0.125
Ns 0
illum 5
newmtl gloss3
Ks 1 1 1
Ns 1000
illum 3
newmtl black3
Kd 0.3 0.2 0.1
Ks 0 0 0
Ns 10
illum 3
newmtl lamp
Kd 0 0 0
Ke 4 3 2
"""
MTL_RULE_PLAIN = "newmtl diffuse2\nKd 0.1 0.2 0.3\nnewmtl mirror3\nKd 0.4 0.4 0.4\nnewmtl rough5\nnewmtl gloss3\nnewmtl black3\n" \
                 "Kd 0.3 0.2 0.1\nnewmtl lamp\nKd 0 0 0\nKe 4 3 2\n"
OBJ_RULE = "mtllib lib.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nf 1 2 3\nusemtl mirror3\nf 1 2 3 4\nusemtl gloss3\nf 1 2 3\n" \
           "usemtl nobody\nf 1 2 3\nusemtl lamp\nf 2 3 4\n"


def write_specular_room(directory):
    """room.obj + room.mtl in `directory`: a diffuse back wall and floor, a tilted mirror panel (illum 3, no Ns), a glossy floor
    strip (illum 3, Ns 40), a panel that stays diffuse (illum 2 with Ks) and a small lamp.  Returns the OBJ's path.  Seen from the
    hosts' default camera at (-0.001, 1, 6)."""
    import os
    with open(os.path.join(directory, "room.mtl"), "w") as f:
        f.write("newmtl wall\nKd 0.8 0.7 0.6\n"
                "newmtl floor\nKd 0.6 0.6 0.7\n"
                "newmtl mirror\nKd 0.1 0.1 0.1\nKs 0.9 0.9 0.95\nillum 3\n"
                "newmtl gloss\nKd 0.1 0.1 0.1\nKs 0.7 0.5 0.3\nNs 40\nillum 3\n"
                "newmtl satin\nKd 0.2 0.6 0.3\nKs 1 1 1\nNs 10\nillum 2\n"
                "newmtl lamp\nKd 0 0 0\nKe 4 3 2\n")
    with open(os.path.join(directory, "room.obj"), "w") as f:
        f.write("mtllib room.mtl\n"
                "v -2 -0.2 -1\nv 2 -0.2 -1\nv 2 2.4 -1\nv -2 2.4 -1\n"        # back wall
                "v -2 -0.2 3\nv 2 -0.2 3\n"                                   # floor front edge
                "v -1.6 0.2 0.6\nv -0.2 0.1 0.1\nv -0.1 1.5 -0.3\nv -1.5 1.6 0.2\n"   # mirror panel
                "v 0.3 -0.19 0.2\nv 1.7 -0.19 0.2\nv 1.7 -0.19 2.4\nv 0.3 -0.19 2.4\n"   # glossy strip on the floor
                "v 0.4 0.4 0.3\nv 1.4 0.3 0.1\nv 1.5 1.3 -0.1\nv 0.5 1.4 0.2\n"   # satin panel
                "v 1.0 1.8 -0.9\nv 1.5 1.8 -0.9\nv 1.5 2.2 -0.9\nv 1.0 2.2 -0.9\n"   # lamp
                "usemtl wall\nf 1 2 3 4\n"
                "usemtl floor\nf 5 6 2 1\n"
                "usemtl mirror\nf 7 8 9 10\n"
                "usemtl gloss\nf 11 14 13 12\n"
                "usemtl satin\nf 15 16 17 18\n"
                "usemtl lamp\nf 19 20 21 22\n")
    return os.path.join(directory, "room.obj")
