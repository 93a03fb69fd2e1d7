"""Seeded generators of adversarial inputs for what runs between closest hit and the filter (numpy only; no fixture, no GPU):

  cull scenes   at most 64 triangles, the scenes whose primary rays go through the padded 16-bit screen rectangles of
                screen_bounds() (csrc/api_context.hip) and span_candidates() / closest_hit_brute_set() (csrc/closest_hit.hpp):
                many SMALL triangles in a slab, so that a 16 x 4 pixel block meets a few rectangles out of dozens, a backdrop
                that makes every pixel hit (a dropped candidate changes an id, it does not turn into background), and named
                members placed against the rules of screen_bounds for the camera at EYE0 looking down -z;
  cameras       for K0 (view / proj) and K2 (cameraPos, fov_slope, pixel_jitter);
  K1 plane sets ids, world positions, previous LUTs and push constants for temporalGradient.comp.glsl on filter_planes.soup.

tests/test_gbuffer_scenes_cpu.py checks on the oracle what is claimed here; tests/test_gbuffer_scenes_gpu.py feeds all of it to
the HIP kernels and to the oracle.  Every id a generator returns went through filter_planes.check_ids: the kernels index their
per-id tables unguarded."""
from functools import lru_cache

import numpy as np

import filter_planes as FP

F32 = np.float32
T_VALUES = (1, 2, 40, 63, 64)
SHAPES = ((1, 1), (15, 3), (16, 4), (17, 5), (65, 7), (130, 33))      # (W, H)
MAIN_SHAPE = (130, 33)
STRIP = (130, 33, 5, 21)                                              # W, H and the stored rows [5, 21)
FOVY = 0.4                                                            # the reference's field of view (2 x 0.20)
EYE0 = (0.1, -0.05, 6.0)      # the camera the named members are placed for: looks down -z, its plane is z = 6
SLAB = ((-4.5, 4.5), (-1.1, 1.1), (-1.0, 1.0))                        # where the small triangles are scattered
EXTENT = 9.0                                                          # the slab's longest side
BLOCK = (16, 4)                                                       # the pixels a wave starts on (closest_hit.hpp: kWaveW x kWaveH)

# ids (triangle index + 1) of the named members of a cull scene with T >= 40
(ID_BACKDROP_A, ID_BACKDROP_B, ID_STRADDLE, ID_BEHIND, ID_NEAR_BOUNDED, ID_NEAR_UNBOUNDED, ID_SLIVER, ID_CLOSE, ID_BOUNDARY,
 ID_TWO_EQUAL, ID_COLLINEAR, ID_POINT) = range(1, 13)
N_NAMED = 12
ZERO_AREA_IDS = (ID_TWO_EQUAL, ID_COLLINEAR, ID_POINT)
BOUNDARY_PIXEL = (64, 16)     # the continuous screen coordinate of ID_BOUNDARY's first vertex on MAIN_SHAPE from EYE0
NEAR_RULE = 1e-4              # screen_bounds: a vertex with -z_view <= NEAR_RULE (distance + 1) makes the rectangle unbounded


def _rng(*key):
    return FP._rng(23, *key)


def _frozen(a, dtype=F32):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


def proj_scale(W, H, fovy=FOVY, aspect=None):
    """(P00, P11) of perspective(fovy, aspect) with the y flip every caller here applies (proj[5] *= -1), float64"""
    aspect = float(F32(W) / F32(H)) if aspect is None else aspect
    t = np.tan(0.5 * fovy)
    return 1.0 / (aspect * t), -1.0 / t


# ------------------------------------------------------------------------------------------ cull scenes
def _small_triangles(rng, n, box):
    """n triangles with edges of 0.05 .. 0.15 of the slab's extent, centres uniform in `box`"""
    c = np.stack([rng.uniform(lo, hi, n) for lo, hi in box], -1)
    def edge():
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return d * rng.uniform(0.05, 0.15, (n, 1)) * EXTENT
    e1, e2 = edge(), edge()
    return np.stack([c - (e1 + e2) / 3.0, c + (2.0 * e1 - e2) / 3.0, c + (2.0 * e2 - e1) / 3.0], 1)


def _named_members():
    """[N_NAMED, 3, 3] float64, see cull_scene"""
    e = np.array(EYE0, np.float64)
    m = np.zeros((N_NAMED, 3, 3))
    a, b, c, d = (-80.0, -80.0, -3.0), (80.0, -80.0, -3.0), (80.0, 80.0, -3.0), (-80.0, 80.0, -3.0)
    m[ID_BACKDROP_A - 1] = (a, b, c)
    m[ID_BACKDROP_B - 1] = (a, c, d)
    m[ID_STRADDLE - 1] = ((1.0, -0.3, 4.0), (1.6, -0.45, 4.5), (1.2, -0.4, 7.0))
    m[ID_BEHIND - 1] = ((-0.5, 0.2, 7.2), (0.5, 0.3, 7.5), (0.0, -0.4, 8.0))
    for k, (idx, side, factor, far) in enumerate(((ID_NEAR_BOUNDED, (0.3, 0.2), 1.05, ((-1.0, -0.25, 4.5), (-0.6, -0.3, 4.4))),
                                                  (ID_NEAR_UNBOUNDED, (-0.3, 0.25), 0.95, ((0.5, -0.2, 4.6), (0.9, -0.28, 4.5))))):
        zv = NEAR_RULE * (np.hypot(*side) + 1.0) * factor          # (the distance's own z part, 1e-4 of it, changes nothing)
        m[idx - 1] = (e + (side[0], side[1], -zv),) + far
    m[ID_SLIVER - 1] = ((-2.2, -0.6, 3.0), (2.4, 0.5, 3.05), (-2.2, -0.54, 3.0))
    m[ID_CLOSE - 1] = (e + (-2.0, 3e-4, -2e-3), e + (2.0, 3e-4, -2e-3), e + (0.0, 7e-4, -2e-3))
    W, H = MAIN_SHAPE
    p00, p11 = proj_scale(W, H)
    depth = 2.5
    v = e + ((2.0 * BOUNDARY_PIXEL[0] / W - 1.0) / p00 * depth, (2.0 * BOUNDARY_PIXEL[1] / H - 1.0) / p11 * depth, -depth)
    m[ID_BOUNDARY - 1] = (v, v + (0.35, -0.12, 0.1), v + (0.1, -0.3, -0.05))      # (-y is down the screen: rows >= 16)
    m[ID_TWO_EQUAL - 1] = ((-2.0, 0.5, 5.0), (-1.6, 0.6, 5.1), (-1.6, 0.6, 5.1))
    a0, e0 = np.array((2.0, -0.625, 5.0)), np.array((0.25, 0.125, 0.0625))
    m[ID_COLLINEAR - 1] = (a0, a0 + e0, a0 + 2.0 * e0)
    m[ID_POINT - 1] = ((0.5, 0.5, 5.2),) * 3
    return m


@lru_cache(maxsize=None)
def cull_scene(T, seed=0):
    """[T, 9] float32.  Small triangles scattered through SLAB; with T >= 40 the first N_NAMED are, for the camera at EYE0
    that looks down -z with the reference field of view:
      1, 2   a backdrop quad at z = -3, 160 wide: behind everything, it fills the frame of every camera that looks towards -z
      3      one vertex behind the camera plane, two in front (in view)
      4      entirely behind the camera plane
      5, 6   one vertex in front of the camera plane by 1.05 / 0.95 times NEAR_RULE (distance + 1): the rectangle of the first
             is finite (and clamps), that of the second is unbounded; the other two vertices are in view
      7      a sliver across the frame, at most 0.06 wide: a large rectangle, few pixels
      8      0.002 in front of the camera and 4 wide: the projected rectangle clamps at +-32000
      9      its first vertex projects onto column 64 = 4 x 16 and row 16 = 4 x 4 of MAIN_SHAPE (as closely as binary32 vertices
             allow); the triangle lies right of and below it, so the unpadded rectangle starts on a block corner
      10-12  zero area: two equal vertices, three collinear ones (exactly: dyadic steps), a point."""
    rng = _rng(1, T, seed)
    if T < 40:
        tris = _small_triangles(rng, T, ((-1.0, 1.0), (-0.5, 0.5), (-1.0, 1.0)))
    else:
        tris = np.concatenate([_named_members(), _small_triangles(rng, T - N_NAMED, SLAB)])
    return _frozen(tris.reshape(T, 9))


@lru_cache(maxsize=None)
def fan_strip(n_quads, odd=False):
    """[2 n_quads (+ 1), 9] float32: a heightfield strip along x in front of EYE0, every quad the fan pair (a, b, c), (a, c, d) —
    rtpt_scene_upload's test for the pair records, so closest_hit_brute_set takes its `paired` branch.  odd: one more
    triangle, the scene is no longer all pairs and the branch is off."""
    x = np.linspace(-3.6, 3.8, n_quads + 1)
    lo = np.stack([x, -0.55 + 0.1 * np.cos(2.0 * x), 0.6 * np.sin(1.7 * x)], -1).astype(F32)
    hi = np.stack([x + 0.05, 0.5 + 0.1 * np.sin(3.0 * x), 0.6 * np.cos(1.3 * x)], -1).astype(F32)
    tris = []
    for i in range(n_quads):
        a, b, c, d = lo[i], lo[i + 1], hi[i + 1], hi[i]
        tris += [np.stack([a, b, c]), np.stack([a, c, d])]
    if odd:
        tris.append(np.stack([lo[0], hi[0], lo[0] + F32(0.3) * (lo[0] - lo[1])]))
    return _frozen(np.stack(tris).reshape(-1, 9))


def is_all_fan_pairs(tris):
    """rtpt_scene_upload's test: every (2q, 2q + 1) is (a, b, c), (a, c, d), bitwise"""
    tris = np.asarray(tris, F32)
    if len(tris) < 2 or len(tris) % 2:
        return False
    t = np.ascontiguousarray(tris).reshape(-1, 2, 9).view(np.uint32)
    return bool((t[:, 0, 0:3] == t[:, 1, 0:3]).all() and (t[:, 0, 6:9] == t[:, 1, 3:6]).all())


SCENES = tuple(("cull", T) for T in T_VALUES) + (("fan", 20), ("fan_odd", 20), ("fan", 32))


def scene(kind):
    """kind: ("cull", T), ("fan", n_quads) or ("fan_odd", n_quads)"""
    name, n = kind
    if name == "cull":
        return cull_scene(n)
    return fan_strip(n, odd=(name == "fan_odd"))


# ------------------------------------------------------------------------------------------ cameras
# K0: name -> (eye, direction or None with `at`, up, fovy, aspect or None for W / H)
K0_CAMERAS = {
    "outside": dict(eye=EYE0, dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)),
    "rolled": dict(eye=(0.1, -0.05, 24.0), dir=(0.0, 0.0, -1.0), up=(1.0, 0.0, 0.0)),
    "rolled_near": dict(eye=EYE0, dir=(0.0, 0.0, -1.0), up=(1.0, 0.0, 0.0)),
    "along_x": dict(eye=(-9.0, 0.2, 0.1), dir=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)),
    "along_y": dict(eye=(0.3, -7.0, 0.2), dir=(0.0, 1.0, 0.0), up=(0.0, 0.0, 1.0)),
    "diagonal": dict(eye=(4.0, 2.0, 7.0), dir=(-4.0, -2.0, -7.0), up=(0.0, 1.0, 0.0)),
    "inside": dict(eye=(0.2, 0.1, 0.95), dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fovy=1.6),
    "narrow": dict(eye=(0.3, 0.1, 300.0), dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fovy=0.01),
    "wide": dict(eye=(0.0, 0.0, 2.5), dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), fovy=2.6),
    "aspect": dict(eye=EYE0, dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), aspect=1.7),
}
MAIN_CAMERAS = ("outside", "rolled", "diagonal", "inside")     # every pixel hits, dozens of ids (asserted on the CPU)


def k0_camera(O, name, W, H):
    """(view, proj) float32[16] column-major from the oracle module's look_at / perspective, y flipped like the reference's"""
    c = K0_CAMERAS[name]
    eye = np.asarray(c["eye"], F32)
    view = O.look_at(eye, (eye + np.asarray(c["dir"], F32)).astype(F32), c["up"])
    aspect = F32(c["aspect"]) if "aspect" in c else F32(W) / F32(H)
    proj = O.perspective(F32(c.get("fovy", FOVY)), aspect, 0.1, 400.0)
    proj[5] *= -1
    return view, proj


def view_space(name, pts):
    """float64 view-space coordinates of world points for a K0 camera (x right, y up, -z ahead), for the CPU-side claims"""
    c = K0_CAMERAS[name]
    f = np.asarray(c["dir"], np.float64)
    f /= np.linalg.norm(f)
    s = np.cross(f, np.asarray(c["up"], np.float64))
    s /= np.linalg.norm(s)
    u = np.cross(s, f)
    r = np.asarray(pts, np.float64) - np.asarray(c["eye"], np.float64)
    return np.stack([r @ s, r @ u, -(r @ f)], -1)


REF_SLOPE = 0.20271003
K2_POSITIONS = {"outside": EYE0, "inside": (0.2, 0.1, 0.95), "far": (0.1, -0.05, 24.0)}
K2_SLOPES = (REF_SLOPE, 1.0, 4.0)
K2_JITTERS = (0.0, 0.375, 8.0)
# (position, fov_slope, pixel_jitter): every slope x jitter, the positions in turn
K2_CAMERAS = tuple((tuple(K2_POSITIONS)[(i + j) % 3], s, jt) for i, s in enumerate(K2_SLOPES) for j, jt in enumerate(K2_JITTERS))


# ------------------------------------------------------------------------------------------ K1 plane sets
WP_CLASSES = ("on", "off", "vertex", "huge", "tiny", "planted")
LUT_PREV_CLASSES = ("equal", "perturbed", "unrelated", "point", "huge")
PC_CLASSES = ("rest", "moved", "light_on_pixel", "camera_on_pixel", "both_black", "one_black", "bright")
K1_T = 40
DEGENERATE_IDS = (FP.ID_TWO_EQUAL, FP.ID_COLLINEAR, FP.ID_POINT)     # of filter_planes.soup


def lut_numpy(tris):
    """[(T+1), 3, 4] float32: the LUT of un-posed triangles (the identity model leaves every coordinate as it is)"""
    tris = np.asarray(tris, F32).reshape(-1, 3, 3)
    lut = np.zeros((len(tris) + 1, 3, 4), F32)
    lut[1:, :, :3] = tris
    return lut


@lru_cache(maxsize=None)
def k1_ids(T, W, H, seed=0):
    """[H, W] uint32, uniform in [0, T]"""
    ids = _rng(2, T, W, H, seed).integers(0, T + 1, (H, W), dtype=np.uint32)
    return _frozen(FP.check_ids(ids, T), np.uint32)


def k1_worldpos(cls, tris, ids, seed=0):
    """[H, W, 4] float32 (w = 1) of one class, for the triangles `tris` ([T, 9]) and the id plane:
    on: a point of the pixel's triangle; off: that point moved by up to a scene extent (4) along every axis; vertex: exactly one
    of its vertices; huge / tiny: the point times 1e18 / 1e-30; planted: NaN, +Inf, -Inf in single coordinates.  Pixels of
    id 0 carry the clear colour's zeros."""
    ids = np.asarray(ids)
    H, W = ids.shape
    T = len(tris)
    rng = _rng(3, FP._seed_of(cls), T, W, H, seed)
    v = np.concatenate([np.zeros((1, 3, 3)), np.asarray(tris, np.float64).reshape(T, 3, 3)])[ids.astype(np.int64)]   # [H, W, 3, 3]
    b = rng.dirichlet((1.0, 1.0, 1.0), (H, W))
    p = (b[..., None] * v).sum(-2)
    if cls == "off":
        p = p + rng.uniform(-4.0, 4.0, (H, W, 3))
    elif cls == "vertex":
        k = rng.integers(0, 3, (H, W))
        p = np.take_along_axis(v, k[..., None, None], 2)[:, :, 0, :]
    elif cls == "huge":
        p = p * 1e18
    elif cls == "tiny":
        p = p * 1e-30
    else:
        assert cls in ("on", "planted"), cls
    wp = np.ones((H, W, 4), F32)
    wp[..., :3] = p
    wp[ids == 0, :3] = 0.0
    if cls == "planted":
        for n, (y, x, val) in enumerate(FP.planted_positions(ids, T)):
            wp[y, x, n % 3] = val
    return wp


def k1_lut_prev(cls, tris, seed=0):
    """[(T+1), 12] float32 previous LUT of one class: equal to the LUT; every vertex moved by up to 0.05; unrelated triangles;
    every third id collapsed to its first vertex (area exactly 0), the others perturbed; every third id at +-1e30"""
    T = len(tris)
    rng = _rng(4, FP._seed_of(cls), T, seed)
    lut = lut_numpy(tris)
    if cls == "equal":
        return np.ascontiguousarray(lut.reshape(T + 1, 12))
    out = lut.copy()
    out[1:, :, :3] += rng.uniform(-0.05, 0.05, (T, 3, 3)).astype(F32)
    if cls == "unrelated":
        out[1:, :, :3] = rng.uniform(-2.0, 2.0, (T, 3, 3))
    elif cls == "point":
        out[1::3, 1:, :3] = out[1::3, :1, :3]
    elif cls == "huge":
        sign = np.where(np.arange(len(out[1::3])) % 2 == 0, 1.0, -1.0)[:, None, None]
        out[1::3, :, :3] = (sign * 1e30 * rng.uniform(0.5, 1.5, (len(sign), 3, 3))).astype(F32)
    else:
        assert cls == "perturbed", cls
    return np.ascontiguousarray(out.reshape(T + 1, 12))


def k1_push_constants(cls, ids, worldpos):
    """dict(cameraPos, lightPos, lightPosPrev, currentCameraColor, previousCameraColor) of one class.  rest: light and colour as
    in the frame before (only the reprojected point differs, by its rounding, when LUT_PREV is the LUT); moved: both changed; light_on_pixel /
    camera_on_pixel: the light / the camera exactly at the world position of the first finite pixel with an id (normalize(0)
    there); both_black: 0 / 0; one_black: the previous colour is 0 (lambda 1); bright: colours of 1e20 (lengths overflow)."""
    pc = dict(cameraPos=(0.3, 0.4, 5.0), lightPos=(1.0, 1.5, 3.0), lightPosPrev=(0.6, 1.2, 3.3),
              currentCameraColor=(0.5, 0.5, 0.5), previousCameraColor=(0.4, 0.5, 0.45))
    ids, worldpos = np.asarray(ids), np.asarray(worldpos)
    ok = np.argwhere((ids > 0) & np.isfinite(worldpos[..., :3]).all(-1))
    at = tuple(float(c) for c in worldpos[tuple(ok[len(ok) // 2])][:3]) if len(ok) else (0.0, 0.0, 0.0)
    if cls == "rest":
        pc["lightPosPrev"], pc["previousCameraColor"] = pc["lightPos"], pc["currentCameraColor"]
    elif cls == "light_on_pixel":
        pc["lightPos"] = at
    elif cls == "camera_on_pixel":
        pc["cameraPos"] = at
    elif cls == "both_black":
        pc["currentCameraColor"] = pc["previousCameraColor"] = (0.0, 0.0, 0.0)
    elif cls == "one_black":
        pc["previousCameraColor"] = (0.0, 0.0, 0.0)
    elif cls == "bright":
        pc["currentCameraColor"], pc["previousCameraColor"] = (1e20, 1e20, 1e20), (1e20, 0.5e20, 2e20)
    else:
        assert cls == "moved", cls
    return pc


def fill_push_constants(pc, values, frame=0):
    """set a PushConstants structure (the oracle's or the library's) from k1_push_constants' dict"""
    for name, v in values.items():
        getattr(pc, name)[:] = [float(F32(c)) for c in v]
    pc.frameNumber = frame
    return pc


# ------------------------------------------------------------------------------------------ float64 restatement of K1
def gradient_numpy(ids, worldpos, lut, lut_prev, pc):
    """temporalGradient.comp.glsl:128-167 in float64 numpy, from the shader text: [H, W] lambda (0 where the id is 0).  NaN
    where the shader's arithmetic is 0 / 0 before its min(1, .) (GLSL leaves min with a NaN undefined; the project's
    contract makes it 1)."""
    ids = np.asarray(ids).astype(np.int64)
    p = np.asarray(worldpos, np.float64)[..., :3]
    cur_v = np.asarray(lut, np.float64).reshape(-1, 3, 4)[ids][..., :3]
    prv_v = np.asarray(lut_prev, np.float64).reshape(-1, 3, 4)[ids][..., :3]
    v1, v2, v3 = cur_v[..., 0, :], cur_v[..., 1, :], cur_v[..., 2, :]
    length = lambda a: np.sqrt((a * a).sum(-1))
    dot = lambda a, b: (a * b).sum(-1)

    def normalize(a):
        return a / length(a)[..., None]

    def area(a, b, c):                                              # :50-55
        return length(np.cross(b - a, c - a)) * 0.5

    def phong(pt, n, cam, lpos, lcol):                              # :71-101
        ldir = normalize(lpos - pt)
        ambient = 0.1 * lcol
        diffuse = np.maximum(dot(n, ldir), 0.0)[..., None] * lcol
        vdir = normalize(cam - pt)
        inc = -ldir
        rdir = inc - 2.0 * dot(n, inc)[..., None] * n               # reflect(I, N)
        spec = np.maximum(dot(vdir, rdir), 0.0) ** 128
        return (ambient + diffuse + (0.5 * spec)[..., None] * lcol) * 1.0 * 0.7

    with np.errstate(all="ignore"):
        normal = normalize(np.cross(v2 - v1, v3 - v1))              # :142
        total = area(v1, v2, v3)                                    # :60-66
        bc = np.stack([area(p, v2, v3), area(v1, p, v3), area(v1, v2, p)], -1) / total[..., None]
        wpp = (bc[..., None] * prv_v).sum(-2)                       # :153
        g = lambda k: np.asarray(pc[k], np.float64)
        cur = phong(p, normal, g("cameraPos"), g("lightPos"), g("currentCameraColor"))                  # :158
        prv = phong(wpp, normal, g("cameraPos"), g("lightPosPrev"), g("previousCameraColor"))           # :161
        delta = np.maximum(length(cur), length(prv))                # :166
        ratio = length(cur - prv) / delta
        lam = np.where(np.isnan(ratio), np.nan, np.minimum(1.0, ratio))   # :167
    return np.where(ids == 0, 0.0, lam)
