"""Seeded generators of adversarial scenes for everything the path-trace kernels (K2) do after the first hit (numpy only; no
fixture, no GPU): shade_segment, the per-segment compaction, the hand-over queue between the tile kernel and k_pathtrace_queue,
the accumulators of samples_per_pixel > 1 and the ray counter (csrc/pathtrace_tile.hpp, csrc/kernels.hip).  Every scene carries its K2 camera, its
light and an optional material table, and exists in up to three forms:

  small   at most 64 triangles: the wave-uniform brute-force kernels (k_pathtrace_small / k_gbuffer_pathtrace_small);
          RTPT_FLAG_FORCE_BVH runs the same triangles through the BVH
  pairs   tessellated, more than 64 triangles, every (2q, 2q + 1) a fan pair: the BVH over pairs
  odd     `pairs` plus one unpaired triangle: the BVH over single triangles

  closed room    the camera inside a box, the light 5 000 units away: every path of the small form lives to the segment
                 bound, so every compaction keeps 256 of 256 paths and every queue is exactly full
  mask room      the closed room made wider than the frustum, pixel_jitter 0, emissive rectangles 0.01 in front of the far
                 wall whose edges lie on pixel EDGES (a pixel centre is half a pixel from the nearest one): they choose which
                 paths of a 64 x 4 tile end at segment 0 (mask()).  Kd components are powers of two below 1: every product
                 of albedos is exact, whatever the order of its factors
  three ends     a floor and two walls open to the sky, the light inside the scene, one emissive quad: paths of one tile end
                 by light, sky, emitter and bound, at different segments
  placed         closed room and three ends far from the origin (ray_offset is at or below an ulp there), scaled by 1e-3
                 and by 1e3
  sphere, soup   the camera inside a UV sphere (zero-area halves at the poles, long bounces); a soup of 300 triangles
                 inside the closed room (BVH only)

tests/test_pathtrace_scenes_cpu.py checks on the oracle what is claimed here, tests/test_pathtrace_scenes_gpu.py feeds the
scenes to the HIP kernels and to the oracle.  MEASURED holds the oracle's counts the CPU test takes its floors
from."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import filter_planes as FP
from gbuffer_scenes import MAIN_SHAPE, REF_SLOPE, STRIP, is_all_fan_pairs  # noqa: F401 (the tests take them from here)

F32 = np.float32
SEGMENTS = 9                                  # the GPU test's max_segments outside its window cases
EDGE_SHAPES = ((65, 7), (1, 1))
RESIZED_SHAPE = (197, 45)                     # the larger frame of the GPU test's resize
TILE = (64, 4)                                # pathtrace_tile's pixels; a wave owns 16 x 4 of them (tile_pixel, closest_hit.hpp)
WAVE_W = 16
FORMS = ("small", "pairs", "odd")
LIGHT_FAR = (300.0, 5000.0, -400.0)           # the "closed" scenes' light
LIGHT_COLOR = (0.5, 0.5, 0.5)
EMISSIVE_GAP = 0.01

Scene = namedtuple("Scene", "name form tris cam slope jitter light light_radius tri_material materials")


def _rng(*key):
    return FP._rng(29, *key)


def _frozen(a, dtype=F32):
    a = np.ascontiguousarray(a, dtype)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------ building blocks
def _quad_tris(quads):
    """[n, 4, 3] corners (a, b, c, d) -> [2n, 9] float32: the fan pairs (a, b, c), (a, c, d)"""
    q = np.asarray(quads, F32).reshape(-1, 4, 3)
    return np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 1).reshape(-1, 9)


def _box_quads(lo, hi):
    """the six walls of a box, float64 [6, 4, 3]: -x, +x, -y, +y, -z, +z"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    return np.array([
        [(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)],
        [(x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)],
        [(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)],
        [(x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)],
        [(x0, y0, z0), (x0, y1, z0), (x1, y1, z0), (x1, y0, z0)],
        [(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]], np.float64)


def _tessellate(quads, n):
    """every quad as n x n sub-quads (corners of one float32 grid per quad, so neighbours share them bitwise): the
    sub-quads [q n n, 4, 3] and the index of the quad each came from"""
    out, src = [], []
    s = np.linspace(0.0, 1.0, n + 1)
    for k, (a, b, c, d) in enumerate(np.asarray(quads, np.float64)):
        grid = ((1 - s)[:, None, None] * ((1 - s)[None, :, None] * a + s[None, :, None] * b) +
                s[:, None, None] * ((1 - s)[None, :, None] * d + s[None, :, None] * c)).astype(F32)      # [v, u, 3]
        for j in range(n):
            for i in range(n):
                out.append([grid[j, i], grid[j, i + 1], grid[j + 1, i + 1], grid[j + 1, i]])
                src.append(k)
    return np.array(out, F32), np.array(src)


def _with_form(form, quads, quad_material):
    """triangles and per-triangle material indices of a quad list in one form"""
    tris = _quad_tris(quads)
    mat = np.repeat(np.asarray(quad_material, np.uint32), 2)
    if form == "odd":      # one unpaired triangle, coplanar with the first quad (a, b, d): at equal t the lower id wins (D4)
        q = np.asarray(quads[0], F32)
        tris = np.concatenate([tris, np.concatenate([q[0], q[1], q[3]])[None]])
        mat = np.concatenate([mat, mat[:1]])
    return _frozen(tris), _frozen(mat, np.uint32)


def _materials(kd_rows, ke_rows=()):
    """[m, 6] float32: (Kd, 0) rows, then (0.5, Ke) rows"""
    kd = [tuple(k) + (0.0, 0.0, 0.0) for k in kd_rows]
    ke = [(0.5, 0.5, 0.5) + tuple(k) for k in ke_rows]
    return _frozen(np.array(kd + ke, F32).reshape(-1, 6))


# six Kd whose components are powers of two below 1 (see the module text), one per wall
WALL_KD = ((0.5, 0.25, 0.125), (0.25, 0.5, 0.5), (0.5, 0.5, 0.25), (0.125, 0.5, 0.25), (0.5, 0.125, 0.5), (0.25, 0.25, 0.5))
ROOM = ((-2.0, -1.0, -3.0), (2.0, 1.0, 1.0))
ROOM_CAM = (0.1, -0.05, 0.5)


# ------------------------------------------------------------------------------------------ 1. closed room
@lru_cache(maxsize=None)
def closed_room(form="small"):
    quads, wall = _box_quads(*ROOM), np.arange(6)
    if form != "small":
        quads, wall = _tessellate(quads, 3)           # 108 triangles
    tris, mat = _with_form(form, quads, wall)
    return Scene("closed_room", form, tris, ROOM_CAM, REF_SLOPE, 0.375, LIGHT_FAR, 0.2, mat, _materials(WALL_KD))


# ------------------------------------------------------------------------------------------ 2. mask room
SMALL_PATTERNS = ("only_first", "only_last", "all_but_one", "block", "two_rows", "empty", "untouched")
TESS_PATTERNS = SMALL_PATTERNS + ("checker", "one_lane")
MASK_DZ = 4.0                                 # camera to the emissive plane
ALL_BUT_ONE_AT = (17, 2)


def _pattern_rects(p):
    """tile-local pixel rectangles (x0, x1, y0, y1) that END at segment 0"""
    return {"only_first": [(1, 64, 0, 1), (0, 64, 1, 4)], "only_last": [(0, 64, 0, 3), (0, 63, 3, 4)],
            "all_but_one": [(ALL_BUT_ONE_AT[0], ALL_BUT_ONE_AT[0] + 1, ALL_BUT_ONE_AT[1], ALL_BUT_ONE_AT[1] + 1)],
            "block": [(32, 48, 0, 4)], "two_rows": [(0, 64, 1, 3)], "empty": [(0, 64, 0, 4)], "untouched": []}[p]


def tile_patterns(W, H, row0=0, row1=None, tess=False):
    """{(x0, y0) of a tile: pattern} for the tiles of rows [row0, row1).  Tessellated: the patterns in turn over the full tiles
    in raster order, then on over the partial ones (where the frame clips them).  Small: once over the first full tiles, once
    over the first partial ones, every other tile untouched (64 triangles are 26 rectangles at most)"""
    row1 = H if row1 is None else row1
    names = TESS_PATTERNS if tess else SMALL_PATTERNS
    tiles = [(x, y) for y in range(row0, row1, TILE[1]) for x in range(0, W, TILE[0])]
    full = [t for t in tiles if t[0] + TILE[0] <= W and t[1] + TILE[1] <= row1]
    partial = [t for t in tiles if t not in full]
    if tess:
        return {t: names[i % len(names)] for i, t in enumerate(full + partial)}
    order = full[:len(names)] + partial[:len(names)]
    out = {t: "untouched" for t in tiles}
    out.update({t: names[i % len(names)] for i, t in enumerate(order)})
    return out


def mask(W, H, row0=0, row1=None, tess=False):
    """[H, W] bool: the pixels whose path ENDS at segment 0, on an emissive surface"""
    m = np.zeros((H, W), bool)
    for (x0, y0), p in tile_patterns(W, H, row0, row1, tess).items():
        t = np.zeros((TILE[1], TILE[0]), bool)
        if p == "checker":
            t[:] = (np.add.outer(np.arange(TILE[1]), np.arange(TILE[0])) % 2) == 1
        elif p == "one_lane":      # one survivor per wave (16 x 4 pixels), each at another lane
            t[:] = True
            for w in range(TILE[0] // WAVE_W):
                lane = (21 * w + 5) % 64
                t[lane // WAVE_W, WAVE_W * w + lane % WAVE_W] = False
        else:
            for (a, b, c, d) in _pattern_rects(p):
                t[c:d, a:b] = True
        sub = m[y0:y0 + TILE[1], x0:x0 + TILE[0]]
        sub[:] = t[:sub.shape[0], :sub.shape[1]]
    return m


def _mask_plane(cam, W, H):
    """X(xe), Y(ye) of pixel EDGES on the emissive plane (float64) and its z"""
    X = lambda xe: cam[0] + REF_SLOPE * (2.0 * np.asarray(xe, np.float64) - W) / H * MASK_DZ
    Y = lambda ye: cam[1] - REF_SLOPE * (2.0 * np.asarray(ye, np.float64) - H) / H * MASK_DZ
    return X, Y, cam[2] - MASK_DZ


@lru_cache(maxsize=None)
def mask_room(form="small", W=MAIN_SHAPE[0], H=MAIN_SHAPE[1], row0=0, row1=None):
    """the room is wider than the frustum of W x H; material 0..5 the walls, 6 the non-emissive quads of the tessellated
    plane, 7.. one emissive material per rectangle (small) / one (tessellated)"""
    cam = ROOM_CAM
    X, Y, z = _mask_plane(cam, W, H)
    hw, hh = 1.25 * REF_SLOPE * (W / H) * MASK_DZ + 1.0, 1.25 * REF_SLOPE * MASK_DZ + 1.0
    room = _box_quads((cam[0] - hw, cam[1] - hh, z - EMISSIVE_GAP), (cam[0] + hw, cam[1] + hh, cam[2] + 0.5))
    kd = WALL_KD + ((0.25, 0.125, 0.25),)
    if form == "small":
        quads, qmat = list(room), list(range(6))
        for (x0, y0), p in tile_patterns(W, H, row0, row1).items():
            for (a, b, c, d) in _pattern_rects(p):
                xa, xb, ya, yb = x0 + a, min(x0 + b, W), y0 + c, min(y0 + d, H if row1 is None else row1)
                if xa >= xb or ya >= yb:
                    continue
                quads.append([(X(xa), Y(ya), z), (X(xb), Y(ya), z), (X(xb), Y(yb), z), (X(xa), Y(yb), z)])
                qmat.append(len(quads))                # 7 + the rectangle's number
        n_rect = len(quads) - 6
        ke = [(2.0 + k / 8.0, 1.5, 1.25 + k / 16.0) for k in range(n_rect)]
        tris, mat = _with_form(form, np.array(quads, np.float64), qmat)
        assert len(tris) <= 64
    else:
        m = mask(W, H, row0, row1, tess=True)
        gx, gy = X(np.arange(W + 1)).astype(F32), Y(np.arange(H + 1)).astype(F32)      # one float32 grid: shared corners
        quads = [q for q in room.astype(F32)]
        qmat = list(range(6))
        for y in range(H):
            for x in range(W):
                quads.append([(gx[x], gy[y], z), (gx[x + 1], gy[y], z), (gx[x + 1], gy[y + 1], z), (gx[x], gy[y + 1], z)])
                qmat.append(7 if m[y, x] else 6)
        ke = [(2.0, 1.5, 1.25)]
        tris, mat = _with_form(form, np.array(quads, F32), qmat)
    return Scene("mask_room", form, tris, cam, REF_SLOPE, 0.0, LIGHT_FAR, 0.2, mat, _materials(kd, ke))


# ------------------------------------------------------------------------------------------ 3. three ends in one tile
THREE_CAM = (0.1, 0.6, 3.0)
THREE_LIGHT = (0.5, 0.9, -0.6)


@lru_cache(maxsize=None)
def three_ends(form="small"):
    """a trench along z: its floor and its two walls, open at both ends and above"""
    floor = [(-1.6, 0.0, -5.0), (1.2, 0.0, -5.0), (1.2, 0.0, 4.0), (-1.6, 0.0, 4.0)]
    right = [(1.2, 0.0, -5.0), (1.2, 3.0, -5.0), (1.2, 3.0, 4.0), (1.2, 0.0, 4.0)]
    left = [(-1.6, 0.0, -5.0), (-1.6, 0.0, 4.0), (-1.6, 3.5, 4.0), (-1.6, 3.5, -5.0)]
    emitter = [(-1.59, 0.35, -1.9), (-1.59, 0.35, -1.2), (-1.55, 0.9, -1.2), (-1.55, 0.9, -1.9)]
    quads, qmat = np.array([floor, right, left, emitter], np.float64), np.array([0, 1, 2, 3])
    if form != "small":
        quads, src = _tessellate(quads, 5)             # 200 triangles
        qmat = qmat[src]
    tris, mat = _with_form(form, quads, qmat)
    materials = _materials(((0.75, 0.7, 0.6), (0.3, 0.55, 0.8), (0.85, 0.35, 0.3)), ((4.0, 3.0, 1.5),))
    return Scene("three_ends", form, tris, THREE_CAM, REF_SLOPE, 0.375, THREE_LIGHT, 0.2, mat, materials)


# ------------------------------------------------------------------------------------------ 4. placement and scale
PLACEMENTS = {"far": (1.0, (1000.0, -2000.0, 500.0)), "tiny": (1e-3, (0.0, 0.0, 0.0)), "huge": (1e3, (0.0, 0.0, 0.0))}


def placed(scene, how):
    """the scene scaled, then translated, camera, light and light radius with it (float64, rounded once).  ray_offset stays
    1e-4: at or below an ulp of the coordinates of `far`, a tenth of the room of `tiny`"""
    s, t = PLACEMENTS[how]
    t = np.asarray(t, np.float64)
    move = lambda p: tuple(float(F32(v)) for v in (np.asarray(p, np.float64) * s + t))
    tris = (np.asarray(scene.tris, np.float64).reshape(-1, 3, 3) * s + t).reshape(-1, 9)
    return scene._replace(name=scene.name + "_" + how, tris=_frozen(tris), cam=move(scene.cam), light=move(scene.light),
                          light_radius=float(F32(scene.light_radius * s)))


# ------------------------------------------------------------------------------------------ 5. curved and cluttered
@lru_cache(maxsize=None)
def sphere(form="small"):
    """the camera inside test_traversal_gpu's UV sphere; no material table: the reference's normal-keyed colours"""
    from test_traversal_gpu import _sphere
    xyz, idx = _sphere(8, 4) if form == "small" else _sphere(32, 16)
    tris = xyz[idx].reshape(-1, 9)
    if form == "odd":
        tris = np.concatenate([tris, tris[40:41]])
    return Scene("sphere", form, _frozen(tris), (0.05, 0.02, 0.2), REF_SLOPE, 0.375, LIGHT_FAR, 0.2, None, None)


@lru_cache(maxsize=None)
def soup(seed=0):
    """300 triangles of every orientation inside the closed room (312 triangles, no pairs: the BVH over triangles)"""
    rng = _rng(5, seed)
    (x0, y0, z0), (x1, y1, z1) = ROOM
    n = 300
    c = np.stack([rng.uniform(x0 + 0.3, x1 - 0.3, n), rng.uniform(y0 + 0.2, y1 - 0.2, n), rng.uniform(z0 + 0.3, -0.2, n)], -1)
    v = c[:, None, :] + rng.normal(0.0, 0.12, (n, 3, 3))
    room = closed_room("small")
    tris = np.concatenate([room.tris, v.reshape(n, 9).astype(F32)])
    mat = np.concatenate([room.tri_material, rng.integers(0, 6, n).astype(np.uint32)])
    return room._replace(name="soup", form="odd", tris=_frozen(tris), tri_material=_frozen(mat, np.uint32))


# ------------------------------------------------------------------------------------------ the list
def scene(name, form="small", W=MAIN_SHAPE[0], H=MAIN_SHAPE[1], rows=None):
    """name: closed_room, closed_room_unjittered, mask_room, three_ends, sphere, soup, or closed_room / three_ends + _far, _tiny,
    _huge"""
    for how in PLACEMENTS:
        if name.endswith("_" + how):
            return placed(scene(name[:-len(how) - 1], form, W, H, rows), how)
    if name == "mask_room":
        return mask_room(form, W, H, *(rows or (0, None)))
    if name == "closed_room_unjittered":      # shares a context (one pixel_jitter) with the mask room
        return closed_room(form)._replace(name=name, jitter=0.0)
    if name == "soup":
        return soup()
    return {"closed_room": closed_room, "three_ends": three_ends, "sphere": sphere}[name](form)


PLACED = tuple(b + "_" + how for b in ("closed_room", "three_ends") for how in PLACEMENTS)
# (name, form) of everything that runs on the main shape
MAIN_SCENES = tuple((n, f) for n in ("closed_room", "mask_room", "three_ends", "sphere") for f in FORMS) + (("soup", "odd"),) + \
    tuple((n, "small") for n in PLACED) + (("closed_room_far", "pairs"), ("three_ends_far", "odd"))


# the window cases: RTPT_PT_WINDOW = w makes the tile kernel hand over after w segments; the queue launches run w, 2w, 4w, ... more
WINDOW_SCENES = (("closed_room", "small"), ("mask_room", "small"), ("three_ends", "small"), ("closed_room", "pairs"), ("three_ends", "odd"))
WINDOWS = (1, 2, 3, None)                     # None: the default, 4 (brute force) / 8 (BVH) (pt_first_window, csrc/kernels.hpp)


def window_of(window, form):
    return window or (4 if form == "small" else 8)


def segment_values(w):
    """max_segments on, one past and far past the boundaries of window w; above 17 only with w = 1 (17: five queue launches)"""
    return sorted({s for s in (w, w + 1, 2 * w, 2 * w + 1, 4 * w, 4 * w + 1, 8 * w + 1, 17 if w == 1 else w) if w == 1 or s <= 17})


def window_boundaries(w, max_segments):
    """the segment numbers at which paths change launch"""
    return [b for b in (w, 2 * w, 4 * w, 8 * w, 16 * w) if b < max_segments]


def push_constants(scene, frame=0):
    """the dict gbuffer_scenes.fill_push_constants takes"""
    return dict(cameraPos=scene.cam, lightPos=scene.light, lightPosPrev=scene.light, currentCameraColor=LIGHT_COLOR,
                previousCameraColor=LIGHT_COLOR)


# ------------------------------------------------------------------------------------------ what a dump says
def alive_after(seq_n, boundaries):
    """paths (1 spp) that are handed over each window boundary b: they ran more than b segments"""
    return [int((seq_n > b).sum()) for b in boundaries]


def tiles_with_end_segments(seq_n, k=3):
    """64 x 4 tiles (from row 0) that hold at least k different path lengths"""
    H, W = seq_n.shape
    return sum(len(np.unique(seq_n[y:y + TILE[1], x:x + TILE[0]])) >= k for y in range(0, H, TILE[1]) for x in range(0, W, TILE[0]))


def self_hits(seq_id, seq_n):
    """bounce rays whose hit id equals the id they left (1 spp)"""
    a, b = seq_id[..., :-1], seq_id[..., 1:]
    k = np.arange(seq_id.shape[-1] - 1)
    return int(((a == b) & (a > 0) & (k[None, None, :] + 1 < seq_n[..., None])).sum())


# what the oracle measured at MAIN_SHAPE, SEGMENTS, frame 0, 1 spp (tests/test_pathtrace_scenes_cpu.py asserts at least half of
# each; a count of 0 is left out, so no floor is met by nothing): paths by the way they end, tiles with at least three different
# path lengths, paths alive after 4 and after 8 segments, bounce rays that hit the triangle they left
MEASURED = {
    ('three_ends', 'small'): {'light': 154, 'sky': 3930, 'bound': 85, 'emissive': 121, 'tiles3': 26, 'alive4': 1029, 'alive8': 144},
    ('three_ends', 'pairs'): {'light': 154, 'sky': 3930, 'bound': 85, 'emissive': 121, 'tiles3': 26, 'alive4': 1029, 'alive8': 144},
    ('three_ends', 'odd'): {'light': 154, 'sky': 3930, 'bound': 85, 'emissive': 121, 'tiles3': 26, 'alive4': 1029, 'alive8': 144},
    ('sphere', 'small'): {'bound': 4290, 'alive4': 4290, 'alive8': 4290},
    ('sphere', 'pairs'): {'bound': 4290, 'alive4': 4290, 'alive8': 4290},
    ('sphere', 'odd'): {'bound': 4290, 'alive4': 4290, 'alive8': 4290},
    ('soup', 'odd'): {'bound': 4290, 'alive4': 4290, 'alive8': 4290},
    ('closed_room_far', 'small'): {'sky': 13, 'bound': 4277, 'tiles3': 2, 'alive4': 4285, 'alive8': 4280, 'self_hits': 17},
    ('closed_room_tiny', 'small'): {'bound': 4290, 'alive4': 4290, 'alive8': 4290},
    ('closed_room_huge', 'small'): {'sky': 445, 'bound': 3845, 'tiles3': 18, 'alive4': 4053, 'alive8': 3877, 'self_hits': 599},
    ('three_ends_far', 'small'): {'light': 154, 'sky': 3930, 'bound': 85, 'emissive': 121, 'tiles3': 26, 'alive4': 1028, 'alive8': 144, 'self_hits': 3},
    ('three_ends_tiny', 'small'): {'light': 165, 'sky': 3946, 'bound': 81, 'emissive': 98, 'tiles3': 26, 'alive4': 1024, 'alive8': 143},
    ('three_ends_huge', 'small'): {'light': 155, 'sky': 3929, 'bound': 85, 'emissive': 121, 'tiles3': 26, 'alive4': 1027, 'alive8': 144, 'self_hits': 2},
    ('closed_room_far', 'pairs'): {'sky': 11, 'bound': 4279, 'tiles3': 3, 'alive4': 4288, 'alive8': 4281, 'self_hits': 12},
    ('three_ends_far', 'odd'): {'light': 155, 'sky': 3929, 'bound': 85, 'emissive': 121, 'tiles3': 26, 'alive4': 1027, 'alive8': 144, 'self_hits': 2},
}


# ------------------------------------------------------------------------------------------ the oracle's frame
def configure(cfg, scene, max_segments=SEGMENTS, spp=1):
    """a config (the oracle's or the library's) set for a scene"""
    cfg.max_segments, cfg.samples_per_pixel = max_segments, spp
    cfg.fov_slope, cfg.pixel_jitter, cfg.light_radius = scene.slope, scene.jitter, scene.light_radius
    return cfg


def oracle_frame(O, scene, W, H, max_segments=SEGMENTS, spp=1, frame=0, rows=None):
    """oracle.raytrace_seq_mat of the scene (O: the oracle module): dict of IMAGE, HIT_ID (full frame; rows [y0, y1) computed),
    rays, seq_id, seq_n, seq_end"""
    from gbuffer_scenes import fill_push_constants
    cfg = configure(O.config_default(W, H), scene, max_segments, spp)
    pc = fill_push_constants(O.PushConstants(), push_constants(scene), frame)
    tri_mat = None if scene.materials is None else O.material_records(scene.tri_material, scene.materials)
    y0, y1 = rows or (0, H)
    image, rays, hit, seq_id, seq_n, seq_end, _ = O.raytrace_seq_mat(cfg, pc, scene.tris, tri_mat, y0, y1)
    return dict(IMAGE=image, HIT_ID=hit, rays=rays, seq_id=seq_id, seq_n=seq_n, seq_end=seq_end)
