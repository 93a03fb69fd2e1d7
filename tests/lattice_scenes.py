"""Scenes that make every cell of K2's shading lattice visible — TEX 0 / 1 / 2 x DEMOD x SPEC 2 .. 6 — for test_lattice_*.py
(numpy only; no fixture, no GPU).  Rooms seen from inside, in the three forms of tests/pathtrace_scenes.py (small: brute force;
pairs: the BVH over fan pairs; odd: the BVH over triangles), built from the pieces of tests/shading_scenes.py: its textured, partly
glossy room, its mixed atlas of distinct texels, its box of three instances.

  lattice_room       shading_scenes.glossy_textured_room (five walls read five textures, walls +x, +y, +z and the floor specular) with
                     a closed, TEXTURED glass block between the camera and the far wall: primary rays cross it and meet the block's
                     inner faces and the mip-mapped walls behind it at several distances, along refracted directions.  Two
                     emissive quads of unequal area x Ke (a large dim one under the ceiling, a small bright one on the far wall, in
                     view: paths end on it at segment 0), one emissive quad whose corners lie on a line (weight 0, never hit), a diffuse
                     occluder under the large lamp, and the sphere light inside the room, in view
  lattice_instances  shading_scenes.instanced_pair's box (its top emissive) with a glass pane, a small bright lamp and a degenerate
                     emitter in the BASE mesh, three times: scaled by 3 around the camera, translated, and rotated.  Material,
                     texture and light records are the base triangle's, (id - 1) % n_base, in every SPEC

A Case is a shading_scenes.Shading plus `glass` {material: (colour, ior)}.  setup() gives, per SPEC value of the GPU test, what the
walker (tests/path_walker.py) and the upload take.  MEASURED holds the walker's counts tests/test_lattice_cpu.py asserts."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import dielectric_scenes as DS
import path_walker as WK
import nee_paths as NP
import nee_power as PW
import nee_sphere as NS
import pathtrace_scenes as P
import shading_scenes as SS

F32 = np.float32
SHAPES = SS.SHAPES
SEGMENTS = SS.SEGMENTS
SCENES = ("lattice_room", "lattice_instances")
SPECS = (2, 3, 4, 5, 6, "4-without-list")
NEE, SPHERE, POWER = 0x10000, 0x20000, 0x40000
SPEC_FLAGS = {2: 0, 3: NEE, 4: NEE | SPHERE, 5: NEE | POWER, 6: NEE | POWER | SPHERE, "4-without-list": SPHERE}

Case = namedtuple("Case", "sh glass")

GLASS = ((0.75, 0.875, 1.0), DS.GLASS_IOR)


# ------------------------------------------------------------------------------------------ the room
BLOCK_LO, BLOCK_HI = (-1.0, -0.7, -1.6), (0.6, 0.5, -1.2)
BIG_LAMP = SS.EMITTER                                                     # 0.8 x 0.6 under the ceiling
BIG_KE = SS.EMITTER_KE
SMALL_LAMP = [(1.3, -0.3, -2.95), (1.6, -0.3, -2.95), (1.6, 0.1, -2.95), (1.3, 0.1, -2.95)]      # on the far wall, facing the camera
SMALL_KE = (24.0, 20.0, 16.0)
LINE_LAMP = [(-1.0, 0.875, 0.25), (-0.75, 0.875, 0.25), (-0.5, 0.875, 0.25), (-0.25, 0.875, 0.25)]   # four points on a line: no area
LINE_KE = (5.0, 5.0, 5.0)
OCCLUDER = [(-0.7, 0.6, -1.7), (0.4, 0.6, -1.7), (0.4, 0.6, -0.8), (-0.7, 0.6, -0.8)]
OCCLUDER_KD = (0.625, 0.5, 0.75)
ROOM_LIGHT = (1.2, 0.1, -0.8)                                              # the sphere light, inside the room and in view
# "wall" -> texture + 1 and uv scale: 0 .. 5 the walls (shading_scenes), 6 the glass, 7 the occluder, 8 .. 10 the emitters
ROOM_TEXTURE = SS.ROOM_WALL_TEXTURE + (1, 2, 0, 0, 0)
ROOM_UV_SCALE = SS.ROOM_UV_SCALE + (0.25, 0.5, 1.0, 1.0, 1.0)


@lru_cache(maxsize=None)
def lattice_room(form="small"):
    quads = np.concatenate([P._box_quads(*P.ROOM), P._box_quads(BLOCK_LO, BLOCK_HI), np.array([OCCLUDER, BIG_LAMP, SMALL_LAMP, LINE_LAMP], np.float64)])
    part = np.array([0, 1, 2, 3, 4, 5] + [6] * 6 + [7, 8, 9, 10])
    tris, mat = SS._quads_of(form, quads, part, 3)                        # 32 / 288 (+ 1) triangles
    materials = P._materials(P.WALL_KD + ((0.5, 0.5, 0.5), OCCLUDER_KD), (BIG_KE, SMALL_KE, LINE_KE))
    scene = P.Scene("lattice_room", form, tris, P.ROOM_CAM, P.REF_SLOPE, 0.375, ROOM_LIGHT, 0.2, mat, materials)
    tri_texture = np.asarray(ROOM_TEXTURE, np.uint32)[mat]
    tri_uv = SS._uv(len(tris), mat, ROOM_UV_SCALE, 31)
    images, flags = SS._images(SS.ROOM_TEXTURES)
    spec = {m: (SS.ROOM_KS[m], g) for m, g in SS.ROOM_G.items()}
    sh = SS.Shading(scene, spec, SS._frozen(tri_uv), SS._frozen(tri_texture, np.uint32), images, flags, None, None)
    return Case(sh, {6: GLASS})


# ------------------------------------------------------------------------------------------ one box with a pane, three instances
PANE = [(-0.3, -0.3, -0.15), (0.3, -0.3, -0.15), (0.3, 0.25, -0.15), (-0.3, 0.25, -0.15)]        # its stored normal looks down +z
BOX_LAMP = [(0.125, 0.34375, 0.125), (0.25, 0.34375, 0.125), (0.25, 0.34375, 0.25), (0.125, 0.34375, 0.25)]
BOX_LINE = [(-0.25, 0.3125, -0.25), (-0.125, 0.3125, -0.25), (0.0, 0.3125, -0.25), (0.125, 0.3125, -0.25)]
BOX_TEXTURE = SS.BOX_WALL_TEXTURE + (2, 0, 0)
BOX_UV_SCALE = SS.BOX_UV_SCALE + (0.5, 1.0, 1.0)
BOX_LIGHT = (-0.5, 0.2, 0.1)


@lru_cache(maxsize=None)
def lattice_instances(form="small"):
    h = SS.BOX_HALF
    quads = np.concatenate([P._box_quads((-h, -h, -h), (h, h, h)), np.array([PANE, BOX_LAMP, BOX_LINE], np.float64)])
    tris, mat = SS._quads_of(form, quads, np.arange(9), 2)                # 18 / 72 (+ 1) base triangles
    materials = np.zeros((9, 6), F32)
    materials[:6, :3] = np.array(SS.BOX_KD, F32)
    materials[6:, :3] = 0.5
    materials[3, 3:], materials[7, 3:], materials[8, 3:] = SS.BOX_KE, SMALL_KE, LINE_KE
    scene = P.Scene("lattice_instances", form, None, SS.BOX_CAM, P.REF_SLOPE, 0.375, BOX_LIGHT, 0.2, mat, SS._frozen(materials))
    tri_texture = np.asarray(BOX_TEXTURE, np.uint32)[mat]
    tri_uv = SS._uv(len(tris), mat, BOX_UV_SCALE, 33)
    images, flags = SS._images(SS.BOX_TEXTURES)
    xyz = SS._frozen(tris.reshape(-1, 3))
    idx = SS._frozen(np.arange(len(xyz)).reshape(-1, 3), np.uint32)
    sh = SS.Shading(scene, dict(SS.BOX_SPEC), SS._frozen(tri_uv), SS._frozen(tri_texture, np.uint32), images, flags, (xyz, idx), SS.box_xforms())
    return Case(sh, {6: GLASS})


def case(O, name, form="small", xforms=None):
    """the Case with its world triangles (shading_scenes.world)"""
    c = {"lattice_room": lattice_room, "lattice_instances": lattice_instances}[name](form)
    return c._replace(sh=SS.world(O, c.sh, xforms))


def n_instances(c):
    return len(c.sh.xforms) if c.sh.mesh is not None else 1


# ------------------------------------------------------------------------------------------ what a SPEC value walks and uploads
def setup(O, c, spec):
    """dict(rec, lights, sphere, power) for path_walker.walk at a SPEC value of SPECS: 2 the glass and the glossy materials, no
    light sample; 3 / 4 / 5 / 6 the list, with the sphere (4, 6) and the weighted pick (5, 6); "4-without-list": no material table at
    all — the normal-keyed colours per POSED triangle, no list, the sphere sample alone"""
    sc = c.sh.scene
    if spec == "4-without-list":
        return dict(rec=NS.normal_keyed_records(O, sc), lights=np.zeros(0, np.uint32), sphere=True, power=False)
    rec = DS.records(sc, c.sh.spec, c.glass)
    flags = SPEC_FLAGS[spec]
    lights = NP.light_list(sc, n_instances(c), rec) if flags & NEE else np.zeros(0, np.uint32)
    return dict(rec=rec, lights=lights, sphere=bool(flags & SPHERE), power=bool(flags & POWER))


def table(O, c):
    """the cumulative table of the Case's list on its posed triangles"""
    s = setup(O, c, 5)
    return PW.table(PW.weights(O, c.sh.scene.tris, s["rec"], s["lights"]))


def weightless(O, c):
    """the entries of the Case's list whose weight is exactly 0 (the degenerate emitter wherever its pose keeps it on a line)"""
    s = setup(O, c, 5)
    return np.flatnonzero(PW.counted(PW.weights(O, c.sh.scene.tris, s["rec"], s["lights"])) == 0)


# ------------------------------------------------------------------------------------------ what the scenes must show
# per (scene, form), by the walker at SHAPES[0], SEGMENTS, frame 0, 1 spp, the mixed atlas: SPEC 2's transmitted / reflected, the
# levels behind glass and the paths alive behind segment 1 and behind the form's window; SPEC 6's samples (SPEC 5 and 3 for the picks)
REQUIRED = ("transmitted", "reflected", "mip_behind", "lod_levels_behind", "lod_fraction_behind", "alive1", "alive", "lit", "shadowed",
            "kept", "dropped", "sphere_valid", "sphere_dropped", "sphere_kept", "uniform_picks_weightless")
MIN_LEVELS_BEHIND = 3

MEASURED = {
    ('lattice_room', 'small'): {'transmitted': 1528, 'reflected': 383, 'mip_behind': 2564, 'lod_levels_behind': 6, 'lod_fraction_behind': 662, 'alive1': 1070, 'alive': 997, 'lit': 1553, 'kept': 19, 'dropped': 30, 'sphere_valid': 2066, 'sphere_dropped': 8, 'sphere_kept': 48, 'shadowed': 514, 'uniform_picks_weightless': 680},
    ('lattice_room', 'pairs'): {'transmitted': 1528, 'reflected': 383, 'mip_behind': 2564, 'lod_levels_behind': 6, 'lod_fraction_behind': 1866, 'alive1': 1070, 'alive': 872, 'lit': 1546, 'kept': 19, 'dropped': 30, 'sphere_valid': 2066, 'sphere_dropped': 8, 'sphere_kept': 48, 'shadowed': 521, 'uniform_picks_weightless': 680},
    ('lattice_room', 'odd'): {'transmitted': 1528, 'reflected': 383, 'mip_behind': 2564, 'lod_levels_behind': 6, 'lod_fraction_behind': 1866, 'alive1': 1070, 'alive': 872, 'lit': 1546, 'kept': 19, 'dropped': 30, 'sphere_valid': 2066, 'sphere_dropped': 8, 'sphere_kept': 48, 'shadowed': 521, 'uniform_picks_weightless': 680},
    ('lattice_instances', 'small'): {'transmitted': 648, 'reflected': 124, 'mip_behind': 1659, 'lod_levels_behind': 5, 'lod_fraction_behind': 439, 'alive1': 1021, 'alive': 624, 'lit': 1207, 'kept': 276, 'dropped': 362, 'sphere_valid': 1513, 'sphere_dropped': 41, 'sphere_kept': 47, 'shadowed': 322, 'uniform_picks_weightless': 432},
    ('lattice_instances', 'pairs'): {'transmitted': 648, 'reflected': 124, 'mip_behind': 1659, 'lod_levels_behind': 6, 'lod_fraction_behind': 786, 'alive1': 1021, 'alive': 266, 'lit': 1222, 'kept': 276, 'dropped': 362, 'sphere_valid': 1513, 'sphere_dropped': 41, 'sphere_kept': 47, 'shadowed': 316, 'uniform_picks_weightless': 496},
    ('lattice_instances', 'odd'): {'transmitted': 648, 'reflected': 124, 'mip_behind': 1659, 'lod_levels_behind': 6, 'lod_fraction_behind': 786, 'alive1': 1021, 'alive': 266, 'lit': 1222, 'kept': 276, 'dropped': 362, 'sphere_valid': 1513, 'sphere_dropped': 41, 'sphere_kept': 47, 'shadowed': 316, 'uniform_picks_weightless': 496},
}


def measure(O, name, form):
    """the counts of REQUIRED (tests/test_lattice_cpu.py asserts at least half of each measured count, and > 0)"""
    c = case(O, name, form)
    W, H = SHAPES[0]
    tex = WK.textures(c.sh, 2)
    r2 = WK.walk(O, c.sh.scene, W, H, SEGMENTS, tex=tex, **setup(O, c, 2))
    r6 = WK.walk(O, c.sh.scene, W, H, SEGMENTS, tex=tex, **setup(O, c, 6))
    r3 = WK.walk(O, c.sh.scene, W, H, SEGMENTS, tex=tex, **setup(O, c, 3))
    dead = weightless(O, c)
    out = {k: int(r2[k]) for k in ("transmitted", "reflected", "mip_behind", "lod_levels_behind", "lod_fraction_behind")}
    out["alive1"], out["alive"] = P.alive_after(r2["seq_n"], [1, P.window_of(None, form)])
    out.update({k: int(r6[k]) for k in ("lit", "kept", "dropped", "sphere_valid", "sphere_dropped", "sphere_kept")})
    out["shadowed"] = int(r6["queries"] - r6["lit"])
    out["uniform_picks_weightless"] = int(r3["picks"][dead].sum())
    assert len(dead) and int(r6["picks"][dead].sum()) == 0, "an entry of weight 0 is never picked by weight"
    return out
