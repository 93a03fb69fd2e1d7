"""Scenes for K2's three shading extensions together — albedo textures, mip levels by ray footprint, specular bounces — and the
ALBEDO plane, seen from INSIDE closed or half-open rooms, so that bounce hits dominate and land at all distances (numpy only; no
fixture, no GPU).  tests/test_shading_ext_cpu.py checks on the oracle what is claimed here, tests/test_shading_ext_gpu.py feeds
the scenes to the HIP kernels and to the oracle's path loop with the extensions (oracle_raytrace_ext).

Every scene exists in the three forms of tests/pathtrace_scenes.py (small: brute force; pairs: the BVH over fan pairs; odd: the BVH
over triangles) and carries, per triangle of its BASE mesh, a material, a uv record and a texture index:

  textured_room         the closed room of pathtrace_scenes; five walls read five textures of distinct texels (33 x 17, 8 x 8, 16 x 4
                        mip-mapped, the 16 x 4 one nearest; 3 x 5 without a chain, 1 x 1 with a chain of one level), the floor is untextured, one triangle
                        of the far wall has a uv triangle of zero area (level 0 by rule), one emitter under the ceiling
  glossy_textured_room  the same room; walls +x, +y, +z specular with g = 0, 0.3, 1 (specular_scenes.MIXED_G), the floor with
                        g = 2^-24; Ks differs from Kd, and the specular walls stay textured (Ks x texel)
  mirror_corridor       two facing mirrors 0.7 apart (one of them textured), textured diffuse end walls and floor, open to the sky
                        above; glossy strips (g = 0.3 and 1) on the floor absorb paths; paths live long between the mirrors
  instanced_pair        one box (textured, three walls specular, its top emissive) three times: scaled by 3 around the camera, and
                        translated and rotated inside that room.  Triangle id reads record (id - 1) % n_base; the scaled instance's
                        texel density, and hence its level, differs from the others'

MEASURED holds the oracle's counts the CPU test takes its floors from."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import pathtrace_scenes as P
import specular_scenes as S
import texture_mip_scenes as MS
import texture_scenes as TS

F32 = np.float32
SHAPES = ((96, 12), (97, 13))                 # as tests/test_trace_shading_gpu.py: a partial tile column; a partial tile row, a 1-pixel column
SEGMENTS = 9
SCENES = ("textured_room", "glossy_textured_room", "mirror_corridor", "instanced_pair")
NEAREST, MIPMAP, MIPS_GIVEN = MS.NEAREST, MS.MIPMAP, MS.MIPS_GIVEN

# scene: a pathtrace_scenes.Scene (tris: the world triangles, None for an instanced scene until world() poses it; tri_material per
# BASE triangle); spec {material: (Ks, g)}; tri_uv [b, 6], tri_texture [b] per base triangle; images: level 0 of every texture;
# tex_flags: its flags in the mixed atlas; mesh (xyz, idx) and xforms [i, 3, 4] of an instanced scene
Shading = namedtuple("Shading", "scene spec tri_uv tri_texture images tex_flags mesh xforms")


def _frozen(a, dtype=F32):
    return P._frozen(a, dtype)


# ------------------------------------------------------------------------------------------ textures
def atlas(sh, mode):
    """(descriptors [n, 4] u32, texels [m, 4] f32) for rtpt_scene_set_textures.  mode 1: no texture has a mip flag (NEAREST stays);
    mode 2: the mixed atlas, the library generates the chains"""
    desc, texels = TS.atlas(sh.images)
    flags = np.asarray(sh.tex_flags, np.uint32)
    desc[:, 3] = flags & NEAREST if mode == 1 else flags
    return desc, texels


def given_atlas(sh, chains):
    """the atlas of whole chains (MS.chain_atlas with RTPT_TEX_MIPS_GIVEN) with the scene's NEAREST flags"""
    desc, texels = MS.chain_atlas(chains, 0, True)
    desc[:, 3] |= np.asarray(sh.tex_flags, np.uint32) & NEAREST
    return desc, texels


def oracle_textures(desc, texels, level_row):
    """what oracle.raytrace_ext reads for the atlas the library is given: (descriptors, texels, level table).  A texture with
    RTPT_TEX_MIPMAP alone gets the levels of MS.build_chain appended behind the atlas, one with RTPT_TEX_MIPS_GIVEN reads the levels
    that follow its level 0, any other has one level.  level_row: oracle.level_row"""
    desc = np.asarray(desc, np.uint32).reshape(-1, 4)
    parts, end, rows = [np.asarray(texels, F32).reshape(-1, 4)], len(texels), []
    for w, h, first, flags in desc.tolist():
        firsts = [first]
        if flags & MIPMAP and flags & MIPS_GIVEN:
            for lw, lh in MS.chain_dims(w, h)[:-1]:
                firsts.append(firsts[-1] + lw * lh)
        elif flags & MIPMAP:
            for level in MS.build_chain(parts[0][first:first + w * h].reshape(h, w, 4))[1:]:
                firsts.append(end)
                parts.append(level.reshape(-1, 4))
                end += level.shape[0] * level.shape[1]
        rows.append(level_row(firsts))
    return desc, np.concatenate(parts), np.stack(rows)


def random_chains(sh, seed=3):
    """a chain no box filter made for every texture of the scene (level 0 is NOT the scene's image)"""
    return [MS.random_chain(im.shape[1], im.shape[0], seed + k) for k, im in enumerate(sh.images)]


# ------------------------------------------------------------------------------------------ building blocks
def _quads_of(form, quads, qmat, n):
    quads, qmat = np.asarray(quads, np.float64), np.asarray(qmat)
    if form != "small":
        quads, src = P._tessellate(quads, n)
        qmat = qmat[src]
    return P._with_form(form, quads, qmat)


def _uv(n_tris, tri_wall, scale, seed):
    """TS.random_uv (-2.5 ... 3.5: several repeats, negative) per triangle, scaled per wall"""
    uv = TS.random_uv(n_tris, seed).astype(np.float64)
    return (uv * np.asarray(scale, np.float64)[tri_wall][:, None]).astype(F32)


# texture k of the rooms: (width, height, seed of TS.distinct_image, flags in the mixed atlas)
ROOM_TEXTURES = ((33, 17, 1, MIPMAP), (8, 8, 2, MIPMAP), (16, 4, 3, MIPMAP | NEAREST), (3, 5, 4, 0), (1, 1, 5, MIPMAP))
# wall (-x, +x, -y, +y, -z, +z) -> texture + 1 (0: untextured) and the scale of its uv
ROOM_WALL_TEXTURE = (3, 2, 0, 4, 1, 5)
ROOM_UV_SCALE = (0.25, 0.5, 1.0, 1.0, 0.125, 1.0)
EMITTER = [(-0.5, 0.95, -1.5), (0.3, 0.95, -1.5), (0.3, 0.95, -0.9), (-0.5, 0.95, -0.9)]
EMITTER_KE = (6.0, 5.0, 3.0)
ROOM_KS = {1: (0.875, 0.75, 0.625), 3: (0.75, 0.875, 0.5), 5: (0.625, 0.5, 0.875), 2: (0.5, 0.625, 0.75)}
ROOM_G = dict(S.MIXED_G)
ROOM_G[2] = 2.0 ** -24


def _images(textures):
    return tuple(_frozen(TS.distinct_image(w, h, seed)) for w, h, seed, _ in textures), tuple(f for _, _, _, f in textures)


@lru_cache(maxsize=None)
def textured_room(form="small"):
    quads = np.concatenate([P._box_quads(*P.ROOM), np.array([EMITTER], np.float64)])
    tris, wall = _quads_of(form, quads, np.arange(7), 3)           # 14 / 126 (+ 1) triangles; "wall" 6 is the emitter
    materials = P._materials(P.WALL_KD, (EMITTER_KE,))
    scene = P.Scene("textured_room", form, tris, P.ROOM_CAM, P.REF_SLOPE, 0.375, P.LIGHT_FAR, 0.2, wall, materials)
    tri_texture = np.asarray(ROOM_WALL_TEXTURE + (0,), np.uint32)[wall]
    tri_uv = np.array(_uv(len(tris), wall, ROOM_UV_SCALE + (1.0,), 21))
    flat = np.flatnonzero(wall == 4)[1::4]                         # triangles of the far wall: uv on one line, zero texel area
    tri_uv[flat] = F32([0.125, 0.25, 0.625, 0.75, 1.125, 1.25])
    images, flags = _images(ROOM_TEXTURES)
    return Shading(scene, None, _frozen(tri_uv), _frozen(tri_texture, np.uint32), images, flags, None, None)


@lru_cache(maxsize=None)
def glossy_textured_room(form="small"):
    sh = textured_room(form)
    spec = {m: (ROOM_KS[m], g) for m, g in ROOM_G.items()}
    return sh._replace(scene=sh.scene._replace(name="glossy_textured_room"), spec=spec)


# ------------------------------------------------------------------------------------------ the corridor of mirrors
CORRIDOR_CAM = (0.05, 0.9, 2.0)
CORRIDOR = dict(x=(-0.35, 0.35), y=(0.0, 4.0), z=(-5.0, 3.0))
CORRIDOR_TEXTURES = ((33, 17, 6, MIPMAP), (16, 4, 7, MIPMAP), (8, 8, 8, MIPMAP | NEAREST), (3, 5, 9, 0))
# materials: 0, 1 the mirrors (-x, +x), 2 the floor, 3 the far wall, 4 the wall behind the camera, 5 a strip with g = 0.3, 6 one with g = 1
CORRIDOR_KD = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0.75, 0.625, 0.5), (0.875, 0.75, 0.75), (0.5, 0.75, 0.875), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
CORRIDOR_SPEC = {0: ((0.9375, 0.875, 0.9375), 0.0), 1: ((0.875, 0.9375, 0.875), 0.0), 5: ((0.75, 0.5, 0.25), 0.3), 6: ((0.25, 0.5, 0.75), 1.0)}
CORRIDOR_TEXTURE = (0, 2, 1, 2, 3, 4, 0)      # material -> texture + 1: the +x mirror is textured too (Ks x texel)
CORRIDOR_UV_SCALE = (1.0, 0.25, 0.5, 0.25, 1.0, 1.0, 1.0)


@lru_cache(maxsize=None)
def mirror_corridor(form="small"):
    (x0, x1), (y0, y1), (z0, z1) = CORRIDOR["x"], CORRIDOR["y"], CORRIDOR["z"]
    box = P._box_quads((x0, y0, z0), (x1, y1, z1))
    strip = lambda za, zb, xa, xb: [(xa, 0.01, za), (xb, 0.01, za), (xb, 0.01, zb), (xa, 0.01, zb)]
    quads = [box[0], box[1], box[2], box[4], box[5],               # no +y wall: open to the sky
             strip(-1.5, 0.5, -0.3, 0.0), strip(-3.5, -2.0, -0.1, 0.3), strip(0.8, 1.6, 0.0, 0.3)]
    qmat = [0, 1, 2, 3, 4, 5, 6, 6]
    tris, mat = _quads_of(form, quads, qmat, 3)                    # 16 / 144 (+ 1) triangles
    scene = P.Scene("mirror_corridor", form, tris, CORRIDOR_CAM, P.REF_SLOPE, 0.375, P.LIGHT_FAR, 0.2, mat, P._materials(CORRIDOR_KD))
    tri_texture = np.asarray(CORRIDOR_TEXTURE, np.uint32)[mat]
    tri_uv = _uv(len(tris), mat, CORRIDOR_UV_SCALE, 22)
    images, flags = _images(CORRIDOR_TEXTURES)
    return Shading(scene, dict(CORRIDOR_SPEC), _frozen(tri_uv), _frozen(tri_texture, np.uint32), images, flags, None, None)


# ------------------------------------------------------------------------------------------ one box, three instances
BOX_HALF = 0.4
BOX_CAM = (0.05, 0.1, 1.0)
BOX_TEXTURES = ((33, 17, 10, MIPMAP), (8, 8, 11, MIPMAP), (16, 4, 12, MIPMAP | NEAREST), (3, 5, 13, 0))
BOX_WALL_TEXTURE = (1, 2, 3, 0, 1, 4)         # the emissive top reads none
BOX_UV_SCALE = (0.25, 0.5, 0.5, 1.0, 0.125, 1.0)
BOX_KD = ((0.75, 0.5, 0.5), (0.5, 0.5, 0.5), (0.5, 0.75, 0.5), (0.5, 0.5, 0.5), (0.5, 0.625, 0.875), (0.875, 0.75, 0.5))
BOX_KE = (3.0, 2.5, 2.0)                      # of wall +y
BOX_SPEC = {1: ((0.875, 0.9375, 0.75), 0.0), 2: ((0.75, 0.625, 0.875), 1.0), 4: ((0.625, 0.875, 0.75), 0.3)}


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def _xform(m, t):
    return np.concatenate([np.asarray(m, np.float64), np.asarray(t, np.float64)[:, None]], 1)


def box_xforms(moved=False):
    """[3, 3, 4] float32: a scale of 3 (the room around the camera), a translation, a rotation with a translation; `moved`: other
    transforms of the same kinds (the camera stays inside the scaled instance, the small boxes inside it too)"""
    if moved:
        x = [_xform(3.0 * np.eye(3), (0.1, 0.05, -0.1)), _xform(np.eye(3), (-0.45, -0.3, -0.2)),
             _xform(_rotation((0.3, 1.0, -0.2), np.deg2rad(-50.0)), (0.5, -0.45, -0.35))]
    else:
        x = [_xform(3.0 * np.eye(3), (0.0, 0.0, 0.0)), _xform(np.eye(3), (-0.6, -0.7, -0.4)),
             _xform(_rotation((0.2, 1.0, 0.1), np.deg2rad(30.0)), (0.4, -0.2, -0.45))]
    return _frozen(np.array(x))


@lru_cache(maxsize=None)
def instanced_pair(form="small"):
    h = BOX_HALF
    tris, wall = _quads_of(form, P._box_quads((-h, -h, -h), (h, h, h)), np.arange(6), 2)      # 12 / 48 (+ 1) base triangles
    kd = np.array(BOX_KD, F32)
    materials = np.concatenate([kd, np.zeros((6, 3), F32)], 1)
    materials[3, 3:] = BOX_KE
    scene = P.Scene("instanced_pair", form, None, BOX_CAM, P.REF_SLOPE, 0.375, P.LIGHT_FAR, 0.2, wall, _frozen(materials))
    tri_texture = np.asarray(BOX_WALL_TEXTURE, np.uint32)[wall]
    tri_uv = _uv(len(tris), wall, BOX_UV_SCALE, 23)
    images, flags = _images(BOX_TEXTURES)
    xyz = _frozen(tris.reshape(-1, 3))
    idx = _frozen(np.arange(len(xyz)).reshape(-1, 3), np.uint32)
    return Shading(scene, dict(BOX_SPEC), _frozen(tri_uv), _frozen(tri_texture, np.uint32), images, flags, (xyz, idx), box_xforms())


def world(O, sh, xforms=None):
    """the scene with its world triangles: an instanced scene flattened by the oracle (the library's arithmetic, bit for bit) under
    `xforms` (default: its own), any other as it is"""
    if sh.mesh is None:
        return sh
    xf = sh.xforms if xforms is None else xforms
    return sh._replace(scene=sh.scene._replace(tris=_frozen(O.flatten(sh.mesh[0], sh.mesh[1], xf))), xforms=xf)


def scene(name, form="small"):
    return {"textured_room": textured_room, "glossy_textured_room": glossy_textured_room, "mirror_corridor": mirror_corridor,
            "instanced_pair": instanced_pair}[name](form)


def n_base(sh):
    return len(sh.tri_texture)


# ------------------------------------------------------------------------------------------ the oracle's frame
def oracle_frame(O, sh, W, H, segments=SEGMENTS, spp=1, tex=2, spec=True, demod=False, rows=None, textures=None, frame=0, records=True):
    """oracle.raytrace_ext of a scene posed by world().  tex 0: no textures, 1: the atlas without mip flags, 2: the mixed atlas;
    `textures` = (descriptors, texels) replaces the scene's atlas (a given chain); spec False: every material diffuse (Kd);
    demod: with the ALBEDO plane"""
    from gbuffer_scenes import fill_push_constants
    sc = sh.scene
    cfg = P.configure(O.config_default(W, H), sc, segments, spp)
    pc = fill_push_constants(O.PushConstants(), P.push_constants(sc), frame)
    tri_mat = O.material_records_ext(sc.tri_material, sc.materials, sh.spec if spec else None)
    tx = levels = None
    if tex:
        desc, texels, levels = oracle_textures(*(textures or atlas(sh, tex)), O.level_row)
        tx = (sh.tri_uv, sh.tri_texture, desc, texels)
        if not (desc[:, 3] & MIPMAP).any():
            levels = None
    y0, y1 = rows or (0, H)
    return O.raytrace_ext(cfg, pc, sc.tris, tri_mat, n_base(sh), y0, y1, textures=tx, levels=levels, bounce_spread=MS.BOUNCE_SPREAD,
                          specular=spec and bool(sh.spec), want_albedo=demod, records=records)


# ------------------------------------------------------------------------------------------ what a dump says
def counts(O, sh, r, window):
    """the preconditions of tests/test_shading_ext_gpu.py on the dump of a 1 spp frame `r` of oracle_frame(tex=2, spec=True)"""
    code, seq_id, seq_n = r["rec_code"], r["seq_id"].astype(np.int64), r["seq_n"]
    k = np.arange(code.shape[-1])[None, None, :]
    hit = (code & O.REC_HIT) != 0
    ended_here = (code & O.REC_ABSORBED) != 0
    bounce = (hit | ended_here) & (k >= 1)                         # closest hits at segment >= 1 that were shaded
    textured = bounce & ((code & O.REC_TEXTURED) != 0)
    rec = (seq_id - 1) % n_base(sh)
    tex_of = sh.tri_texture[np.where(seq_id > 0, rec, 0)].astype(np.int64)
    flags = np.asarray(sh.tex_flags + (0,), np.int64)[tex_of - 1]
    levels = np.array([len(MS.chain_dims(im.shape[1], im.shape[0])) for im in sh.images] + [1])[tex_of - 1]
    mipped = textured & ((flags & MIPMAP) != 0) & (levels > 1)
    lod = r["rec_lod"][mipped]
    g = np.zeros(len(sh.scene.materials))
    is_spec = np.zeros(len(sh.scene.materials), bool)
    for m, (_, gm) in (sh.spec or {}).items():
        g[m], is_spec[m] = gm, True
    mat = sh.scene.tri_material[np.where(seq_id > 0, rec, 0)]
    specular = bounce & ((code & O.REC_SPECULAR) != 0)
    assert np.array_equal(specular, bounce & is_spec[mat]), "the code names the material's kind"
    out = dict(tex_bounce=int(textured.sum()), lod_levels=len(np.unique(np.floor(lod))), lod_fraction=int((lod % 1 != 0).sum()),
               albedos=len(np.unique(np.ascontiguousarray(r["rec_albedo"][bounce]).view(np.uint32), axis=0)),
               mirror=int((specular & (g[mat] == 0)).sum()), glossy=int((specular & (g[mat] > 0)).sum()),
               diffuse=int((bounce & ~specular).sum()), absorbed=int((r["seq_end"] == O.END_ABSORBED).sum()),
               alive=P.alive_after(seq_n, [window])[0], alive1=P.alive_after(seq_n, [1])[0])
    if sh.mesh is not None:
        inst = (seq_id - 1) // n_base(sh)
        for i in range(len(sh.xforms)):
            out[f"instance{i}"] = int((bounce & (inst == i)).sum())
    return out


# what every scene must show (a count of 0 is left out of MEASURED, so no floor is met by nothing)
REQUIRED = {
    "textured_room": ("tex_bounce", "lod_levels", "lod_fraction", "albedos", "diffuse", "alive", "alive1"),
    "glossy_textured_room": ("tex_bounce", "lod_levels", "lod_fraction", "albedos", "mirror", "glossy", "diffuse", "absorbed", "alive", "alive1"),
    "mirror_corridor": ("tex_bounce", "lod_levels", "lod_fraction", "albedos", "mirror", "glossy", "diffuse", "absorbed", "alive", "alive1"),
    "instanced_pair": ("tex_bounce", "lod_levels", "lod_fraction", "albedos", "mirror", "glossy", "diffuse", "absorbed", "alive", "alive1",
                       "instance0", "instance1", "instance2"),
}
MIN_LOD_LEVELS = 4                            # different integer parts of the level among bounce hits on mip-mapped textures

# what the oracle measured at SHAPES[0], SEGMENTS, frame 0, 1 spp, the mixed atlas, specular on (tests/test_shading_ext_cpu.py asserts
# at least half of each, and MIN_LOD_LEVELS whatever was measured): `alive` is the number of paths alive behind the form's first
# window (4 brute force, 8 BVH), alive1 behind segment 1
MEASURED = {
    ('textured_room', 'small'): {'tex_bounce': 6623, 'lod_levels': 5, 'lod_fraction': 1273, 'albedos': 4532, 'diffuse': 8839, 'alive': 1120, 'alive1': 1152},
    ('textured_room', 'pairs'): {'tex_bounce': 6623, 'lod_levels': 6, 'lod_fraction': 2085, 'albedos': 4490, 'diffuse': 8839, 'alive': 1075, 'alive1': 1152},
    ('textured_room', 'odd'): {'tex_bounce': 6623, 'lod_levels': 6, 'lod_fraction': 2085, 'albedos': 4490, 'diffuse': 8839, 'alive': 1075, 'alive1': 1152},
    ('glossy_textured_room', 'small'): {'tex_bounce': 6303, 'lod_levels': 5, 'lod_fraction': 1207, 'albedos': 4201, 'mirror': 1032, 'glossy': 5022, 'diffuse': 2199, 'absorbed': 166, 'alive': 1061, 'alive1': 1152},
    ('glossy_textured_room', 'pairs'): {'tex_bounce': 6303, 'lod_levels': 6, 'lod_fraction': 1945, 'albedos': 4165, 'mirror': 1032, 'glossy': 5022, 'diffuse': 2199, 'absorbed': 166, 'alive': 913, 'alive1': 1152},
    ('glossy_textured_room', 'odd'): {'tex_bounce': 6303, 'lod_levels': 6, 'lod_fraction': 1945, 'albedos': 4165, 'mirror': 1032, 'glossy': 5022, 'diffuse': 2199, 'absorbed': 166, 'alive': 913, 'alive1': 1152},
    ('mirror_corridor', 'small'): {'tex_bounce': 4742, 'lod_levels': 6, 'lod_fraction': 329, 'albedos': 4706, 'mirror': 7800, 'glossy': 82, 'diffuse': 844, 'absorbed': 22, 'alive': 1133, 'alive1': 1152},
    ('mirror_corridor', 'pairs'): {'tex_bounce': 4742, 'lod_levels': 6, 'lod_fraction': 987, 'albedos': 4654, 'mirror': 7800, 'glossy': 82, 'diffuse': 844, 'absorbed': 22, 'alive': 1025, 'alive1': 1152},
    ('mirror_corridor', 'odd'): {'tex_bounce': 4742, 'lod_levels': 6, 'lod_fraction': 987, 'albedos': 4654, 'mirror': 7800, 'glossy': 82, 'diffuse': 844, 'absorbed': 22, 'alive': 1025, 'alive1': 1152},
    ('instanced_pair', 'small'): {'tex_bounce': 4231, 'lod_levels': 5, 'lod_fraction': 700, 'albedos': 3795, 'mirror': 975, 'glossy': 1470, 'diffuse': 1786, 'absorbed': 80, 'alive': 625, 'alive1': 1140, 'instance0': 3373, 'instance1': 251, 'instance2': 607},
    ('instanced_pair', 'pairs'): {'tex_bounce': 4231, 'lod_levels': 6, 'lod_fraction': 1800, 'albedos': 3770, 'mirror': 975, 'glossy': 1470, 'diffuse': 1786, 'absorbed': 80, 'alive': 281, 'alive1': 1140, 'instance0': 3373, 'instance1': 251, 'instance2': 607},
    ('instanced_pair', 'odd'): {'tex_bounce': 4231, 'lod_levels': 6, 'lod_fraction': 1800, 'albedos': 3770, 'mirror': 975, 'glossy': 1470, 'diffuse': 1786, 'absorbed': 80, 'alive': 281, 'alive1': 1140, 'instance0': 3373, 'instance1': 251, 'instance2': 607},
}
