"""The light list of next-event estimation (RTPT_FLAG_EXT_NEE; csrc/light_sample.hpp states the rules) and its scenes for
test_nee_paths_*.py.

light_list restates csrc/light_list_host.hpp; the scenes are the receiver with an occluder, with two lamps, and translated copies.
The light sample itself is nee_scenes.sample32, and the paths are walked by tests/path_walker.py (`lights=`): with an empty list it
takes no light draw, which tests/test_nee_paths_cpu.py asks for bit by bit against the recorded frames of the walker without one."""
from functools import lru_cache

import numpy as np

import nee_scenes as N
import pathtrace_scenes as P
from dielectric_scenes import records

F32, U32 = np.float32, np.uint32


# ------------------------------------------------------------------------------------------ the light list
def light_list(scene, n_instances=1, rec=None):
    """uint32 [L]: id + 1 of every posed triangle inst * n_base + t whose base triangle's record is emissive, ascending.  rec: the
    per-base-triangle records (dielectric_scenes.records) where some material is specular or dielectric; else the scene's own"""
    rec = records(scene) if rec is None else np.asarray(rec, F32)
    t = np.flatnonzero(rec[:, 7] != 0).astype(np.int64)
    n_base = len(rec)
    ids = (np.arange(n_instances, dtype=np.int64)[:, None] * n_base + t[None, :] + 1).ravel()
    return ids.astype(U32)


# ------------------------------------------------------------------------------------------ scenes
OCCLUDER = np.array([(0.2, -1.0, 0.8), (1.4, -1.0, 0.8), (1.4, 0.6, 0.8), (0.2, 0.6, 0.8)], np.float64)
SMALL_LAMP = np.array([(-1.8, 0.4, 1.5), (-1.5, 0.4, 1.5), (-1.5, 0.8, 1.5), (-1.8, 0.8, 1.5)], np.float64)
SMALL_LAMP_KE = (1.0, 6.0, 3.0)


def _receiver_quads():
    return [[(-2.3, -1.8, 0.0), (2.3, -1.8, 0.0), (2.3, 1.8, 0.0), (-2.3, 1.8, 0.0)], N.RECEIVER_LAMP]


@lru_cache(maxsize=None)
def occluder():
    """nee_scenes.receiver() plus one opaque diffuse quad in the plane z = 0.8, between part of the receiver and the lamp (z = 2) and
    inside the view: pixels whose light samples it stops get no direct term.  Materials: 0 the receiver, 1 the occluder, 2 the lamp"""
    quads = np.array(_receiver_quads()[:1] + [OCCLUDER] + [N.RECEIVER_LAMP], np.float64)
    tris, mat = P._with_form("small", quads, np.array([0, 1, 2]))
    materials = P._materials((N.RECEIVER_KD, (0.25, 0.5, 0.125)), (N.RECEIVER_KE,))
    return P.Scene("nee_occluder", "small", tris, N.RECEIVER_CAM, N.RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)


@lru_cache(maxsize=None)
def two_lamps():
    """the receiver under two lamps of unequal area and colour — the trapezoid and a small quad on the other side, nearer — and one
    DEGENERATE emissive triangle (three points on a line): it is in the list, its samples are never valid and no ray hits it.
    Materials: 0 the receiver, 1 the trapezoid, 2 the small lamp and the degenerate triangle"""
    quads = np.array(_receiver_quads() + [SMALL_LAMP], np.float64)
    tris, mat = P._with_form("small", quads, np.array([0, 1, 2]))
    line = np.array([[0.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 1.0, 1.0]], F32)
    tris = P._frozen(np.concatenate([np.asarray(tris, F32).reshape(-1, 9), line]))
    mat = P._frozen(np.concatenate([np.asarray(mat), [2]]).astype(np.asarray(mat).dtype))
    materials = P._materials((N.RECEIVER_KD,), (N.RECEIVER_KE, SMALL_LAMP_KE))
    return P.Scene("nee_two_lamps", "small", tris, N.RECEIVER_CAM, N.RECEIVER_SLOPE, 0.0, P.LIGHT_FAR, 0.2, mat, materials)


def translated(scene, offsets):
    """the scene's mesh as len(offsets) instances, instance i moved by offsets[i]: (instance transforms [n, 12] float32, the posed
    scene the walker takes — every instance's triangles, one record per base triangle).  A translation poses a vertex as v + t, one
    rounding, which is what the flatten's fused arithmetic gives for rows of the identity"""
    base = np.asarray(scene.tris, F32).reshape(-1, 3, 3)
    xf = np.zeros((len(offsets), 3, 4), F32)
    xf[:, 0, 0] = xf[:, 1, 1] = xf[:, 2, 2] = 1
    xf[:, :, 3] = F32(offsets)
    posed = np.concatenate([(base + F32(t)[None, None, :]).astype(F32) for t in offsets]).reshape(-1, 9)
    return xf.reshape(-1, 12), scene._replace(name=scene.name + "_x%d" % len(offsets), tris=P._frozen(posed))
