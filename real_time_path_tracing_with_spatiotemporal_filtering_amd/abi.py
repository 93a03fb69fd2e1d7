"""ctypes binding of the C ABI declared in ``include/rtpt.h`` (``librtpt_hip.so``).

This is the only way Python reaches the hot path: there is no CPU fallback.  ``load()`` raises
``RtptLibraryMissing`` when the HIP library has not been built and every call raises
``RtptError`` on a negative status code, carrying ``rtpt_last_error()``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
# RTPT_LIB_PATH: a differently-built library for compile-time A/B runs on the GPU box (never set in tests or bench lines)
LIB_PATH = os.environ.get("RTPT_LIB_PATH") or os.path.join(PKG_DIR, "librtpt_hip.so")
HEADER_PATH = os.path.join(REPO_DIR, "include", "rtpt.h")

RTPT_OK, RTPT_E_INVALID, RTPT_E_NOMEM, RTPT_E_DEVICE, RTPT_E_NO_SCENE, RTPT_E_NO_GPU = 0, -1, -2, -3, -4, -5
FLAG_EXACT_FILTER, FLAG_FORCE_BVH, FLAG_DIRECT_FILTER, FLAG_NO_PATH_COMPACTION = 0x1, 0x2, 0x4, 0x8
# extension modes (not reference behaviour, see include/rtpt.h)
FLAG_EXT_ADAPTIVE_ALPHA, FLAG_EXT_GAUSS5, FLAG_EXT_POW2_STRIDE, FLAG_EXT_DISOCCLUSION = 0x10, 0x20, 0x40, 0x80
FLAG_EXT_VARIANCE = 0x100
FLAG_SINGLE_LAUNCH_PATHS = 0x200
FLAG_NO_FILTER_FUSION = 0x400
FLAG_EXT_SVGF_VARIANCE = 0x800
FLAG_EXT_MASK = 0x9F0
FLAG_DEVICE_BVH_BUILD = 0x1000  # rtpt_scene_upload builds the tree on the device (csrc/bvh_build.hip)
FLAG_DEVICE_BVH_SAH = 0x2000  # with FLAG_DEVICE_BVH_BUILD: the device SAH builder, the host's tree node for node (csrc/bvh_build_sah.hip)
FLAG_EXT_DEMODULATE = 0x8000  # filter illumination, multiply the first hit's albedo back afterwards (modulate / present); not in FLAG_EXT_MASK
FLAG_DEVICE_FLATTEN = 0x4000  # with FLAG_DEVICE_BVH_BUILD: mesh x transforms -> triangles and the fan-pair test on the device (csrc/scene_flatten.hip)
FLAG_EXT_NEE = 0x10000  # next-event estimation: rtpt_raytrace samples the scene's emissive triangles (csrc/light_sample.hpp); not in FLAG_EXT_MASK
FLAG_EXT_NEE_SPHERE = 0x20000  # next-event estimation of the analytic sphere light: every diffuse hit samples its cone, no shadow ray (csrc/light_sample.hpp); not in FLAG_EXT_MASK
FLAG_EXT_NEE_POWER = 0x40000  # with FLAG_EXT_NEE: the emissive triangle is picked by area x emission from a cumulative table built on the device (csrc/light_table.hip); ignored alone; not in FLAG_EXT_MASK
FLAG_EXT_NEE_MIS = 0x80000  # with FLAG_EXT_NEE: the light sample and the bounce that meets the same emitter are weighed by the power heuristic (csrc/light_sample.hpp); the sphere sample is not; ignored alone; not in FLAG_EXT_MASK
FLAG_EXT_SMOOTH_GUIDE = 0x100000  # while the scene holds normals (set_normals): K0 writes interpolated guide normals and the filter's edge stop reads them per pixel (csrc/shading_normal.hpp G1-G5); ignored without normals; not in FLAG_EXT_MASK
BVH_BUILDER_HOST_SAH, BVH_BUILDER_DEVICE_LBVH = 0, 1
BUILDER_DEVICE_SAH = 2
BVH_FALLBACK_NONE, BVH_FALLBACK_DEPTH = 0, 1
DEBUG_HIT_ID, DEBUG_PREV_PIXEL = 0x1, 0x2
TEX_NEAREST = 0x1  # rtpt_texture.flags: nearest texel instead of bilinear
TEX_MIPMAP = 0x10  # sampled from a mip chain at the level of the ray's footprint; the library generates the chain
TEX_MIPS_GIVEN = 0x20  # with TEX_MIPMAP: texels holds the whole chain, level l right behind level l - 1

# rtpt_plane
(PLANE_IMAGE, PLANE_FILTERED, PLANE_PREVIOUS, PLANE_WORLDPOS, PLANE_GRADIENT, PLANE_DEPTH, PLANE_VIS_ID,
 PLANE_PREV_VIS_ID, PLANE_LUT, PLANE_LUT_PREV, PLANE_PREV_PIXEL, PLANE_RAYCOUNT, PLANE_HIT_ID, PLANE_MOMENTS,
 PLANE_VARIANCE, PLANE_MOMENTS_PREV, PLANE_ALBEDO, PLANE_SHADED) = range(18)
PLANE_COUNT = 18
# rtpt_kernel_id
(K_GBUFFER, K_LUT, K_GRADIENT, K_PATHTRACE, K_ATROUS, K_ATROUS_FINAL, K_ATROUS_CHAIN, K_ATROUS_CHAIN_FINAL,
 K_GBUFFER_GRADIENT, K_PRESENT, K_GBUFFER_PATHTRACE, K_MODULATE, K_COUNT) = range(13)
KERNEL_NAMES = ["k_gbuffer", "k_lut", "k_gradient", "k_pathtrace", "k_atrous", "k_atrous_final", "k_atrous_chain",
                "k_atrous_chain_final", "k_gbuffer_gradient", "k_present", "k_gbuffer_pathtrace", "k_modulate"]


class RtptLibraryMissing(RuntimeError):
    pass


class RtptError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rtpt error {code}: {msg}")
        self.code = code


class PushConstants(C.Structure):
    """rtpt_push_constants == PushConstants, main.cpp:35-49 (112 bytes)."""
    _fields_ = [
        ("sample_batch", C.c_uint32), ("frameNumber", C.c_uint32), ("_pad0", C.c_uint32 * 2),
        ("cameraPos", C.c_float * 3), ("_pad1", C.c_float),
        ("lightPos", C.c_float * 3), ("_pad2", C.c_float),
        ("lightPosPrev", C.c_float * 3), ("_pad3", C.c_float),
        ("currentCameraColor", C.c_float * 3), ("_pad4", C.c_float),
        ("previousCameraColor", C.c_float * 3),
        ("waveletIteration", C.c_int32), ("maxWaveletIteration", C.c_int32),
        ("_pad5", C.c_uint32 * 3),
    ]


class Ubo(C.Structure):
    """rtpt_ubo == UniformBufferObject, main.cpp:82-90 (384 bytes, column-major)."""
    _fields_ = [(n, C.c_float * 16) for n in ("model", "view", "proj", "modelPrev", "viewPrev", "projPrev")]


class Material(C.Structure):
    """rtpt_material: .mtl Kd / Ke"""
    _fields_ = [("albedo", C.c_float * 3), ("emission", C.c_float * 3)]


MAT_SPECULAR = 0x1
MAT_DIELECTRIC = 0x2
# rtpt_material_ext as a numpy record (48 bytes): Kd, Ke, Ks, roughness, flags (MAT_*), and the last word under its two names:
# `_pad` (uint32) and `ior` (float32, read when MAT_DIELECTRIC is set) overlap, as the union of rtpt.h does
MATERIAL_EXT = np.dtype({"names": ["albedo", "emission", "specular", "roughness", "flags", "_pad", "ior"],
                         "formats": [(np.float32, 3), (np.float32, 3), (np.float32, 3), np.float32, np.uint32, np.uint32, np.float32],
                         "offsets": [0, 12, 24, 36, 40, 44, 44], "itemsize": 48})
assert MATERIAL_EXT.itemsize == 48


def materials_ext(materials, specular=None, dielectric=None) -> np.ndarray:
    """MATERIAL_EXT records of (Kd, Ke) rows [m, 6] (flags 0: the set rtpt_scene_set_materials would take); specular: a dict
    material index -> (Ks, roughness) of the rows to make specular; dielectric: a dict material index -> (colour, ior) of the
    rows to make dielectric"""
    rows = np.ascontiguousarray(materials, np.float32).reshape(-1, 6)
    out = np.zeros(len(rows), MATERIAL_EXT)
    out["albedo"], out["emission"] = rows[:, :3], rows[:, 3:]
    for i, (ks, g) in (specular or {}).items():
        out["specular"][i], out["roughness"][i], out["flags"][i] = np.float32(ks), np.float32(g), MAT_SPECULAR
        out["emission"][i] = 0
    for i, (colour, ior) in (dielectric or {}).items():
        out["specular"][i], out["roughness"][i], out["flags"][i], out["ior"][i] = np.float32(colour), 0, MAT_DIELECTRIC, np.float32(ior)
        out["emission"][i] = 0
    return out


class SceneBuildInfo(C.Structure):
    """struct rtpt_scene_build_info (32 bytes)."""
    _fields_ = [
        ("builder", C.c_uint32), ("fallback", C.c_uint32), ("n_primitives", C.c_uint32), ("n_nodes", C.c_uint32),
        ("depth", C.c_uint32), ("leaf_pairs", C.c_uint32), ("build_ms", C.c_float), ("upload_ms", C.c_float),
    ]


class Config(C.Structure):
    """rtpt_config."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("row_begin", C.c_uint32), ("row_end", C.c_uint32),
        ("max_segments", C.c_uint32), ("samples_per_pixel", C.c_uint32),
        ("sigma_n", C.c_int32), ("sigma_z", C.c_float), ("sigma_l", C.c_float), ("alpha", C.c_float),
        ("light_radius", C.c_float), ("light_intensity", C.c_float), ("first_hit_light_divisor", C.c_float),
        ("fov_slope", C.c_float), ("pixel_jitter", C.c_float), ("ray_offset", C.c_float), ("ray_tmax", C.c_float),
        ("flags", C.c_uint32), ("device", C.c_int32),
    ]


assert C.sizeof(PushConstants) == 112 and C.sizeof(Ubo) == 384 and C.sizeof(SceneBuildInfo) == 32

# every symbol include/rtpt.h declares (tests check the header and this list agree)
SYMBOLS = [
    "rtpt_config_default", "rtpt_create", "rtpt_destroy", "rtpt_resize", "rtpt_last_error", "rtpt_set_stream", "rtpt_bind_plane",
    "rtpt_plane_ptr", "rtpt_plane_bytes", "rtpt_set_external_history", "rtpt_stream_wait", "rtpt_scene_upload", "rtpt_gbuffer", "rtpt_temporal_gradient",
    "rtpt_raytrace", "rtpt_temporal_filter", "rtpt_end_frame", "rtpt_sync", "rtpt_readback", "rtpt_set_plane",
    "rtpt_reset_counters", "rtpt_set_count_rows", "rtpt_enable_debug", "rtpt_timing_enable", "rtpt_timing_collect", "rtpt_kernel_name",
    "rtpt_selftest_math", "rtpt_selftest_exhaustive", "rtpt_selftest_div", "rtpt_selftest_trace", "rtpt_util_look_at", "rtpt_util_perspective", "rtpt_util_load_obj", "rtpt_util_bvh_check", "rtpt_util_bvh_check_pairs",
    "rtpt_scene_set_materials", "rtpt_util_load_obj_materials", "rtpt_util_bvh_refit_check", "rtpt_set_external_guides",
    "rtpt_present", "rtpt_debug_bvh_check", "rtpt_present_target", "rtpt_scene_build_info", "rtpt_scene_rebuild",
    "rtpt_debug_reuse_info", "rtpt_debug_bvh_topology", "rtpt_scene_set_instances", "rtpt_debug_upload_info",
    "rtpt_debug_live_device_bytes", "rtpt_modulate", "rtpt_debug_reproj_info", "rtpt_debug_defer_info",
    "rtpt_scene_set_textures", "rtpt_selftest_texture", "rtpt_util_load_obj_texcoords", "rtpt_util_load_obj_map_kd",
    "rtpt_selftest_texture_lod", "rtpt_selftest_texture_footprint", "rtpt_util_texture_chain", "rtpt_selftest_contract",
    "rtpt_scene_set_materials_ext", "rtpt_util_load_obj_materials_ext", "rtpt_selftest_bounce",
    "rtpt_util_load_obj_materials_ni", "rtpt_selftest_refract", "rtpt_debug_empty_run_info",
    "rtpt_selftest_light_sample", "rtpt_debug_light_list", "rtpt_selftest_sphere_sample",
    "rtpt_selftest_light_table", "rtpt_selftest_light_pick", "rtpt_debug_light_table",
    "rtpt_selftest_mis_weight", "rtpt_selftest_light_find",
    "rtpt_scene_set_normals", "rtpt_selftest_shading_normal", "rtpt_util_load_obj_normals",
    "rtpt_debug_guide_normals", "rtpt_debug_set_guide_normals",
    "rtpt_set_environment", "rtpt_util_environment_from_latlong", "rtpt_selftest_environment",
]

# rtpt_selftest_contract: (input words, output words) per item of every fn, in the order of the table of rtpt.h
CONTRACT_WORDS = ((6, 1), (6, 3), (3, 1), (3, 3), (2, 1), (1, 1), (2, 2), (4, 1), (1, 3), (1, 2), (1, 1), (1, 1), (19, 4), (2, 1),
                  (3, 2), (9, 1), (12, 3), (13, 3), (12, 3), (36, 2), (10, 1), (3, 3), (3, 6))

_lib = None


def load() -> C.CDLL:
    """dlopen librtpt_hip.so; fails loudly when the HIP extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtptLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the hot path.")
    lib = C.CDLL(LIB_PATH)
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    lib.rtpt_last_error.restype = C.c_char_p
    lib.rtpt_last_error.argtypes = [vp]
    lib.rtpt_kernel_name.restype = C.c_char_p
    lib.rtpt_kernel_name.argtypes = [C.c_int]
    sigs = {
        "rtpt_config_default": [C.POINTER(Config), u32, u32],
        "rtpt_create": [C.POINTER(Config), C.POINTER(vp)],
        "rtpt_destroy": [vp],
        "rtpt_resize": [vp, u32, u32, u32, u32],
        "rtpt_set_stream": [vp, vp],
        "rtpt_bind_plane": [vp, C.c_int, vp, sz],
        "rtpt_plane_ptr": [vp, C.c_int, C.POINTER(vp)],
        "rtpt_plane_bytes": [vp, C.c_int, C.POINTER(sz)],
        "rtpt_set_external_history": [vp, vp, u32, u32],
        "rtpt_stream_wait": [vp, vp],
        "rtpt_set_external_guides": [vp, vp, vp, u32, u32],
        "rtpt_scene_upload": [vp, vp, u32, vp, u32, vp, u32],
        "rtpt_gbuffer": [vp, C.POINTER(Ubo), u32, u32],
        "rtpt_temporal_gradient": [vp, C.POINTER(PushConstants), u32, u32],
        "rtpt_raytrace": [vp, C.POINTER(PushConstants), u32, u32],
        "rtpt_temporal_filter": [vp, C.POINTER(PushConstants), C.POINTER(Ubo), u32, u32],
        "rtpt_end_frame": [vp],
        "rtpt_present": [vp, vp, u32, u32],
        "rtpt_present_target": [vp, vp, u32, u32],
        "rtpt_modulate": [vp, u32, u32],
        "rtpt_sync": [vp],
        "rtpt_readback": [vp, C.c_int, vp, sz],
        "rtpt_set_plane": [vp, C.c_int, vp, sz],
        "rtpt_reset_counters": [vp],
        "rtpt_enable_debug": [vp, u32],
        "rtpt_set_count_rows": [vp, u32, u32],
        "rtpt_timing_enable": [vp, C.c_int],
        "rtpt_timing_collect": [vp, C.POINTER(C.c_double * K_COUNT), C.POINTER(u32 * K_COUNT)],
        "rtpt_selftest_math": [vp, C.c_int, vp, vp, sz],
        "rtpt_selftest_exhaustive": [vp, C.c_int, vp, vp],
        "rtpt_selftest_div": [vp, C.c_int, C.c_uint32, C.c_uint32, vp, vp],
        "rtpt_selftest_trace": [vp, vp, sz, vp, vp],
        "rtpt_selftest_contract": [vp, C.c_int, vp, vp, sz],
        "rtpt_util_load_obj": [C.c_char_p, vp, C.POINTER(u32), vp, C.POINTER(u32)],
        "rtpt_util_bvh_check": [vp, u32, C.POINTER(C.c_uint64 * 8)],
        "rtpt_util_bvh_check_pairs": [vp, u32, C.c_int, C.POINTER(C.c_uint64 * 8)],
        "rtpt_scene_set_materials": [vp, vp, u32, vp, u32],
        "rtpt_util_bvh_refit_check": [vp, vp, u32, C.POINTER(C.c_uint64 * 8)],
        "rtpt_debug_bvh_check": [vp, C.POINTER(C.c_uint64 * 8)],
        "rtpt_scene_build_info": [vp, C.POINTER(SceneBuildInfo)],
        "rtpt_scene_rebuild": [vp],
        "rtpt_debug_bvh_topology": [vp, vp, C.POINTER(u32), vp, C.POINTER(u32)],
        "rtpt_debug_reuse_info": [vp, C.POINTER(C.c_uint64 * 4)],
        "rtpt_debug_reproj_info": [vp, C.POINTER(C.c_uint64 * 4)],
        "rtpt_debug_defer_info": [vp, C.POINTER(C.c_uint64 * 4)],
        "rtpt_debug_empty_run_info": [vp, C.POINTER(C.c_uint64 * 4)],
        "rtpt_scene_set_instances": [vp, vp, u32],
        "rtpt_debug_upload_info": [vp, C.POINTER(C.c_uint64 * 4)],
        "rtpt_debug_live_device_bytes": [C.POINTER(C.c_uint64)],
        "rtpt_util_load_obj_materials": [C.c_char_p, vp, C.POINTER(u32), vp, C.POINTER(u32)],
        "rtpt_scene_set_textures": [vp, vp, vp, u32, vp, u32, vp, sz],
        "rtpt_selftest_texture": [vp, u32, vp, sz, vp],
        "rtpt_util_load_obj_texcoords": [C.c_char_p, vp, C.POINTER(u32)],
        "rtpt_util_load_obj_map_kd": [C.c_char_p, vp, C.POINTER(sz), C.POINTER(u32)],
        "rtpt_selftest_texture_lod": [vp, u32, vp, vp, sz, vp],
        "rtpt_selftest_texture_footprint": [vp, vp, sz, u32, vp, vp],
        "rtpt_util_texture_chain": [u32, u32, C.POINTER(u32), C.POINTER(C.c_uint64)],
        "rtpt_scene_set_materials_ext": [vp, vp, u32, vp, u32],
        "rtpt_util_load_obj_materials_ext": [C.c_char_p, vp, C.POINTER(u32), vp, C.POINTER(u32)],
        "rtpt_selftest_bounce": [vp, vp, vp, sz],
        "rtpt_util_load_obj_materials_ni": [C.c_char_p, vp, C.POINTER(u32), vp, C.POINTER(u32)],
        "rtpt_selftest_refract": [vp, vp, vp, sz],
        "rtpt_selftest_light_sample": [vp, vp, vp, sz],
        "rtpt_debug_light_list": [vp, vp, u32, C.POINTER(u32)],
        "rtpt_selftest_light_table": [vp, vp, sz, vp],
        "rtpt_selftest_light_pick": [vp, vp, sz, vp, sz, vp, vp],
        "rtpt_debug_light_table": [vp, vp, u32, C.POINTER(u32)],
        "rtpt_selftest_sphere_sample": [vp, vp, vp, sz],
        "rtpt_selftest_mis_weight": [vp, vp, vp, sz],
        "rtpt_selftest_light_find": [vp, vp, sz, vp, sz, vp],
        "rtpt_scene_set_normals": [vp, vp, vp, u32],
        "rtpt_selftest_shading_normal": [vp, vp, vp, sz],
        "rtpt_util_load_obj_normals": [C.c_char_p, vp, vp, C.POINTER(u32)],
        "rtpt_debug_guide_normals": [vp, vp, sz],
        "rtpt_debug_set_guide_normals": [vp, vp, sz],
        "rtpt_set_environment": [vp, vp, u32, u32, vp, vp],
        "rtpt_util_environment_from_latlong": [vp, u32, u32, u32, vp],
        "rtpt_selftest_environment": [vp, vp, sz, vp],
    }
    for name, args in sigs.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = args
    lib.rtpt_util_look_at.restype = None
    lib.rtpt_util_look_at.argtypes = [vp, vp, vp, vp]
    lib.rtpt_util_perspective.restype = None
    lib.rtpt_util_perspective.argtypes = [C.c_float, C.c_float, C.c_float, C.c_float, vp]
    _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        msg = load().rtpt_last_error(None)
        raise RtptError(rc, msg.decode() if msg else "")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def live_device_bytes() -> int:
    """device memory the library's contexts own right now (rtpt_debug_live_device_bytes)"""
    out = C.c_uint64()
    _check(load().rtpt_debug_live_device_bytes(C.byref(out)))
    return out.value


def config_default(width: int, height: int) -> Config:
    cfg = Config()
    _check(load().rtpt_config_default(C.byref(cfg), width, height))
    return cfg


def look_at(eye, center, up) -> np.ndarray:
    out = np.zeros(16, np.float32)
    e, c, u = (np.ascontiguousarray(v, np.float32) for v in (eye, center, up))
    load().rtpt_util_look_at(_ptr(e), _ptr(c), _ptr(u), _ptr(out))
    return out


def perspective(fovy, aspect, z_near, z_far) -> np.ndarray:
    out = np.zeros(16, np.float32)
    load().rtpt_util_perspective(fovy, aspect, z_near, z_far, _ptr(out))
    return out


def load_obj(path: str):
    """(xyz[n,3] f32, idx[t,3] u32) — `v`/`f` records, fan triangulation (main.cpp:416-428, D5)."""
    nv, nt = C.c_uint32(), C.c_uint32()
    _check(load().rtpt_util_load_obj(path.encode(), None, C.byref(nv), None, C.byref(nt)))
    xyz = np.zeros((nv.value, 3), np.float32)
    idx = np.zeros((nt.value, 3), np.uint32)
    _check(load().rtpt_util_load_obj(path.encode(), _ptr(xyz), C.byref(nv), _ptr(idx), C.byref(nt)))
    return xyz, idx


def _load_obj_materials(fn, path: str, new_materials):
    """count, then fill: (tri_material, new_materials(m) filled), or (None, None) when *n_materials comes back 0"""
    nt, nm = C.c_uint32(), C.c_uint32()
    _check(fn(path.encode(), None, C.byref(nt), None, C.byref(nm)))
    if nm.value == 0:
        return None, None
    tri, mats = np.zeros(nt.value, np.uint32), new_materials(nm.value)
    _check(fn(path.encode(), _ptr(tri), C.byref(nt), _ptr(mats), C.byref(nm)))
    return tri, mats


def load_obj_materials(path: str):
    """(tri_material[t] u32, materials[m, 6] f32 = Kd, Ke) of an OBJ's `mtllib`/`usemtl`; (None, None) when the OBJ names
    no readable library (the reference's Cornell box: its .mtl is missing upstream)"""
    return _load_obj_materials(load().rtpt_util_load_obj_materials, path, lambda m: np.zeros((m, 6), np.float32))


def load_obj_materials_ext(path: str):
    """load_obj_materials with Ks, Ns and illum: (tri_material[t] u32, materials[m] MATERIAL_EXT) by the rule of rtpt.h
    (specular exactly when illum >= 3, Ks != 0 and Ke == 0; roughness min(1, sqrt(2 / (Ns + 2))), 0 without Ns)"""
    return _load_obj_materials(load().rtpt_util_load_obj_materials_ext, path, lambda m: np.zeros(m, MATERIAL_EXT))


def load_obj_materials_ni(path: str):
    """load_obj_materials_ext with Ni and Tf: a material with illum 4 / 6 / 7 / 9, an `Ni` >= 1, Ke == 0 and a colour (Tf, else
    Ks) that is not 0 is a dielectric (flags MAT_DIELECTRIC, specular = colour, ior = Ni, roughness 0); every other one is
    load_obj_materials_ext's (rtpt_util_load_obj_materials_ni)"""
    return _load_obj_materials(load().rtpt_util_load_obj_materials_ni, path, lambda m: np.zeros(m, MATERIAL_EXT))


def load_obj_texcoords(path: str) -> np.ndarray:
    """tri_uv[t, 6] f32 (u0 v0 u1 v1 u2 v2), lined up with load_obj's triangles; corners without `vt` are (0, 0)"""
    nt = C.c_uint32()
    _check(load().rtpt_util_load_obj_texcoords(path.encode(), None, C.byref(nt)))
    uv = np.zeros((nt.value, 6), np.float32)
    _check(load().rtpt_util_load_obj_texcoords(path.encode(), _ptr(uv), C.byref(nt)))
    return uv


def load_obj_normals(path: str):
    """(tri_normals [t, 9] f32 — the corners' `vn` records —, tri_smooth [t] u32), lined up with load_obj's triangles; a face
    with a corner that has no usable vn gives triangles with tri_smooth 0 and normals 0 (rtpt_util_load_obj_normals)"""
    nt = C.c_uint32()
    _check(load().rtpt_util_load_obj_normals(path.encode(), None, None, C.byref(nt)))
    nrm, smooth = np.zeros((nt.value, 9), np.float32), np.zeros(nt.value, np.uint32)
    _check(load().rtpt_util_load_obj_normals(path.encode(), _ptr(nrm), _ptr(smooth), C.byref(nt)))
    return nrm, smooth


def environment_from_latlong(rgb: np.ndarray, n: int) -> np.ndarray:
    """the [n, n, 4] f32 octahedral map of the lat-long image rgb [h, w, 3] (row 0 at +y, the centre column at -z), one bilinear
    sample per texel, computed on the host in double (rtpt_util_environment_from_latlong)"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("a lat-long image is [height, width, 3]")
    out = np.zeros((max(int(n), 0), max(int(n), 0), 4), np.float32)
    _check(load().rtpt_util_environment_from_latlong(_ptr(rgb), rgb.shape[1], rgb.shape[0], int(n), _ptr(out) if out.size else None))
    return out


def load_obj_map_kd(path: str):
    """the `map_Kd` file name of every material in load_obj_materials' numbering ('' = none; entry 0 is the default
    material); None when the OBJ names no readable library"""
    nb, nm = C.c_size_t(), C.c_uint32()
    _check(load().rtpt_util_load_obj_map_kd(path.encode(), None, C.byref(nb), C.byref(nm)))
    if nm.value == 0:
        return None
    buf = C.create_string_buffer(max(nb.value, 1))
    _check(load().rtpt_util_load_obj_map_kd(path.encode(), buf, C.byref(nb), C.byref(nm)))
    return [n.decode() for n in buf.raw[:nb.value].split(b"\0")[:nm.value]]


_PLANE_DTYPE = {
    PLANE_IMAGE: (np.float32, 4), PLANE_FILTERED: (np.float32, 4), PLANE_PREVIOUS: (np.float32, 4),
    PLANE_WORLDPOS: (np.float32, 4), PLANE_GRADIENT: (np.float32, 4), PLANE_DEPTH: (np.float32, 1),
    PLANE_VIS_ID: (np.uint32, 1), PLANE_PREV_VIS_ID: (np.uint32, 1), PLANE_PREV_PIXEL: (np.int32, 2),
    PLANE_HIT_ID: (np.uint32, 1), PLANE_MOMENTS: (np.float32, 4), PLANE_VARIANCE: (np.float32, 1),
    PLANE_MOMENTS_PREV: (np.float32, 4), PLANE_ALBEDO: (np.float32, 4), PLANE_SHADED: (np.float32, 4),
}


class Context:
    """RAII wrapper of rtpt_ctx."""

    def __init__(self, cfg: Config):
        self._lib = load()
        self.cfg = cfg
        h = C.c_void_p()
        _check(self._lib.rtpt_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.n_tris = 0

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._lib.rtpt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def rows(self) -> int:
        return self.cfg.row_end - self.cfg.row_begin

    def resize(self, width: int, height: int, row_begin: int = 0, row_end: int = 0):
        _check(self._lib.rtpt_resize(self._h, width, height, row_begin, row_end))
        self.cfg.width, self.cfg.height = width, height
        self.cfg.row_begin, self.cfg.row_end = (row_begin, row_end) if (row_begin or row_end) else (0, height)

    # -- configuration
    def set_stream(self, stream_handle: int | None):
        _check(self._lib.rtpt_set_stream(self._h, C.c_void_p(stream_handle or 0)))

    def bind_plane(self, which: int, device_ptr: int | None, nbytes: int = 0):
        _check(self._lib.rtpt_bind_plane(self._h, which, C.c_void_p(device_ptr or 0), nbytes))

    def plane_ptr(self, which: int) -> int:
        p = C.c_void_p()
        _check(self._lib.rtpt_plane_ptr(self._h, which, C.byref(p)))
        return p.value or 0

    def plane_bytes(self, which: int) -> int:
        n = C.c_size_t()
        _check(self._lib.rtpt_plane_bytes(self._h, which, C.byref(n)))
        return n.value

    def set_external_history(self, device_ptr: int | None, row_begin: int = 0, row_end: int = 0):
        _check(self._lib.rtpt_set_external_history(self._h, C.c_void_p(device_ptr or 0), row_begin, row_end))

    def set_external_guides(self, prev_vis_ptr: int | None, moments_ptr: int | None, row_begin: int = 0, row_end: int = 0):
        """previous frame's id (u32) and moment (float4) rows [row_begin,row_end) gathered across strips; None, None:
        the context's own planes"""
        _check(self._lib.rtpt_set_external_guides(self._h, C.c_void_p(prev_vis_ptr or 0), C.c_void_p(moments_ptr or 0),
                                                  row_begin, row_end))

    def plane_dtype(self, which: int):
        return _PLANE_DTYPE[which]

    def stream_wait(self, other: "Context"):
        """work submitted to this context from now on starts after everything submitted to `other` so far"""
        _check(self._lib.rtpt_stream_wait(self._h, other._h))

    def enable_debug(self, mask: int):
        _check(self._lib.rtpt_enable_debug(self._h, mask))

    # -- scene
    def scene_upload(self, xyz: np.ndarray, idx: np.ndarray, instance_xforms: np.ndarray | None = None):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 3)
        ni = 0
        xf = None
        if instance_xforms is not None:
            xf = np.ascontiguousarray(instance_xforms, np.float32).reshape(-1, 12)
            ni = len(xf)
        _check(self._lib.rtpt_scene_upload(self._h, _ptr(xyz), len(xyz), _ptr(idx), len(idx), _ptr(xf), ni))
        self.n_tris = len(idx) * max(ni, 1)

    def scene_set_instances(self, instance_xforms: np.ndarray):
        """replace all instance transforms of the uploaded mesh ([n, 12] or [n, 3, 4], the upload's count): the scene is
        flattened, posed and refit again, on the device where a changed model matrix is (rtpt_scene_set_instances)"""
        xf = np.ascontiguousarray(instance_xforms, np.float32).reshape(-1, 12)
        _check(self._lib.rtpt_scene_set_instances(self._h, _ptr(xf), len(xf)))

    def debug_light_table(self) -> np.ndarray:
        """the cumulative table of FLAG_EXT_NEE_POWER as it stands on the device (rtpt_debug_light_table): uint64 [L]; empty without
        both bits, without materials or without an emitter"""
        n = C.c_uint32()
        _check(self._lib.rtpt_debug_light_table(self._h, None, 0, C.byref(n)))
        cdf = np.zeros(n.value, np.uint64)
        if n.value:
            _check(self._lib.rtpt_debug_light_table(self._h, _ptr(cdf), n.value, C.byref(n)))
        return cdf

    def debug_upload_info(self) -> dict:
        """how the last scene_upload / scene_set_instances moved the geometry (rtpt_debug_upload_info)"""
        out = (C.c_uint64 * 4)()
        _check(self._lib.rtpt_debug_upload_info(self._h, C.byref(out)))
        return dict(zip(("h2d_bytes", "device_flatten", "device_pairs", "moves_without_sync"), (int(v) for v in out)))

    def debug_light_list(self) -> np.ndarray:
        """the light list of FLAG_EXT_NEE as it stands on the device (rtpt_debug_light_list): uint32 [L], id + 1 of every posed
        emissive triangle, ascending; empty without the flag, without materials or without an emitter"""
        n = C.c_uint32()
        _check(self._lib.rtpt_debug_light_list(self._h, None, 0, C.byref(n)))
        ids = np.zeros(n.value, np.uint32)
        if n.value:
            _check(self._lib.rtpt_debug_light_list(self._h, _ptr(ids), n.value, C.byref(n)))
        return ids

    def scene_build_info(self) -> dict:
        """what built the tree that is on the device now (rtpt_scene_build_info): builder, fallback, counts, milliseconds"""
        info = SceneBuildInfo()
        _check(self._lib.rtpt_scene_build_info(self._h, C.byref(info)))
        return {name: getattr(info, name) for name, _ in SceneBuildInfo._fields_}

    def scene_rebuild(self):
        """a new tree, built on the device over the triangles as currently posed (rtpt_scene_rebuild)"""
        _check(self._lib.rtpt_scene_rebuild(self._h))

    def reuse_info(self) -> dict:
        """frame reuse as observed so far (rtpt_debug_reuse_info)"""
        out = (C.c_uint64 * 4)()
        _check(self._lib.rtpt_debug_reuse_info(self._h, C.byref(out)))
        return dict(zip(("frames_skipped", "reproj_stores", "reproj_loads", "tags_invalidated"), (int(v) for v in out)))

    def reproj_info(self) -> dict:
        """the final pass's cached reprojection as observed so far (rtpt_debug_reproj_info)"""
        out = (C.c_uint64 * 4)()
        _check(self._lib.rtpt_debug_reproj_info(self._h, C.byref(out)))
        return dict(zip(("stores", "loads", "invalidations", "plane_bytes"), (int(v) for v in out)))

    def defer_info(self) -> dict:
        """the deferred final pass as observed so far (rtpt_debug_defer_info)"""
        out = (C.c_uint64 * 4)()
        _check(self._lib.rtpt_debug_defer_info(self._h, C.byref(out)))
        return dict(zip(("recorded", "launched_in_trace", "launched_alone", "spare_bytes"), (int(v) for v in out)))

    def empty_run_info(self) -> dict:
        """the last tracing launch's tile columns that no triangle reaches, served in runs (rtpt_debug_empty_run_info)"""
        out = (C.c_uint64 * 4)()
        _check(self._lib.rtpt_debug_empty_run_info(self._h, C.byref(out)))
        return dict(zip(("full_columns", "run_workgroups", "run_tiles", "run_len"), (int(v) for v in out)))

    def set_materials(self, tri_material: np.ndarray | None, materials: np.ndarray | None):
        """per-triangle material indices + (Kd, Ke) rows; None returns to the reference's normal-keyed colours"""
        if tri_material is None or materials is None:
            _check(self._lib.rtpt_scene_set_materials(self._h, None, 0, None, 0))
            return
        tri = np.ascontiguousarray(tri_material, np.uint32)
        mats = np.ascontiguousarray(materials, np.float32).reshape(-1, 6)
        _check(self._lib.rtpt_scene_set_materials(self._h, _ptr(tri), len(tri), _ptr(mats), len(mats)))

    def set_textures(self, tri_uv=None, tri_texture=None, textures=None, texels=None):
        """albedo textures (rtpt_scene_set_textures): tri_uv [t, 6] f32, tri_texture [t] u32 (0 = untextured, i + 1 =
        textures[i]), textures [n, 4] u32 rows (width, height, first_texel, flags), texels [m, 4] f32 RGBA; None drops them"""
        if tri_uv is None or tri_texture is None or textures is None or texels is None:
            _check(self._lib.rtpt_scene_set_textures(self._h, None, None, 0, None, 0, None, 0))
            return
        uv = np.ascontiguousarray(tri_uv, np.float32).reshape(-1, 6)
        tri = np.ascontiguousarray(tri_texture, np.uint32).ravel()
        if len(uv) != len(tri):
            raise ValueError("one uv record and one texture index per triangle")
        desc = np.ascontiguousarray(textures, np.uint32).reshape(-1, 4)
        tex = np.ascontiguousarray(texels, np.float32).reshape(-1, 4)
        _check(self._lib.rtpt_scene_set_textures(self._h, _ptr(uv), _ptr(tri), len(tri), _ptr(desc), len(desc), _ptr(tex), len(tex)))

    def set_normals(self, tri_normals=None, tri_smooth=None):
        """smooth shading (rtpt_scene_set_normals): tri_normals [t, 9] f32, the corners' normals of every triangle of the
        uploaded mesh in its own space; tri_smooth [t] u32 (0: the triangle keeps its geometric normal) or None: all smooth.
        tri_normals None removes them"""
        if tri_normals is None:
            _check(self._lib.rtpt_scene_set_normals(self._h, None, None, 0))
            return
        nrm = np.ascontiguousarray(tri_normals, np.float32).reshape(-1, 9)
        sm = None if tri_smooth is None else np.ascontiguousarray(tri_smooth, np.uint32).ravel()
        if sm is not None and len(sm) != len(nrm):
            raise ValueError("one smooth word per triangle")
        _check(self._lib.rtpt_scene_set_normals(self._h, _ptr(nrm), _ptr(sm), len(nrm)))

    # -- passes
    def gbuffer(self, ubo: Ubo, y0=0, y1=0):
        _check(self._lib.rtpt_gbuffer(self._h, C.byref(ubo), y0, y1))

    def temporal_gradient(self, pc: PushConstants, y0=0, y1=0):
        _check(self._lib.rtpt_temporal_gradient(self._h, C.byref(pc), y0, y1))

    def raytrace(self, pc: PushConstants, y0=0, y1=0):
        _check(self._lib.rtpt_raytrace(self._h, C.byref(pc), y0, y1))

    def temporal_filter(self, pc: PushConstants, ubo: Ubo | None, y0=0, y1=0):
        _check(self._lib.rtpt_temporal_filter(self._h, C.byref(pc), C.byref(ubo) if ubo is not None else None, y0, y1))

    def end_frame(self):
        _check(self._lib.rtpt_end_frame(self._h))

    def present_target(self, dst_device_ptr: int | None, y0=0, y1=0):
        """name the swapchain rows of the frame being built: the final filter pass writes them too (fused blit)"""
        _check(self._lib.rtpt_present_target(self._h, C.c_void_p(dst_device_ptr) if dst_device_ptr else None, y0, y1))

    def present(self, dst_device_ptr: int, y0=0, y1=0):
        """main.cpp:1338-1361: rows [y0,y1) of the finished frame -> B8G8R8A8_UNORM at the device address"""
        _check(self._lib.rtpt_present(self._h, C.c_void_p(dst_device_ptr), y0, y1))

    def modulate(self, y0=0, y1=0):
        """FLAG_EXT_DEMODULATE: SHADED = frame x ALBEDO for rows [y0,y1) of the finished frame (rtpt_modulate)"""
        _check(self._lib.rtpt_modulate(self._h, y0, y1))

    def sync(self):
        _check(self._lib.rtpt_sync(self._h))

    def debug_bvh_topology(self):
        """(child_refs [n_nodes, 2], leaf_order [n_tris]) of the tree as it stands on the device (rtpt_debug_bvh_topology)"""
        nn, nl = C.c_uint32(0), C.c_uint32(0)
        _check(self._lib.rtpt_debug_bvh_topology(self._h, None, C.byref(nn), None, C.byref(nl)))
        refs = np.empty((nn.value, 2), np.uint32)
        leaf = np.empty(nl.value, np.uint32)
        _check(self._lib.rtpt_debug_bvh_topology(self._h, refs.ctypes.data_as(C.c_void_p), C.byref(nn), leaf.ctypes.data_as(C.c_void_p), C.byref(nl)))
        return refs, leaf

    def debug_bvh_check(self):
        """the acceleration structure as it stands on the device (after an upload or a device-side refit), checked on the host"""
        st = (C.c_uint64 * 8)()
        _check(self._lib.rtpt_debug_bvh_check(self._h, C.byref(st)))
        return dict(zip(("nodes", "leaves", "depth", "largest_leaf", "bad_refs_to_triangles", "boxes_not_containing", "boxes_beyond_scene",
                         "dangling"), (int(v) for v in st)))

    # -- data movement
    def readback(self, which: int) -> np.ndarray:
        if which in (PLANE_LUT, PLANE_LUT_PREV):
            out = np.zeros((self.n_tris + 1, 12), np.float32)
        elif which == PLANE_RAYCOUNT:
            out = np.zeros(1, np.uint64)
        else:
            dt, ch = _PLANE_DTYPE[which]
            shape = (self.rows, self.cfg.width) + ((ch,) if ch > 1 else ())
            out = np.zeros(shape, dt)
        _check(self._lib.rtpt_readback(self._h, which, _ptr(out), out.nbytes))
        return out

    def set_plane(self, which: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        _check(self._lib.rtpt_set_plane(self._h, which, _ptr(arr), arr.nbytes))

    def debug_guide_normals(self) -> np.ndarray:
        """the per-pixel normal plane of the filter's edge stop (rtpt_debug_guide_normals): float32 [rows, width, 4] = (n.xyz, self
        weight); RtptError when the context has none (a scene with an id-pair table and FLAG_EXT_SMOOTH_GUIDE not active)"""
        out = np.zeros((self.rows, self.cfg.width, 4), np.float32)
        _check(self._lib.rtpt_debug_guide_normals(self._h, _ptr(out), out.nbytes))
        return out

    def debug_set_guide_normals(self, cells: np.ndarray):
        """inject that plane ([rows, width, 4] float32; rtpt_debug_set_guide_normals): it counts as written by K0 for every stored
        row of the current frame, until the next K0"""
        cells = np.ascontiguousarray(cells, np.float32)
        _check(self._lib.rtpt_debug_set_guide_normals(self._h, _ptr(cells), cells.nbytes))

    def reset_counters(self):
        _check(self._lib.rtpt_reset_counters(self._h))

    def set_count_rows(self, y0: int, y1: int):
        _check(self._lib.rtpt_set_count_rows(self._h, y0, y1))

    def raycount(self) -> int:
        return int(self.readback(PLANE_RAYCOUNT)[0])

    # -- timing
    def timing_enable(self, period):
        """0/False off; n: bracket the kernels of every n-th frame with HIP events (True == 1)."""
        _check(self._lib.rtpt_timing_enable(self._h, int(period)))

    def timing_collect(self):
        ms = (C.c_double * K_COUNT)()
        n = (C.c_uint32 * K_COUNT)()
        _check(self._lib.rtpt_timing_collect(self._h, C.byref(ms), C.byref(n)))
        return {KERNEL_NAMES[i]: (ms[i], n[i]) for i in range(K_COUNT)}

    # -- self tests
    def selftest_math(self, op: int, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        _check(self._lib.rtpt_selftest_math(self._h, op, _ptr(x), _ptr(out), x.size))
        return out

    def selftest_exhaustive(self, op: int):
        """(mismatches, first offending patterns) of exact sqrt (op 3) / reciprocal (op 4) over all 2^32 binary32 patterns"""
        n = C.c_uint64(0)
        first = np.zeros(4, np.uint32)
        _check(self._lib.rtpt_selftest_exhaustive(self._h, op, C.byref(n), _ptr(first)))
        return int(n.value), first

    def selftest_div(self, mode: int, first_pass: int, n_passes: int):
        """(mismatches, bits of one offending (a, b)) of exact::div_ against the compiler's division; see rtpt.h"""
        n = C.c_uint64(0)
        first = np.zeros(2, np.uint32)
        _check(self._lib.rtpt_selftest_div(self._h, mode, first_pass, n_passes, C.byref(n), _ptr(first)))
        return int(n.value), first

    def selftest_contract(self, fn: int, words: np.ndarray) -> np.ndarray:
        """words [n, n_in] uint32 -> [n, n_out] uint32: contract function fn on the device, one thread per item; the table of
        fn and its words per item is in rtpt.h (rtpt_selftest_contract)"""
        n_in, n_out = CONTRACT_WORDS[fn]
        words = np.ascontiguousarray(words, np.uint32)
        if words.ndim != 2 or words.shape[1] != n_in:
            raise ValueError(f"contract function {fn} takes {n_in} words per item, got an array of shape {words.shape}")
        out = np.zeros((len(words), n_out), np.uint32)
        _check(self._lib.rtpt_selftest_contract(self._h, fn, _ptr(words), _ptr(out), len(words)))
        return out

    def set_materials_ext(self, tri_material: np.ndarray | None, materials: np.ndarray | None):
        """per-triangle material indices + MATERIAL_EXT records (diffuse or specular); None drops the set"""
        if tri_material is None or materials is None:
            _check(self._lib.rtpt_scene_set_materials_ext(self._h, None, 0, None, 0))
            return
        tri = np.ascontiguousarray(tri_material, np.uint32)
        mats = np.ascontiguousarray(materials, MATERIAL_EXT)
        _check(self._lib.rtpt_scene_set_materials_ext(self._h, _ptr(tri), len(tri), _ptr(mats), len(mats)))

    def selftest_bounce(self, cases: np.ndarray) -> np.ndarray:
        """[n, 4] (d', absorbed) of the device's specular bounce on cases [n, 9] = d, n, u1, u2, g (rtpt_selftest_bounce)"""
        cases = np.ascontiguousarray(cases, np.float32).reshape(-1, 9)
        out = np.zeros((len(cases), 4), np.float32)
        _check(self._lib.rtpt_selftest_bounce(self._h, _ptr(cases), _ptr(out), len(cases)))
        return out

    def selftest_refract(self, cases: np.ndarray) -> np.ndarray:
        """[n, 5] (d', transmitted, F) of the device's dielectric interface on cases [n, 9] = d, n, u1, u2, ior (rtpt_selftest_refract)"""
        cases = np.ascontiguousarray(cases, np.float32).reshape(-1, 9)
        out = np.zeros((len(cases), 5), np.float32)
        _check(self._lib.rtpt_selftest_refract(self._h, _ptr(cases), _ptr(out), len(cases)))
        return out

    def selftest_light_sample(self, cases: np.ndarray) -> np.ndarray:
        """[n, 9] uint32 words (y, wd, g, valid as floats, the picked entry) of the device's light sample on cases [n, 19] words =
        v0, v1, v2, x, nf, u_l, u_a, u_b as floats, L as uint32 (rtpt_selftest_light_sample)"""
        cases = np.ascontiguousarray(cases, np.uint32).reshape(-1, 19)
        out = np.zeros((len(cases), 9), np.uint32)
        _check(self._lib.rtpt_selftest_light_sample(self._h, _ptr(cases), _ptr(out), len(cases)))
        return out

    def selftest_light_table(self, w: np.ndarray) -> np.ndarray:
        """uint64 [n]: the cumulative table of FLAG_EXT_NEE_POWER the device builds from the weights w [n] float32
        (rtpt_selftest_light_table; needs neither a scene nor the flag)"""
        w = np.ascontiguousarray(w, np.float32).ravel()
        out = np.zeros(len(w), np.uint64)
        _check(self._lib.rtpt_selftest_light_table(self._h, _ptr(w), len(w), _ptr(out)))
        return out

    def selftest_light_pick(self, cdf: np.ndarray, u_l: np.ndarray):
        """(entry uint32 [k], inv_p float32 [k]) of the device's weighted pick of draws u_l [k] on the table cdf [n] uint64
        (rtpt_selftest_light_pick)"""
        cdf = np.ascontiguousarray(cdf, np.uint64).ravel()
        u_l = np.ascontiguousarray(u_l, np.float32).ravel()
        idx = np.zeros(len(u_l), np.uint32)
        inv_p = np.zeros(len(u_l), np.float32)
        _check(self._lib.rtpt_selftest_light_pick(self._h, _ptr(cdf), len(cdf), _ptr(u_l), len(u_l), _ptr(idx), _ptr(inv_p)))
        return idx, inv_p

    def selftest_mis_weight(self, cases: np.ndarray) -> np.ndarray:
        """[n, 3] float32 (g_hit, wb(g_hit), g_hit * m(g_hit)) of the device's weights of FLAG_EXT_NEE_MIS on cases [n, 20] floats =
        v0, v1, v2 of the hit emitter, o, d, b1, b2, cb, inv_p, one word that is not read (rtpt_selftest_mis_weight)"""
        cases = np.ascontiguousarray(cases, np.float32).reshape(-1, 20)
        out = np.zeros((len(cases), 3), np.float32)
        _check(self._lib.rtpt_selftest_mis_weight(self._h, _ptr(cases), _ptr(out), len(cases)))
        return out

    def set_environment(self, texels=None, flags: int = 0, rotation=None, scale=None):
        """the environment map (rtpt_set_environment): texels [n, n, 4] f32 of an octahedral map, flags TEX_NEAREST or 0, rotation
        [3, 3] row-major (None: the identity), scale [3] (None: 1, 1, 1); texels None drops it.  Of the context, not of the scene"""
        if texels is None:
            _check(self._lib.rtpt_set_environment(self._h, None, 0, 0, None, None))
            return
        tx = np.ascontiguousarray(texels, np.float32)
        if tx.ndim != 3 or tx.shape[0] != tx.shape[1] or tx.shape[2] != 4:
            raise ValueError("an environment map is [n, n, 4]")
        rot = None if rotation is None else np.ascontiguousarray(rotation, np.float32).reshape(9)
        sc = None if scale is None else np.ascontiguousarray(scale, np.float32).reshape(3)
        _check(self._lib.rtpt_set_environment(self._h, _ptr(tx), tx.shape[0], int(flags), None if rot is None else _ptr(rot),
                                              None if sc is None else _ptr(sc)))

    def selftest_environment(self, dirs: np.ndarray) -> np.ndarray:
        """[n, 3] f32: the device lookup of the context's environment map at directions [n, 3] (rtpt_selftest_environment)"""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros((len(dirs), 3), np.float32)
        _check(self._lib.rtpt_selftest_environment(self._h, _ptr(dirs), len(dirs), _ptr(out)))
        return out

    def selftest_shading_normal(self, cases: np.ndarray) -> np.ndarray:
        """[n, 8] float32 (smooth, ns[3], absorbed, sample_side, the dielectric's offset, 0) of the device's smooth-shading rules
        on cases [n, 36] floats = n0, n1, n2, b1, b2, the cofactor rows [9], ng, d, d', wd, ray_offset, three words that are
        not read (rtpt_selftest_shading_normal)"""
        cases = np.ascontiguousarray(cases, np.float32).reshape(-1, 36)
        out = np.zeros((len(cases), 8), np.float32)
        _check(self._lib.rtpt_selftest_shading_normal(self._h, _ptr(cases), _ptr(out), len(cases)))
        return out

    def selftest_light_find(self, ids: np.ndarray, queries: np.ndarray) -> np.ndarray:
        """uint32 [k]: the index of every query in the ascending list ids [n] uint32, n for an id that is not in it
        (rtpt_selftest_light_find: the search of FLAG_EXT_NEE_MIS)"""
        ids = np.ascontiguousarray(ids, np.uint32).ravel()
        queries = np.ascontiguousarray(queries, np.uint32).ravel()
        out = np.zeros(len(queries), np.uint32)
        _check(self._lib.rtpt_selftest_light_find(self._h, _ptr(ids) if len(ids) else None, len(ids), _ptr(queries), len(queries), _ptr(out)))
        return out

    def selftest_sphere_sample(self, cases: np.ndarray) -> np.ndarray:
        """[n, 6] uint32 words (wd, g, taken, valid as floats; wd and g 0 where not taken) of the device's sphere sample on cases
        [n, 12] words = x, nf, c, r2, u_c, u_p as floats (rtpt_selftest_sphere_sample)"""
        cases = np.ascontiguousarray(cases, np.uint32).reshape(-1, 12)
        out = np.zeros((len(cases), 6), np.uint32)
        _check(self._lib.rtpt_selftest_sphere_sample(self._h, _ptr(cases), _ptr(out), len(cases)))
        return out

    def selftest_texture(self, texture: int, uv: np.ndarray) -> np.ndarray:
        """[n, 4] RGBA the device sampler reads from textures[texture] at uv [n, 2] (rtpt_selftest_texture)"""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        out = np.zeros((len(uv), 4), np.float32)
        _check(self._lib.rtpt_selftest_texture(self._h, texture, _ptr(uv), len(uv), _ptr(out)))
        return out

    def selftest_texture_lod(self, texture: int, uv: np.ndarray, lod: np.ndarray) -> np.ndarray:
        """[n, 4] RGBA the device sampler reads from textures[texture] at uv [n, 2] and level lod [n] (rtpt_selftest_texture_lod)"""
        uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        lod = np.ascontiguousarray(np.broadcast_to(np.asarray(lod, np.float32), (len(uv),)))
        out = np.zeros((len(uv), 4), np.float32)
        _check(self._lib.rtpt_selftest_texture_lod(self._h, texture, _ptr(uv), _ptr(lod), len(uv), _ptr(out)))
        return out

    def selftest_texture_footprint(self, rays: np.ndarray, bounce: int):
        """(hit id + 1, the level shade_segment would sample the hit's texture at) of rays [n, 6]; bounce 0: the rule of
        segment 0, 1: of every later segment (rtpt_selftest_texture_footprint)"""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        ids = np.zeros(len(rays), np.uint32)
        lod = np.zeros(len(rays), np.float32)
        _check(self._lib.rtpt_selftest_texture_footprint(self._h, _ptr(rays), len(rays), bounce, _ptr(ids), _ptr(lod)))
        return ids, lod

    def selftest_trace(self, rays: np.ndarray):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        ids = np.zeros(len(rays), np.uint32)
        ts = np.zeros(len(rays), np.float32)
        _check(self._lib.rtpt_selftest_trace(self._h, _ptr(rays), len(rays), _ptr(ids), _ptr(ts)))
        return ids, ts


def texture_chain(width: int, height: int):
    """(levels, texels) of the mip chain of a width x height texture (rtpt_util_texture_chain; needs no GPU)"""
    n, t = C.c_uint32(0), C.c_uint64(0)
    _check(load().rtpt_util_texture_chain(width, height, C.byref(n), C.byref(t)))
    return int(n.value), int(t.value)


def bvh_check(tris: np.ndarray, built_for: np.ndarray | None = None, pairs: bool = False) -> dict:
    """host-only self check of the BVH builder + device node packing (needs no GPU): see rtpt_util_bvh_check;
    with `built_for` the tree is built over those triangles and REFIT to `tris` (rtpt_util_bvh_refit_check); with `pairs`
    it is built over the fan pairs (2q, 2q + 1) and every leaf must be one of them (rtpt_util_bvh_check_pairs)"""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 9)
    st = (C.c_uint64 * 8)()
    if built_for is not None:
        built_for = np.ascontiguousarray(built_for, np.float32).reshape(-1, 9)
        assert built_for.shape == tris.shape
        _check(load().rtpt_util_bvh_refit_check(_ptr(built_for), _ptr(tris), len(tris), C.byref(st)))
    elif pairs:
        _check(load().rtpt_util_bvh_check_pairs(_ptr(tris), len(tris), 1, C.byref(st)))
    else:
        _check(load().rtpt_util_bvh_check(_ptr(tris), len(tris), C.byref(st)))
    keys = ("nodes", "leaves", "max_depth", "largest_leaf", "bad_triangle_refs", "loose_boxes", "loose_device_boxes", "bad_child_refs")
    return dict(zip(keys, (int(v) for v in st)))
