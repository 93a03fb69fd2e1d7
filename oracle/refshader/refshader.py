"""ORACLE — TEST INFRASTRUCTURE ONLY.

ctypes front end of oracle/_ref/librefshader.so: the reference's three compute shaders, executed on the CPU as written
(prep.py + glsl_compat.hpp + host.cpp), in two arithmetics: "f32" (binary32, unfused, contract builtins) and "f64"
(double, libm).  Plane layouts are those of oracle/oracle.py's wrappers; f64 planes are float64 arrays.

available() is False when the library has not been built (no reference tree on this machine and none shipped).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "_ref", "librefshader.so")
_libs: dict = {}
NO_LOAD = np.int32(-2 ** 31)  # prev_pixel where the invocation did no previousFrameImage load


def available(path: str | None = None) -> bool:
    return os.path.exists(path or LIB_PATH)


def lib(path: str | None = None) -> C.CDLL:
    path = path or LIB_PATH
    if path not in _libs:
        from oracle import oracle as O
        L = C.CDLL(path)
        # R32's ray query is served by the oracle's exported closest hit (the contract's ray-triangle routine, D4)
        fn = C.cast(O.lib().oracle_closest_hit, C.c_void_p)
        L.ref_set_closest_hit_f32(fn)
        L.ref_set_closest_hit_f64(fn)
        L.ref_raytrace_f32.restype = C.c_uint64
        L.ref_raytrace_f64.restype = C.c_uint64
        _libs[path] = L
    return _libs[path]


def _dt(arith):
    return {"f32": np.float32, "f64": np.float64}[arith]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _real(a, arith):
    return None if a is None else np.ascontiguousarray(a, _dt(arith))


def rng_floats(arith, state: int, n: int, path=None):
    s = C.c_uint32(state)
    out = np.zeros(n, _dt(arith))
    getattr(lib(path), "ref_rng_floats_" + arith)(C.byref(s), C.c_int(n), _p(out))
    return out, int(s.value)


def random_gaussian(arith, state: int, path=None):
    s = C.c_uint32(state)
    out = np.zeros(2, _dt(arith))
    getattr(lib(path), "ref_random_gaussian_" + arith)(C.byref(s), _p(out))
    return out, int(s.value)


def raytrace(arith, W, H, pc, tris, max_segments=32, num_samples=1, path=None, want_rays=False):
    """-> dict(image[H,W,4], rays, seq_id[H,W,max_rec] uint16 (id+1, 0 = none), seq_t, seq_n[H,W], dir0[H,W,3])"""
    max_rec = max_segments * num_samples
    tris = np.ascontiguousarray(tris, np.float32)
    img = np.zeros((H, W, 4), _dt(arith))
    seq_id = np.zeros((H, W, max_rec), np.uint16)
    seq_t = np.zeros((H, W, max_rec), _dt(arith))
    seq_n = np.zeros((H, W), np.int32)
    dir0 = np.zeros((H, W, 3), _dt(arith))
    seq_od = np.zeros((H, W, max_rec, 6), _dt(arith)) if want_rays else None  # origin, direction of every query
    rays = getattr(lib(path), "ref_raytrace_" + arith)(
        C.c_uint32(W), C.c_uint32(H), C.byref(pc), _p(tris), C.c_uint32(len(tris)), C.c_int(max_segments),
        C.c_int(num_samples), _p(img), _p(seq_id), _p(seq_t), _p(seq_n), C.c_int(max_rec), _p(dir0), _p(seq_od))
    return dict(image=img, rays=int(rays), seq_id=seq_id, seq_t=seq_t, seq_n=seq_n, dir0=dir0, seq_od=seq_od)


def temporal_gradient(arith, W, H, pc, vis, worldpos, lut, lut_prev, path=None):
    grad = np.full((H, W, 4), 7.0, _dt(arith))  # sentinel: the shader's store-before-check has to clear it
    vis = np.ascontiguousarray(vis, np.uint32)
    lut = np.ascontiguousarray(lut, np.float32)
    lut_prev = np.ascontiguousarray(lut_prev, np.float32)
    getattr(lib(path), "ref_temporal_gradient_" + arith)(
        C.c_uint32(W), C.c_uint32(H), C.byref(pc), _p(vis), _p(_real(worldpos, arith)), _p(lut), _p(lut_prev),
        C.c_uint32(len(lut)), _p(grad))
    return grad


def temporal_filter(arith, W, H, pc, ubo, img_in, depth, vis, lut, lut_prev, worldpos, history, serial_in_place=False,
                    path=None):
    """one iteration -> (filtered[H,W,4], blend[H,W,4] (NaN where colorImage was not stored), prev_pixel[H,W,2] (NO_LOAD
    where previousFrameImage was not loaded))"""
    filtered = np.zeros((H, W, 4), _dt(arith))
    blend = np.full((H, W, 4), np.nan, _dt(arith))
    pp = np.full((H, W, 2), NO_LOAD, np.int32)
    vis = np.ascontiguousarray(vis, np.uint32)
    lut = np.ascontiguousarray(lut, np.float32)
    lut_prev = np.ascontiguousarray(lut_prev, np.float32)
    if history is None:
        history = np.zeros((H, W, 4), _dt(arith))
    a, d, wp, hs = (_real(x, arith) for x in (img_in, depth, worldpos, history))
    getattr(lib(path), "ref_temporal_filter_" + arith)(
        C.c_uint32(W), C.c_uint32(H), C.byref(pc), C.byref(ubo), _p(a), _p(d), _p(vis), _p(lut), _p(lut_prev),
        C.c_uint32(len(lut)), _p(wp), _p(hs), _p(filtered), _p(blend), _p(pp), C.c_int(1 if serial_in_place else 0))
    return filtered, blend, pp


class RefApp:
    """Four-stage frame driver on the shader host: K1, K2, K3 x N from the reference's text; K0 (rasterisation) and the
    end-of-frame role rotation from the oracle's host mirror (oracle.OracleApp), which also poses camera and light."""

    def __init__(self, arith, oracle_app=None, path=None):
        self.arith, self.path = arith, path
        self.tris = None if oracle_app is None else oracle_app.tris  # world-space triangles of the current frame
        self.history = None
        self.lut_prev = None

    def draw(self, fo, pc, ubo, max_segments, iterations):
        """fo: the oracle's FrameOut of the same frame (K0 planes are taken from it); pc / ubo as the oracle posed them"""
        from oracle import oracle as O
        A, (H, W) = self.arith, fo.vis.shape
        lut_prev = fo.lut if self.lut_prev is None else self.lut_prev
        grad = temporal_gradient(A, W, H, pc, fo.vis, fo.worldpos, fo.lut, lut_prev, self.path)
        pcs = O.PushConstants.from_buffer_copy(bytes(pc))
        tr = raytrace(A, W, H, pcs, self.tris, max_segments, 1, self.path)
        cur, per_it, pp = tr["image"], [], None
        pcs.maxWaveletIteration = iterations
        for k in range(1, iterations + 1):
            pcs.waveletIteration = k
            filtered, blend, ppk = temporal_filter(A, W, H, pcs, ubo, cur, fo.depth, fo.vis, fo.lut, lut_prev,
                                                   fo.worldpos, self.history, path=self.path)
            # main.cpp:1264-1281 (the oracle's host mirror): only an odd final pass blends into the image that is read
            cur = blend if (k == iterations and k & 1) else filtered
            if k == iterations:
                pp = ppk
            per_it.append(cur)
        self.history, self.lut_prev = cur, fo.lut
        return dict(gradient=grad, traced=tr, per_iteration=per_it, image=cur, prev_pixel=pp)
