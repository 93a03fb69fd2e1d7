"""Everything the six OBJ entry points of the C ABI return for one file, as a flat dict of numpy arrays: what
tests/golden/make_obj_reader.py records from the parent commit's library and tests/test_obj_reader_cpu.py compares the
library under test with.  The calls go through abi's ctypes signatures but not through its wrappers, which raise on an
error and so lose the counts and arrays an entry point still writes."""
import ctypes as C
import glob
import os

import numpy as np

CORPUS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj_reader")
EXPECTED = os.path.join(CORPUS, "expected.npz")
FILL = 0xA5  # arrays are handed over filled with this byte: what a call leaves unwritten shows


def corpus_files():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(CORPUS, "*.obj")))


def _buf(n, dtype):
    a = np.empty(n, dtype)
    a.view(np.uint8)[...] = FILL
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _status(abi, rc):
    msg = abi.load().rtpt_last_error(None) if rc else b""
    return np.int32(rc), np.str_((msg or b"").decode())


def call_all(abi, path):
    """{"<entry point>/<what>": array}: for every entry point the count call (rc0, err0, counts), the filling call with
    arrays of exactly those counts (rc, err, counts, arrays), and, where there is a capacity to fall short of, the call with
    one element less (rc_small, err_small)"""
    lib, p, out = abi.load(), path.encode(), {}

    def put(entry, **kw):
        for k, v in kw.items():
            out[f"{entry}/{k}"] = np.asarray(v)

    # rtpt_util_load_obj
    nv, nt = C.c_uint32(0), C.c_uint32(0)
    rc0, err0 = _status(abi, lib.rtpt_util_load_obj(p, None, C.byref(nv), None, C.byref(nt)))
    xyz, idx = _buf(3 * nv.value, np.float32), _buf(3 * nt.value, np.uint32)
    put("load_obj", rc0=rc0, err0=err0, n_verts0=nv.value, n_tris0=nt.value)
    rc, err = _status(abi, lib.rtpt_util_load_obj(p, _ptr(xyz), C.byref(nv), _ptr(idx), C.byref(nt)))
    put("load_obj", rc=rc, err=err, n_verts=nv.value, n_tris=nt.value, xyz=xyz, idx=idx)

    # rtpt_util_load_obj_materials, _ext, _ni
    for entry, dtype in (("load_obj_materials", np.dtype((np.float32, 6))), ("load_obj_materials_ext", abi.MATERIAL_EXT),
                         ("load_obj_materials_ni", abi.MATERIAL_EXT)):
        fn = getattr(lib, "rtpt_util_" + entry)
        nt, nm = C.c_uint32(0), C.c_uint32(0)
        rc0, err0 = _status(abi, fn(p, None, C.byref(nt), None, C.byref(nm)))
        put(entry, rc0=rc0, err0=err0, n_tris0=nt.value, n_materials0=nm.value)
        tri, mats = _buf(nt.value, np.uint32), _buf(nm.value, dtype)
        rc, err = _status(abi, fn(p, _ptr(tri), C.byref(nt), _ptr(mats), C.byref(nm)))
        put(entry, rc=rc, err=err, n_tris=nt.value, n_materials=nm.value, tri_material=tri, materials=mats.view(np.uint8))
        if nm.value:
            small = C.c_uint32(nm.value - 1)
            rc, err = _status(abi, fn(p, _ptr(tri), C.byref(nt), _ptr(mats), C.byref(small)))
            put(entry, rc_small=rc, err_small=err, n_materials_small=small.value)

    # rtpt_util_load_obj_texcoords
    nt = C.c_uint32(0)
    rc0, err0 = _status(abi, lib.rtpt_util_load_obj_texcoords(p, None, C.byref(nt)))
    put("load_obj_texcoords", rc0=rc0, err0=err0, n_tris0=nt.value)
    uv = _buf(6 * nt.value, np.float32)
    rc, err = _status(abi, lib.rtpt_util_load_obj_texcoords(p, _ptr(uv), C.byref(nt)))
    put("load_obj_texcoords", rc=rc, err=err, n_tris=nt.value, tri_uv=uv)

    # rtpt_util_load_obj_map_kd
    nb, nm = C.c_size_t(0), C.c_uint32(0)
    rc0, err0 = _status(abi, lib.rtpt_util_load_obj_map_kd(p, None, C.byref(nb), C.byref(nm)))
    put("load_obj_map_kd", rc0=rc0, err0=err0, names_bytes0=nb.value, n_materials0=nm.value)
    names = _buf(nb.value, np.uint8)
    rc, err = _status(abi, lib.rtpt_util_load_obj_map_kd(p, _ptr(names), C.byref(nb), C.byref(nm)))
    put("load_obj_map_kd", rc=rc, err=err, names_bytes=nb.value, n_materials=nm.value, names=names)
    if nb.value:
        small = C.c_size_t(nb.value - 1)
        rc, err = _status(abi, lib.rtpt_util_load_obj_map_kd(p, _ptr(names), C.byref(small), C.byref(nm)))
        put("load_obj_map_kd", rc_small=rc, err_small=err, names_bytes_small=small.value)
    return out
