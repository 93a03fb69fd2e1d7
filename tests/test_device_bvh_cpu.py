"""The ABI of the device-side BVH build (include/rtpt.h, ABI version 5) as far as it can be checked without a GPU:
the header's constants against the Python binding, and the layout of `struct rtpt_scene_build_info` as a C compiler
lays it out against the ctypes structure."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rtpt.h")

FIELDS = ("builder", "fallback", "n_primitives", "n_nodes", "depth", "leaf_pairs", "build_ms", "upload_ms")


def _header():
    return open(HEADER).read()


def test_abi_version_flag_and_enums_match_the_header(hip_lib):
    text = _header()
    assert re.search(r"#define\s+RTPT_ABI_VERSION\s+5\b", text)
    m = re.search(r"#define\s+RTPT_FLAG_DEVICE_BVH_BUILD\s+(0x[0-9a-fA-F]+)u", text)
    assert m and int(m.group(1), 16) == 0x1000 == hip_lib.FLAG_DEVICE_BVH_BUILD
    # the flag is a bit of its own
    others = [int(v, 16) for n, v in re.findall(r"#define\s+(RTPT_FLAG_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+)u", text)
              if n != "RTPT_FLAG_DEVICE_BVH_BUILD"]
    assert len(others) >= 12 and not any(o & 0x1000 for o in others)
    assert not hip_lib.FLAG_EXT_MASK & hip_lib.FLAG_DEVICE_BVH_BUILD
    enums = dict(re.findall(r"\b(RTPT_BVH_[A-Z_]+)\s*=\s*(\d+)", text))
    assert enums == {"RTPT_BVH_BUILDER_HOST_SAH": "0", "RTPT_BVH_BUILDER_DEVICE_LBVH": "1",
                     "RTPT_BVH_FALLBACK_NONE": "0", "RTPT_BVH_FALLBACK_DEPTH": "1"}
    assert (hip_lib.BVH_BUILDER_HOST_SAH, hip_lib.BVH_BUILDER_DEVICE_LBVH) == (0, 1)
    assert (hip_lib.BVH_FALLBACK_NONE, hip_lib.BVH_FALLBACK_DEPTH) == (0, 1)
    for sym in ("rtpt_scene_build_info", "rtpt_scene_rebuild"):
        assert sym in hip_lib.SYMBOLS and hasattr(hip_lib.load(), sym)


def test_build_info_layout_matches_a_c_compiler(hip_lib, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtpt.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(struct rtpt_scene_build_info));\n' +
                   "".join(f'  printf(" %zu", offsetof(struct rtpt_scene_build_info, {f}));\n' for f in FIELDS) +
                   "  return RTPT_ABI_VERSION == 5 ? 0 : 1;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    S = hip_lib.SceneBuildInfo
    assert out[0] == 32 == C.sizeof(S)
    assert tuple(n for n, _ in S._fields_) == FIELDS
    assert out[1:] == [getattr(S, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24, 28]
    for f in FIELDS[:6]:
        assert dict(S._fields_)[f] is C.c_uint32
    for f in FIELDS[6:]:
        assert dict(S._fields_)[f] is C.c_float


def test_entry_points_refuse_a_null_context(hip_lib):
    lib = hip_lib.load()
    info = hip_lib.SceneBuildInfo()
    assert lib.rtpt_scene_build_info(None, C.byref(info)) == hip_lib.RTPT_E_INVALID
    assert lib.rtpt_scene_rebuild(None) == hip_lib.RTPT_E_INVALID
