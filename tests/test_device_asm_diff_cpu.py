"""scripts/device_asm_diff.py --pair-renamed on two tiny source trees: a kernel whose mangled name changed pairs with its
parent by text and qualified function name, and by nothing weaker.  Compiles for gfx950 with hipcc; needs no GPU."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "scripts", "device_asm_diff.py")
HIPCC = shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) or shutil.which("hipcc")

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")

MAKEFILE = """HIPCC ?= {hipcc}
ARCH ?= gfx950
CXXFLAGS = -O3 -std=c++17 --offload-arch=$(ARCH)
"""

# two template kernels; k_shift never changes
PARENT = """#include <hip/hip_runtime.h>
template <int N> __global__ void k_scale(float* p, float s) { p[threadIdx.x] *= s + N; }
template <int N> __global__ void k_shift(float* p, float s) { p[threadIdx.x] += s * N; }
template __global__ void k_scale<1>(float*, float);
template __global__ void k_shift<2>(float*, float);
"""
# k_scale's signature gains a parameter pack that is empty: another mangled name, the same function type and text
PACK = PARENT.replace("template <int N> __global__ void k_scale(float* p, float s)", "template <int N, class... P> __global__ void k_scale(float* p, float s, P... rest)")
# ... and one statement changes besides
PACK_CHANGED = PACK.replace("p[threadIdx.x] *= s + N;", "p[threadIdx.x] *= s - N;")
# the parent's text under another function name
OTHER_NAME = PARENT.replace("k_scale", "k_grows")


def run(tmp_path, tag, new_source, *options):
    dirs = []
    for side, source in (("parent", PARENT), (tag, new_source)):
        d = tmp_path / side
        d.mkdir(exist_ok=True)
        (d / "Makefile").write_text(MAKEFILE.format(hipcc=HIPCC))
        (d / "k.hip").write_text(source)
        dirs.append(str(d))
    r = subprocess.run([sys.executable, TOOL, *dirs, "-j", "2", *options], capture_output=True, text=True)
    assert r.returncode in (0, 1), r.stderr
    return r.returncode, r.stdout


def test_sources_differ_as_intended():
    assert PACK != PARENT and PACK_CHANGED != PACK and OTHER_NAME != PARENT


@pytest.mark.parametrize("mode", [(), ("--by-kernel",)], ids=["per-file", "by-kernel"])
def test_empty_pack_pairs_and_is_equal(tmp_path, mode):
    rc, out = run(tmp_path, "pack", PACK, "--pair-renamed", *mode)
    assert rc == 0, out
    assert "kernels compared 2, equal 2, renamed 1, paired 1; metadata entries 2, equal 2, renamed 1, paired 1" in out
    assert "only in" not in out and out.endswith("all equal\n")


def test_renamed_and_changed_is_a_difference(tmp_path):
    rc, out = run(tmp_path, "changed", PACK_CHANGED, "--pair-renamed")
    assert rc == 1, out
    assert "kernels compared 3, equal 1, renamed 1, paired 0" in out
    assert "kernel only in the parent: _Z7k_scaleILi1EEvPff" in out and "kernel only in the new code: _Z7k_scaleILi1EJEEvPff" in out
    assert out.endswith("DIFFERENCES\n")


def test_without_the_option_a_rename_is_only_in(tmp_path):
    rc, out = run(tmp_path, "pack", PACK)
    assert rc == 1, out
    assert "kernels compared 3, equal 1; metadata entries 3, equal 1" in out and "renamed" not in out
    for what in ("kernel", "metadata entry"):
        assert f"{what} only in the parent: _Z7k_scaleILi1EEvPff" in out and f"{what} only in the new code: _Z7k_scaleILi1EJEEvPff" in out
    assert out.endswith("DIFFERENCES\n")


def test_another_function_name_does_not_pair(tmp_path):
    rc, out = run(tmp_path, "other", OTHER_NAME, "--pair-renamed")
    assert rc == 1, out
    assert "kernels compared 3, equal 1, renamed 1, paired 0" in out
    assert "kernel only in the parent: _Z7k_scaleILi1EEvPff" in out and "kernel only in the new code: _Z7k_growsILi1EEvPff" in out
    assert out.endswith("DIFFERENCES\n")
