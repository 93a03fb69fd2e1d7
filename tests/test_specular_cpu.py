"""The specular bounce without a GPU: the numpy float32 restatement (tests/specular_scenes.py) against a float64 reflection on
hostile and seeded operands, the loader's Ks / Ns / illum rule on a written library, the old loader on the same file, and the
host-only checks under the sanitizers (csrc/tests/material_host_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import specular_scenes as S
from conftest import ROOT, bits

F32 = np.float32
CSRC = os.path.join(ROOT, "real_time_path_tracing_with_spatiotemporal_filtering_amd", "csrc")
BAR = 2.0 ** -20


@pytest.mark.parametrize("cases", ["hostile", "seeded"])
def test_restatement_against_a_float64_reflection(oracle, cases):
    """|d'| = 1, d' is the float64 direction, the absorbed flag is float64's.

    The bar for a component of d' is 2^-20 where v = r + g s, the vector that is normalized, is at least a unit long — every
    case with g = 0 or 2^-24, where |v| = 1 up to rounding: the chain is a dozen binary32 roundings on values below 2 (three in
    n . d, the doubling, one fma per component of r; sincos2pi, the square root and a product per component of s; the fma of v;
    the normalize), about 2^-21 absolute on v.  The normalize divides by |v|, so where g lets s cancel r the same absolute
    error is 1 / |v| as large in d': the bar there is 2^-20 / |v|.  The draws are multiples of 2^-24 like exact::rng_next's, so
    u = 2 u2 - 1 is exact and rho loses nothing near the poles.  Cases whose |v| is below 2^-10 are two opposite vectors to
    the last bits; their direction is noise in any precision and only their length is looked at.
    The flag is compared wherever float64's |n . d'| exceeds the bar of d' summed over the three components, and the faceforward
    that comes first is decided: |n . d| above 2^-22 (binary32's n . d is three roundings of values below 1 away from it; below
    that the two precisions may face the normal either way, and the flag is about the faced normal)."""
    c = S.hostile_cases() if cases == "hostile" else S.seeded_cases()
    got = S.bounce32(oracle, c)
    want, nd, ln = S.bounce64(c)
    d = got[:, :3].astype(np.float64)
    assert np.isfinite(d).all() or cases == "hostile"
    sound = ln >= 2.0 ** -10
    assert sound.mean() > 0.95
    length = np.abs(np.linalg.norm(d[sound], axis=1) - 1.0)
    bar = BAR / np.minimum(1.0, ln[sound])
    err = np.abs(d[sound] - want[sound]).max(1)
    print(f"{cases}: {len(c)} cases, {sound.sum()} sound; max | |d'| - 1 | = {length.max():.3e}, max err / bar = {(err / bar).max():.3f}, "
          f"max err where |v| >= 1 = {err[ln[sound] >= 1.0].max():.3e} (bar {BAR:.3e})")
    assert (length <= BAR).all()
    assert (err <= bar).all()
    mirror = sound & (c[:, 8] == 0)
    assert mirror.sum() >= 100 and (np.abs(d[mirror] - want[mirror]).max(1) <= BAR).all(), "g = 0: the float64 mirror direction"
    faced = np.abs((c[:, :3].astype(np.float64) * c[:, 3:6]).sum(1)) > 2.0 ** -22      # the faceforward itself is decided
    decided = sound & faced & (np.abs(nd) > 3 * BAR / np.minimum(1.0, np.maximum(ln, 2.0 ** -10)))
    assert decided.sum() >= 0.5 * len(c)
    assert np.array_equal(got[decided, 3] != 0, ~(nd[decided] > 0))
    assert set(np.unique(got[:, 3])) <= {0.0, 1.0}
    if cases == "seeded":
        assert 0.02 < (got[:, 3] != 0).mean() < 0.6, "both ends occur"
    else:
        graze = (c[:, 8] == 0) & (np.abs((c[:, :3].astype(np.float64) * c[:, 3:6]).sum(1)) == 0)
        assert graze.any() and (got[graze, 3] == 1).all(), "n . d = 0 at g = 0: d' = d lies in the surface, absorbed"


@pytest.fixture()
def rule_files(tmp_path):
    (tmp_path / "a.obj").write_text(S.OBJ_RULE)
    (tmp_path / "lib.mtl").write_text(S.MTL_RULE)
    plain = tmp_path / "plain"
    plain.mkdir()
    (plain / "a.obj").write_text(S.OBJ_RULE)
    (plain / "lib.mtl").write_text(S.MTL_RULE_PLAIN)
    return str(tmp_path / "a.obj"), str(plain / "a.obj")


def test_loader_rule(hip_lib, rule_files):
    """illum 2 / 3 / 5, Ks 0 0 0, Ns absent / 0 / 1000, an emitter: the table the rule of include/rtpt.h states"""
    abi = hip_lib
    tri, m = abi.load_obj_materials_ext(rule_files[0])
    assert np.array_equal(tri, [0, 2, 2, 4, 0, 6])
    assert m.dtype == abi.MATERIAL_EXT and len(m) == 7
    gloss = np.sqrt(F32(2.0) / F32(1002.0))
    assert gloss.dtype == F32
    #            flags, roughness, Ks
    want = [(0, 0.0, (0, 0, 0)),                 # the default material
            (0, gloss, (0.5, 0.5, 0.5)),         # illum 2 stays diffuse
            (1, 0.0, (0.9, 0.8, 0.7)),           # no Ns: a mirror
            (1, 1.0, (0.5, 0.25, 0.125)),        # Ns 0: min(1, sqrt(2 / 2))
            (1, gloss, (1, 1, 1)),               # Ns 1000
            (0, np.sqrt(F32(2.0) / F32(12.0)), (0, 0, 0)),      # Ks 0 0 0 stays diffuse
            (0, 0.0, (0, 0, 0))]                 # the lamp
    for i, (flags, g, ks) in enumerate(want):
        assert m[i]["flags"] == flags and m[i]["_pad"] == 0, i
        assert bits(m[i]["roughness"]) == bits(F32(g)), i
        assert np.array_equal(m[i]["specular"], F32(ks)), i
    assert np.array_equal(m["albedo"][[1, 2, 3, 5]], F32([[0.1, 0.2, 0.3], [0.4, 0.4, 0.4], [0.7, 0.7, 0.7], [0.3, 0.2, 0.1]]))
    assert np.array_equal(m["emission"][6], F32([4, 3, 2])) and (m["emission"][:6] == 0).all()


def test_old_loader_is_unchanged_and_agrees(hip_lib, rule_files):
    """rtpt_util_load_obj_materials returns for the library with Ks / Ns / illum lines what it returns without them, and the
    new loader's Kd, Ke and indices are the old one's"""
    abi = hip_lib
    path, plain = rule_files
    for a, b in zip(abi.load_obj_materials(path), abi.load_obj_materials(plain)):
        assert np.array_equal(bits(a), bits(b))
    tri, mats = abi.load_obj_materials(path)
    tri_e, m = abi.load_obj_materials_ext(path)
    assert np.array_equal(tri, tri_e)
    assert np.array_equal(bits(mats), bits(np.concatenate([m["albedo"], m["emission"]], 1)))
    no_library = os.path.join(os.path.dirname(plain), "n.obj")
    with open(no_library, "w") as f:
        f.write("mtllib missing.mtl\nv 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert abi.load_obj_materials_ext(no_library) == (None, None)


def test_materials_ext_records(hip_lib):
    abi = hip_lib
    assert abi.MATERIAL_EXT.itemsize == 48 and abi.MAT_SPECULAR == 1
    m = abi.materials_ext(F32([[0.1, 0.2, 0.3, 0, 0, 0], [0.5, 0.5, 0.5, 1, 2, 3]]), {1: ((0.9, 0.8, 0.7), 0.25)})
    assert m[0]["flags"] == 0 and np.array_equal(m[0]["albedo"], F32([0.1, 0.2, 0.3])) and m[0]["roughness"] == 0
    assert m[1]["flags"] == 1 and m[1]["roughness"] == F32(0.25) and (m[1]["emission"] == 0).all()


def test_host_code_under_sanitizers(tmp_path):
    """`make -C csrc material-host-check`: the checks, the packing and the Ks / Ns / illum reader under the address and
    undefined-behaviour sanitizers, in a program of its own"""
    out = subprocess.run(["make", "-C", CSRC, "material-host-check", f"OBJDIR={tmp_path}"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "material_host_check ok" in out.stdout
