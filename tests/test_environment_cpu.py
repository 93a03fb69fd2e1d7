"""The environment map without a device: the float32 restatement of the lookup (tests/environment_maps.py: E1 to E6) against the
double-precision decode, rtpt_util_environment_from_latlong against its restatement, the refusals the host library decides without a
context, the host-only code under the sanitizers (csrc/tests/environment_host_check.cpp), and the seam that puts the restatement
into tests/path_walker.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import environment_maps as EM
import normal_paths as NP
import path_walker as WK
from conftest import ROOT, bits

F32 = np.float32
CSRC = os.path.join(ROOT, "real_time_path_tracing_with_spatiotemporal_filtering_amd", "csrc")

# The worst distance between the direction a 64 x 64 map of its own texel centres' directions returns and the unit direction asked
# for, over hostile_directions(), as the restatement itself gives it (measured when this test was written): bilinear 0.02839 — at
# (-1.875, -1.125, 0), on a fold of the lower sheet, where the clamped addressing costs its half texel; a texel there spans 0.05 —
# and nearest 0.06530.  With the rotation of EM.rotation(): 0.02679 and 0.05991.  The bars are those worst cases with a margin of a
# quarter.
DIRECTION_BARS = {(0, False): 0.02839 * 1.25, (EM.NEAREST, False): 0.06530 * 1.25, (0, True): 0.02679 * 1.25, (EM.NEAREST, True): 0.05991 * 1.25}


def _unit64(d):
    d = np.asarray(d, np.float64)
    return d / np.linalg.norm(d, axis=1)[:, None]


def refused32(d):
    """E2 on the direction itself (identity rotation), in plain float32: a component that is not finite, a sum that is 0 or overflows"""
    d = np.asarray(d, F32)
    with np.errstate(all="ignore"):
        s = ((np.abs(d[:, 0]) + np.abs(d[:, 1])).astype(F32) + np.abs(d[:, 2])).astype(F32)
    return ~np.isfinite(d).all(1) | ~(s > 0) | np.isinf(s)


def ordinary(d):
    """neither huge nor tiny: under a rotation a huge direction may overflow and a denormal one vanish, which is E2's business"""
    m = np.abs(np.asarray(d, F32)).max(1)
    return (m < 1e30) & (m > 1e-30)


# ------------------------------------------------------------------------------------------ the restatement against the decode
@pytest.mark.parametrize("flags", [0, EM.NEAREST])
@pytest.mark.parametrize("posed", [False, True])
def test_a_map_of_directions_returns_the_direction(oracle, flags, posed):
    d = EM.hostile_directions()
    ok = ~refused32(d) & (ordinary(d) | (not posed))
    rot = EM.rotation() if posed else None
    got = EM.color32(oracle, EM.make_env(EM.direction_map(64), flags, rot), d)
    want = _unit64(d[ok].astype(np.float64) @ (np.eye(3) if rot is None else rot.astype(np.float64)).T)
    err = np.linalg.norm(got[ok].astype(np.float64) - want, axis=1)
    worst = int(np.argmax(err))
    print(f"flags {flags} posed {posed}: worst {err.max():.5f} at {d[ok][worst]}, bar {DIRECTION_BARS[(flags, posed)]:.5f}")
    assert ok.sum() > 1500 and err.max() <= DIRECTION_BARS[(flags, posed)]


def test_a_constant_map_returns_the_constant_times_the_scale(oracle):
    d = EM.hostile_directions()
    ok = ~refused32(d)
    colour, scale = F32([0.3, 1e4, 7.25]), F32(EM.SCALE)
    want = (colour * scale).astype(F32)
    for n in EM.SIZES:
        tx = np.broadcast_to(np.append(colour, F32(0.5)).astype(F32), (n, n, 4))
        for flags in (0, EM.NEAREST):
            for rot in (None, EM.rotation()):
                got = EM.color32(oracle, EM.make_env(tx, flags, rot, scale), d)
                sel = ok if rot is None else ok & ordinary(d)
                assert np.array_equal(bits(got[sel]), bits(np.broadcast_to(want, got[sel].shape))), (n, flags, rot is not None)


def test_e2_refuses_with_zero(oracle):
    d = EM.hostile_directions()
    bad = refused32(d)
    assert bad.sum() >= 15 and np.isnan(d[bad]).any() and np.isinf(d[bad]).any() and (d[bad] == 0).all(1).any()
    for tag, env in EM.envs():
        got = EM.color32(oracle, env, d)
        if not tag[2]:
            assert np.array_equal(bits(got[bad]), np.zeros_like(bits(got[bad]))), tag
            assert (got[~bad] != 0).all(), tag                              # every texel of the generated maps is positive
        else:
            assert np.array_equal(bits(got[~np.isfinite(d).all(1)]), np.zeros((int((~np.isfinite(d).all(1)).sum()), 3), np.uint32)), tag


def test_the_generated_maps_and_directions_are_what_they_claim():
    for n in EM.SIZES:
        tx = EM.distinct_map(n)
        assert tx.shape == (n, n, 4) and np.isfinite(tx).all() and (tx[..., :3] >= 1e4).any()
        assert len({t.tobytes() for t in tx.reshape(-1, 4)}) == n * n
    d = EM.hostile_directions()
    as_set = {tuple(r) for r in bits(d).tolist()}
    for axis in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0]):
        assert tuple(bits(F32(axis)).tolist()) in as_set
    assert (bits(d) == 0x80000000).any() and (np.abs(d[np.isfinite(d)]) < 1e-38).any() and (np.abs(d[np.isfinite(d)]) > 1e38).any()


def test_exact_centres_and_borders(oracle):
    """the generator's directions for n = 64 land exactly on texel centres and borders: U * n and V * n are multiples of one half"""
    d = EM.hostile_directions()
    U, V, ok = EM.octahedral32(oracle, EM.make_env(EM.distinct_map(64)), d)
    on = ok & ((U * 128) % 1 == 0) & ((V * 128) % 1 == 0)
    centre = on & ((U * 64) % 1 == 0.5) & ((V * 64) % 1 == 0.5)
    border = on & (((U * 64) % 1 == 0) | ((V * 64) % 1 == 0))
    lower = d[:, 1] < 0
    assert (centre & lower).sum() > 20 and (centre & ~lower).sum() > 20 and (border & lower).sum() > 20 and (border & ~lower).sum() > 20


# ------------------------------------------------------------------------------------------ rtpt_util_environment_from_latlong
def _image(h, w, seed=3):
    rng = np.random.default_rng(seed)
    im = rng.random((h, w, 3)).astype(F32)
    im[rng.integers(0, h), rng.integers(0, w)] = 1e4       # a sun
    return im


def test_latlong_constant_image_gives_a_constant_map(hip_lib):
    im = np.broadcast_to(F32([0.25, 3.0, 1e4]), (7, 12, 3))
    for n in EM.SIZES:
        got = hip_lib.environment_from_latlong(im, n)
        assert got.shape == (n, n, 4)
        assert np.array_equal(bits(got), bits(np.broadcast_to(F32([0.25, 3.0, 1e4, 1.0]), got.shape))), n


def test_latlong_image_of_y_gives_a_map_of_y(hip_lib):
    """rows that are constant along their length: the texel depends on the decoded d.y only — equal |d.y| with equal sign gives equal
    texels, and the map falls monotonically from the centre (+y, row 0 of the image) to the corners (-y)"""
    h, w, n = 16, 5, 8
    im = np.broadcast_to((np.arange(h, dtype=F32) + 1)[:, None, None], (h, w, 3))
    got = hip_lib.environment_from_latlong(im, n)
    dy = EM.centres64(n)[..., 1]
    order = np.argsort(dy.ravel())
    vals = got[..., 0].ravel()[order]
    assert (np.diff(vals) <= 1e-5).all() and vals[0] > vals[-1]
    keys = np.round(dy.ravel(), 12)
    for k in np.unique(keys):
        same = got[..., 0].ravel()[keys == k]
        assert np.ptp(same) <= 1e-5 * same.max(), k
    assert np.array_equal(got[..., 0], got[..., 1]) and np.array_equal(got[..., 0], got[..., 2])


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (16, 32), (33, 17)])
def test_latlong_against_the_restatement(hip_lib, shape):
    im = _image(*shape)
    for n in EM.SIZES:
        got = hip_lib.environment_from_latlong(im, n)
        want = EM.from_latlong64(im, n)
        lo, hi = np.nextafter(want.astype(F32), F32(-np.inf)), np.nextafter(want.astype(F32), F32(np.inf))
        assert ((got >= lo) & (got <= hi)).all(), (shape, n, np.abs(got - want).max())


# ------------------------------------------------------------------------------------------ refusals the host decides
def test_refusals_without_a_context(hip_lib):
    abi = hip_lib
    lib = abi.load()
    one = np.ones((1, 1, 4), F32)
    assert lib.rtpt_set_environment(None, abi._ptr(one), 1, 0, None, None) == abi.RTPT_E_INVALID
    assert lib.rtpt_selftest_environment(None, abi._ptr(one), 1, abi._ptr(one)) == abi.RTPT_E_INVALID
    px, out = np.ones((1, 1, 3), F32), np.zeros((2, 2, 4), F32)
    f = lib.rtpt_util_environment_from_latlong
    assert f(None, 1, 1, 2, abi._ptr(out)) == abi.RTPT_E_INVALID and f(abi._ptr(px), 1, 1, 2, None) == abi.RTPT_E_INVALID
    for w, h, n in ((0, 1, 2), (1, 0, 2), (65537, 1, 2), (1, 65537, 2), (1, 1, 0), (1, 1, EM.MAX_SIZE + 1)):
        assert f(abi._ptr(px), w, h, n, abi._ptr(out)) == abi.RTPT_E_INVALID, (w, h, n)
    assert not out.any(), "a refused call writes nothing"
    assert f(abi._ptr(px), 1, 1, 2, abi._ptr(out)) == 0 and (out == 1).all()
    with pytest.raises(abi.RtptError):
        abi.environment_from_latlong(px, EM.MAX_SIZE + 1)
    with pytest.raises(ValueError):
        abi.environment_from_latlong(np.ones((2, 2), F32), 2)


def test_environment_host_check(tmp_path):
    """`make -C csrc environment-host-check`: the argument checks of rtpt_set_environment (size, flags, non-finite texels, rotation and
    scale, the A/B flag), the decode and the lat-long conversion under the address and undefined-behaviour sanitizers"""
    out = subprocess.run(["make", "-C", CSRC, "environment-host-check", f"OBJDIR={tmp_path}"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "environment_host_check: ok" in out.stdout.splitlines()


# ------------------------------------------------------------------------------------------ the walker's seam
def test_the_seam_is_transparent_and_counts(oracle):
    """with no environment the patched walker is the walker, bit for bit, and its counts are the paths that ended in the sky; with
    one, HIT_ID, seq_n and the ray count stay and the image changes exactly where a path ended there"""
    W, H = NP.SHAPE
    c, _ = NP.case(oracle, "uv_sphere")
    kw = NP.setup(oracle, c, 2)
    plain = WK.walk(oracle, c.sh.scene, W, H, 4, **kw)
    with EM.environment(oracle, None) as sky:
        same = WK.walk(oracle, c.sh.scene, W, H, 4, **kw)
    assert WK._contract.__module__ == "dielectric_scenes", "the seam is removed behind the walk"
    assert np.array_equal(bits(plain["IMAGE"]), bits(same["IMAGE"])) and len(sky) == 1 and len(sky[0]) == 4
    env = EM.make_env(EM.distinct_map(8), 0, EM.rotation(), EM.SCALE)
    with EM.environment(oracle, env) as smp:
        lit = WK.walk(oracle, c.sh.scene, W, H, 4, **kw)
    assert [len(a) for a in smp[0]] == [len(a) for a in sky[0]]
    assert np.array_equal(lit["HIT_ID"], plain["HIT_ID"]) and np.array_equal(lit["seq_n"], plain["seq_n"]) and lit["rays"] == plain["rays"]
    first, later = EM.shares(smp, W * H)
    assert first >= 0.1 and later >= 0.1
    changed = (bits(lit["IMAGE"]) != bits(plain["IMAGE"])).any(-1)
    assert changed.sum() >= 0.9 * (first + later) * W * H and changed.sum() <= round((first + later) * W * H)
