"""The weighted light pick of next-event estimation without a device (RTPT_FLAG_EXT_NEE_POWER; csrc/light_sample.hpp states the
rules): the numpy restatement of tests/nee_power.py, which tests/test_nee_power_gpu.py holds the table builder, the pick and the
tile kernels to bit for bit, is first held to exact arithmetic — the table to Python integers and Fractions on hostile weights,
the pick to an enumeration of all 2^24 draws — then the walker of tests/path_walker.py with the flag off to the recorded frames of the
walkers without it, and then to the estimator it replaces: the mean
of its frames against the mean of the flag-off walker's."""
from fractions import Fraction

import numpy as np
import pytest

import dielectric_scenes as DS
import nee_paths as NP
import nee_power as PW
import nee_scenes as N
import path_walker as WK
from conftest import bits

F32, U32, U64 = np.float32, np.uint32, np.uint64
W0, H0 = N.SIZES[0]
W1, H1 = N.SIZES[1]
ESTIMATOR_FRAMES = 8192
NONE = np.zeros(0, U32)


# ------------------------------------------------------------------------------------------ exact arithmetic
def f32_of(x):
    """the binary32 nearest the non-negative Fraction x, ties to even, as a Fraction (no overflow: x < 2^128 here)"""
    if x == 0:
        return Fraction(0)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n, r = divmod(x / ulp, 1)
    n = int(n)
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n & 1):
        n += 1
    return n * ulp


def exact_table(w):
    """the table of the weights w in Python integers: list of C_i"""
    ok = [Fraction(float(x)) if (x > 0 and np.isfinite(x)) else Fraction(0) for x in np.asarray(w, F32)]
    w_max = max(ok) if ok else Fraction(0)
    out, c = [], 0
    for x in ok:
        if w_max == 0:
            q = 1
        elif x > 0:
            q = max(1, int(f32_of(x / w_max) * 65536))           # (x 2^16 is exact in binary32; uint32() truncates)
        else:
            q = 0
        assert q <= 1 << 16
        c += q
        out.append(c)
    return out


@pytest.mark.parametrize("n", [1, 2, 65, 1000])
@pytest.mark.parametrize("kind", PW.HOSTILE + ("skewed",))
def test_table_equals_integer_arithmetic(kind, n):
    """table() against Python-integer and Fraction arithmetic on the hostile weights — zeros between positives, all zeros, one
    weight of 1e30 beside ones, subnormals, NaN and the infinities, equal weights, a ratio just below and just at 2^-16 — and on
    seeded skewed ones"""
    w = PW.skewed_weights(n) if kind == "skewed" else PW.hostile_weights(n, kind)
    got = PW.table(w)
    assert got.dtype == U64 and [int(c) for c in got] == exact_table(w), (kind, n)
    q = np.diff(np.concatenate([[0], got.astype(np.int64)]))
    if kind == "all_zero":
        assert (q == 1).all()
    if kind == "nan_inf":
        if n >= 5:
            assert (q[~(np.isfinite(w) & (w > 0))] == 0).all() and (q[4::5] == 65536).all()
        else:
            assert (q == 1).all(), "nothing counts: w_max == 0, the uniform pick"
    if kind in ("ratio_below", "ratio_at") and n > 1:
        assert sorted(set(q.tolist())) == [1, 65536], "below 2^-16 the quotient quantises to 0 and is lifted to 1; at 2^-16 it is 1"
    if kind == "one_huge" and n > 1:
        assert q[n // 2] == 65536 and (np.delete(q, n // 2) == 1).all()
    if kind == "subnormals" and n <= 4:
        assert q.max() == 65536 and q.min() >= 1, "subnormal weights alone: the largest is the maximum"


def pick_tables():
    g = np.random.default_rng(59)
    zeros = np.ones(37, F32)
    zeros[[0, 1, 5, 6, 7, 20, 35, 36]] = 0               # runs of zeros at both ends and inside
    huge = np.ones(100, F32)
    huge[40] = 1e30
    return {"zeros": zeros, "one_huge": huge, "all_zero": np.zeros(13, F32), "skewed_1000": PW.skewed_weights(1000),
            "single": F32([3.0]), "random_8": g.random(8).astype(F32)}


@pytest.mark.parametrize("name", ["zeros", "one_huge", "all_zero", "skewed_1000", "single", "random_8"])
def test_pick_enumerated_over_every_draw(name):
    """all 2^24 values of the draw on tables of up to 1,000 entries: entry i is picked within 1 of q_i 2^24 / S times, a
    zero-weight entry never, u_l = 0 lands on the first positive entry and u_l = 1 - 2^-24 on the last, and inv_p is
    float(S) / float(q_i), correctly rounded"""
    w = pick_tables()[name]
    cdf = PW.table(w)
    L, S = len(cdf), int(cdf[-1])
    q = np.diff(np.concatenate([[0], cdf.astype(np.int64)]))
    m = np.arange(1 << 24, dtype=np.uint32)
    u = (m.astype(F32) * F32(2.0 ** -24)).astype(F32)
    assert (u < 1).all() and ((u * F32(1 << 24)).astype(np.uint32) == m).all(), "a draw is a multiple of 2^-24: m is exact"
    entry, inv_p = PW.pick_power(cdf, u)
    assert (entry.astype(np.int64) == np.searchsorted(cdf, (m.astype(U64) * U64(S)) >> U64(24), side="right")).all()
    count = np.bincount(entry, minlength=L)
    assert np.abs(count - q * float(1 << 24) / S).max() <= 1, name
    assert count[q == 0].sum() == 0, "a zero-weight entry is never picked"
    positive = np.flatnonzero(q > 0)
    assert entry[0] == positive[0] and entry[-1] == positive[-1]
    for i in positive[:: max(1, len(positive) // 16)]:
        want = f32_of(f32_of(Fraction(S)) / Fraction(int(q[i])))
        got = inv_p[np.flatnonzero(entry == i)[0]]
        assert Fraction(float(got)) == want and (inv_p[entry == i] == got).all(), (name, i)
    assert S <= 1 << 24, "these tables are below the known limit: no entry can be skipped"


# ------------------------------------------------------------------------------------------ the walker against the walkers
def test_equal_weights_pick_as_the_uniform_walker(oracle):
    """nee_power.equal_lamps(): four emitters of one weight, L = 4 divides 2^16 and u_l * 4 is exact, so the weighted walk picks
    the entries the uniform one picks and, with inv_p = 4.0f = float(L), renders the recorded frame of nee_paths.walk_nee bit for bit,
    rays included"""
    scene = PW.equal_lamps()
    rec = DS.records(scene)
    lights = NP.light_list(scene)
    assert PW.table(PW.weights(oracle, scene.tris, rec, lights)).tolist() == [65536, 131072, 196608, 262144]
    for segments in (2, 5):
        got = WK.walk(oracle, scene, W0, H0, segments, rec, lights, power=True)
        off = WK.walk(oracle, scene, W0, H0, segments, rec, lights, power=False)
        want = WK.recorded("nee_power_equal/NP", segments)
        assert (got["picks"] == off["picks"]).all() and got["picks"].min() > 0
        assert np.array_equal(bits(got["IMAGE"]), bits(want["IMAGE"])) and np.array_equal(got["HIT_ID"], want["HIT_ID"])
        assert got["rays"] == want["rays"] and got["lit"] == want["lit"] > 0


@pytest.mark.parametrize("sphere", [False, True], ids=["triangles", "both"])
def test_power_off_is_the_sphere_walker(oracle, sphere):
    """with `power` off the walker is the recorded nee_sphere.walk_nee_sphere bit for bit — IMAGE, HIT_ID, rays and every count — on the
    glass room with its second lamp (diffuse, dielectric and emissive hits), 9 segments and two samples, and on two_lamps; and
    with it on the frame differs"""
    scene, glass, rec = PW.glass_room_two_lamps()
    lights = NP.light_list(scene, 1, rec)
    assert len(lights) == 4
    for sc, r, li, seg, spp in ((scene, rec, lights, 9, 2), (NP.two_lamps(), DS.records(NP.two_lamps()), NP.light_list(NP.two_lamps()), 5, 1)):
        want = WK.recorded("nee_power/NS", sc.name, seg, spp, sphere)
        got = WK.walk(oracle, sc, W1, H1, seg, r, li, sphere=sphere, power=False, spp=spp)
        assert np.array_equal(bits(got["IMAGE"]), bits(want["IMAGE"])) and np.array_equal(got["HIT_ID"], want["HIT_ID"])
        for k in want:
            if not isinstance(want[k], np.ndarray):
                assert got[k] == want[k], k
        on = WK.walk(oracle, sc, W1, H1, seg, r, li, sphere=sphere, power=True, spp=spp)
        assert not np.array_equal(bits(on["IMAGE"]), bits(want["IMAGE"])) and on["samples"] == want["samples"]
    empty = WK.walk(oracle, scene, W1, H1, 9, rec, NONE, sphere=True, power=True)
    want = WK.recorded("nee_power/NS", "empty")
    assert np.array_equal(bits(empty["IMAGE"]), bits(want["IMAGE"])), "an empty list: nothing to pick"


def test_the_degenerate_emitter_is_never_picked(oracle):
    """nee_paths.two_lamps(): its degenerate emissive triangle is in the list with weight 0 — the weighted walker never draws
    it, the uniform one does"""
    scene = NP.two_lamps()
    rec = DS.records(scene)
    lights = NP.light_list(scene)
    w = PW.weights(oracle, scene.tris, rec, lights)
    assert len(lights) == 5 and w[4] == 0 and (w[:4] > 0).all()
    on = WK.walk(oracle, scene, W0, H0, 3, rec, lights, power=True)
    off = WK.walk(oracle, scene, W0, H0, 3, rec, lights, power=False)
    assert on["picks"][4] == 0 and off["picks"][4] > 0 and on["queries"] > off["queries"]


# ------------------------------------------------------------------------------------------ the estimator is right
@pytest.mark.parametrize("name", ["two_lamps", "receiver"])
def test_weighted_nee_estimates_what_the_path_tracer_estimates(oracle, name):
    """nee_paths.two_lamps() and nee_scenes.receiver() at 70 x 10, two segments, frames 0 .. 8191: the per-pixel mean of
    the weighted walker's frames against the mean of the flag-off walker's (no list) within 5 standard errors of the
    difference at every pixel and channel, none left out — the bar of test_nee_paths_cpu.py and test_nee_sphere_cpu.py, where the
    pixels that see the sky store the same bits on both sides and have to differ by exactly 0.  The ratio of the summed per-pixel
    variance, weighted against uniform, is printed: a measurement, not a bar.
    Measured: two_lamps max |z| 3.26 over 2100 values (none above 4), summed variance weighted / uniform 0.803, weighted /
    flag-off 0.225; receiver max |z| 3.27 (none above 4), weighted / uniform 0.967, weighted / flag-off 0.226."""
    scene = NP.two_lamps() if name == "two_lamps" else N.receiver()
    rec = DS.records(scene)
    lights = NP.light_list(scene)
    n = ESTIMATOR_FRAMES
    on = np.zeros((n, H1 * W1 * 3), F32)
    uni = np.zeros_like(on)
    off = np.zeros_like(on)
    for f in range(n):
        on[f] = WK.walk(oracle, scene, W1, H1, 2, rec, lights, power=True, frame=f)["IMAGE"][..., :3].ravel()
        uni[f] = WK.walk(oracle, scene, W1, H1, 2, rec, lights, power=False, frame=f)["IMAGE"][..., :3].ravel()
        off[f] = WK.walk(oracle, scene, W1, H1, 2, rec, frame=f)["IMAGE"][..., :3].ravel()
    a, b, c = on.astype(np.float64), off.astype(np.float64), uni.astype(np.float64)
    se = np.sqrt(a.var(0, ddof=1) / n + b.var(0, ddof=1) / n)
    diff = a.mean(0) - b.mean(0)
    with np.errstate(all="ignore"):
        z = np.where(se > 0, diff / se, np.where(diff == 0, 0.0, np.inf))      # no pixel is left out
    assert (se > 0).sum() == 3 * 160 and ((se > 0) | (bits(on[0]) == bits(off[0]))).all()
    print(f"weighted NEE vs flag-off, {name}, {W1} x {H1} x {n} frames: max |z| {np.abs(z).max():.2f} over {z.size} values "
          f"(above 4: {(np.abs(z) > 4).sum()}), summed variance weighted / uniform {a.var(0, ddof=1).sum() / c.var(0, ddof=1).sum():.3f}, "
          f"weighted / flag-off {a.var(0, ddof=1).sum() / b.var(0, ddof=1).sum():.3f}")
    assert np.abs(z).max() <= 5.0


# ------------------------------------------------------------------------------------------ the binding
def test_the_new_entry_points_have_signatures(hip_lib):
    """the flag's value, and every new entry point resolved with its ctypes signature"""
    abi = hip_lib
    assert abi.FLAG_EXT_NEE_POWER == 0x40000 and not abi.FLAG_EXT_NEE_POWER & abi.FLAG_EXT_MASK
    lib = abi.load()
    for name, n_args in (("rtpt_selftest_light_table", 4), ("rtpt_selftest_light_pick", 7), ("rtpt_debug_light_table", 4)):
        assert name in abi.SYMBOLS and len(getattr(lib, name).argtypes) == n_args, name
    assert PW.scratch_bytes(1) == 8 + 8 + 4 and PW.scratch_bytes(1025) == 8 + 8 * 3 + 4 * 1025
    assert PW.scratch_bytes((1 << 20) + 1025) == 8 + 8 * (1026 + 2 + 1) + 4 * ((1 << 20) + 1025)
