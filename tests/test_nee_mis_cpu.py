"""Multiple importance sampling of next-event estimation without a device (RTPT_FLAG_EXT_NEE_MIS; csrc/light_sample.hpp states
the rules): the numpy restatement of tests/nee_mis.py, which tests/test_nee_mis_gpu.py holds the device functions and the tile
kernels to bit for bit, is first held to exact values and to float64, its search to np.searchsorted, then the walker of
tests/path_walker.py with the flag off to the recorded frames of the walkers without it, and then to the estimator it replaces — the mean of its frames against the flag-off walker's, and its variance against
plain next-event estimation's where an emitter is close."""
import os
import subprocess

import numpy as np
import pytest

import dielectric_scenes as DS
import nee_mis as M
import nee_paths as NP
import nee_power as PW
import nee_scenes as N
import path_walker as WK
from conftest import bits

F32, U32 = np.float32, np.uint32
W0, H0 = N.SIZES[0]
W1, H1 = N.SIZES[1]
ESTIMATOR_FRAMES = 2048
NONE = np.zeros(0, U32)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "real_time_path_tracing_with_spatiotemporal_filtering_amd", "csrc")

# measured against float64 on nee_mis.seeded_g (4,096 weights over twelve decades): wb 1.567e-7 relative, gm 1.342e-7 relative — three
# roundings each (the square, the sum, the division) and gm's multiply.  Each bar is the next power of two above four times the
# measurement (6.27e-7, 5.37e-7).
WB_BAR = 2.0 ** -20
GM_BAR = 2.0 ** -20


# ------------------------------------------------------------------------------------------ the weights
def test_weights_on_hostile_operands():
    """g = 0, subnormal, 1, 2, 2^63, 2^64 and above (g2 overflows), +inf, NaN, negative: 0 <= wb <= 1 everywhere, wb(inf) = wb(NaN) =
    1, gm <= 0.5 wherever it is a number and gm = 0 where a finite g's square overflows; exact values where they are dyadic.  g =
    +inf and g = NaN give gm = NaN (inf * 0 by the rule's one multiply): the only operands that do"""
    g = M.G_HOSTILE
    w_b, g_m = M.wb(g), M.gm(g)
    assert w_b.dtype == F32 and g_m.dtype == F32
    assert ((w_b >= 0) & (w_b <= 1)).all(), "0 <= wb <= 1, NaN operands included"
    assert not (g_m > 0.5).any()
    nan = np.isnan(g_m)
    assert np.array_equal(nan, np.isinf(g) | np.isnan(g)), "gm is a number but for g = +-inf and NaN"
    assert (g_m[~nan] <= 0.5).all()
    with np.errstate(all="ignore"):
        over = np.isfinite(g) & np.isinf((g * g).astype(F32))
    assert over.sum() >= 4 and (g_m[over] == 0).all() and (w_b[over] == 1).all(), "g2 = inf: the light side weighs 0, the bounce 1"
    assert M.wb(F32(np.inf)) == 1 and M.wb(F32(np.nan)) == 1 and M.wb(F32(-np.inf)) == 1
    exact = {0.0: (0.0, 0.0), 1.0: (0.5, 0.5), 2.0: (float(F32(4.0) / F32(5.0)), float(F32(2.0) * (F32(1.0) / F32(5.0)))),
             2.0 ** 63: (1.0, 2.0 ** -63), 2.0 ** 64: (1.0, 0.0), -1.0: (0.5, -0.5)}
    for x, (want_wb, want_gm) in exact.items():
        assert float(M.wb(F32(x))) == want_wb and float(M.gm(F32(x))) == want_gm, x
    tiny = F32(1e-40)                                             # subnormal: its square is 0
    assert M.wb(tiny) == 0 and bits(M.gm(tiny)) == bits(tiny)
    # the heuristic's two sides add up to 1 where both are numbers: m + wb, to a rounding each
    s = M.seeded_g()
    assert np.abs(M.m_light(s).astype(np.float64) + M.wb(s).astype(np.float64) - 1).max() <= 2.0 ** -23


def test_weights_against_float64():
    """wb and gm on 4,096 seeded weights over twelve decades against float64 from the same float32 g, relative error.
    Measured: wb 1.567e-7, gm 1.342e-7 (bars 2^-20 = 9.54e-7)."""
    g = M.seeded_g()
    want_wb, want_gm = M.weights64(g)
    rel_wb = np.abs(M.wb(g).astype(np.float64) - want_wb) / want_wb
    rel_gm = np.abs(M.gm(g).astype(np.float64) - want_gm) / want_gm
    print(f"wb vs float64: max rel err {rel_wb.max():.3e} (bar {WB_BAR:.3e}); gm {rel_gm.max():.3e} (bar {GM_BAR:.3e})")
    assert rel_wb.max() <= WB_BAR and rel_gm.max() <= GM_BAR


def test_hit_weight_against_float64(oracle):
    """g_hit of nee_mis.seeded_cases against the same formula in float64 from the float32 operands; and on the hostile rows the
    restatement's outputs stay inside the rules' ranges (0 <= wb <= 1, gm never above 0.5), q_i = 0 (inv_p = inf) weighs the bounce
    1 whatever cb * cl is, and cl = 0 weighs it 0.
    Measured: max rel err of g_hit 1.587e-5 over the 4,041 of 4,096 cases whose float64 cl is above 2^-6 (the cross product of a
    thin emitter and the dot of its normal with d cancel); the bar, 2^-13, is the next power of two above four times that."""
    c = M.seeded_cases()
    got = M.mis_weight32(oracle, c)
    f = c.astype(np.float64)
    v0, v1, v2, o, d = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12:15]
    b1, b2, cb, inv_p = f[:, 15], f[:, 16], f[:, 17], f[:, 18]
    cr = np.cross(v1 - v0, v2 - v0)
    a2 = np.linalg.norm(cr, axis=1)
    y = v0 * (1 - b1 - b2)[:, None] + v1 * b1[:, None] + v2 * b2[:, None]
    cl = np.abs(((cr / a2[:, None]) * d).sum(1))
    want = cb * cl * a2 * inv_p / (2 * np.pi * ((y - o) ** 2).sum(1))
    clear = cl > 2.0 ** -6                                        # a grazing ray's cosine cancels in float32
    rel = np.abs(got[clear, 0].astype(np.float64) - want[clear]) / want[clear]
    print(f"g_hit vs float64: max rel err {rel.max():.3e} over {clear.sum()} of {len(c)} cases")
    assert clear.mean() > 0.95 and rel.max() <= 2.0 ** -13
    h = M.mis_weight32(oracle, M.hostile_cases())
    assert ((h[:, 1] >= 0) & (h[:, 1] <= 1)).all() and not (h[:, 2] > 0.5).any()
    assert h[0, 0] > 0 and 0 < h[0, 1] < 1
    assert h[1, 0] == 0 and h[1, 1] == 0, "cl = 0: the bounce grazes, g_hit = 0"
    assert h[2, 1] == 0, "cb = 0"
    assert np.isinf(h[3, 0]) and h[3, 1] == 1 and np.isnan(h[4, 0]) and h[4, 1] == 1, "q_i = 0 by the formula: wb = 1 either way"
    assert h[5, 1] == 1 and h[7, 1] == 1 and h[14, 1] == 1, "NaN and r2 = 0"
    assert h[10, 1] == 1 and h[10, 2] == 0 and np.isfinite(h[10, 0]), "g2 overflows"


# ------------------------------------------------------------------------------------------ the search
@pytest.mark.parametrize("n", M.FIND_SIZES)
def test_find_equals_searchsorted(n):
    """nee_mis.find against np.searchsorted on ascending lists of 1, 2, 3, 1,000 and 2^20 + 1,025 ids: both ends, every entry,
    every gap, ids below, above and between the entries"""
    ids, q = M.find_case(n)
    got = M.find(ids, q)
    i = np.searchsorted(ids, q, side="left")
    held = (i < n) & (ids[np.minimum(i, n - 1)] == q)
    want = np.where(held, i, n)
    assert got.dtype == U32 and np.array_equal(got, want)
    assert held.sum() >= min(n, 1000) and (~held).sum() >= 7
    assert np.array_equal(M.find(ids, ids[[0, n - 1]]), [0, n - 1])
    assert np.array_equal(M.find(NONE, q[:5]), np.zeros(5, U32)), "an empty list holds nothing: n = 0"


def test_light_find_host_check(tmp_path):
    """`make -C csrc light-find-host-check`: rtpt_light::find of csrc/light_list_host.hpp, the search the device runs, on lists that
    are allocations of their own length, under the address and undefined-behaviour sanitizers"""
    out = subprocess.run(["make", "-C", CSRC, "light-find-host-check", f"OBJDIR={tmp_path}"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "light_find_host_check: ok" in out.stdout.splitlines()


def test_hit_inv_p_of_the_weighted_pick():
    """the inverse probability of a hit emitter's entry is the one pick_power returns for a draw that lands on it; an entry of weight
    0 and an id outside the list are not reached"""
    w = np.ones(37, F32)
    w[[0, 5, 6, 36]] = 0
    w[20] = 9.0
    cdf = PW.table(w)
    lights = (3 + 2 * np.arange(37)).astype(U32)
    m = np.arange(0, 1 << 24, 1 << 10, dtype=np.uint32)
    entry, inv_p = PW.pick_power(cdf, (m.astype(F32) * F32(2.0 ** -24)).astype(F32))
    reached, got = M.hit_inv_p(lights, cdf, lights[entry])
    assert reached.all() and np.array_equal(bits(got), bits(inv_p))
    assert set(entry.tolist()) == set(np.flatnonzero(w > 0).tolist())
    reached, _ = M.hit_inv_p(lights, cdf, np.concatenate([lights[[0, 5, 6, 36]], U32([0, 4, 2, 1000])]))
    assert not reached.any()
    reached, got = M.hit_inv_p(lights, None, U32([3, 4, 77]))
    assert reached.all() and (got == 37).all(), "the uniform pick: float(L), whatever the id"


# ------------------------------------------------------------------------------------------ the walker against the walkers
def _same(got, want, counts=True):
    assert np.array_equal(bits(got["IMAGE"]), bits(want["IMAGE"])) and np.array_equal(got["HIT_ID"], want["HIT_ID"])
    if counts:
        for k in want:
            if not isinstance(want[k], np.ndarray):
                assert got[k] == want[k], k
            else:
                assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("power,sphere", [(False, False), (True, False), (True, True)], ids=["uniform", "weighted", "weighted_sphere"])
def test_mis_off_is_the_power_walker(oracle, power, sphere):
    """with `mis` off the walker is the recorded nee_power.walk_nee_power bit for bit — IMAGE, HIT_ID, rays, every count and the picks — on
    nee_two_lamps and on the glass room with two lamps (diffuse, dielectric and emissive hits; 9 segments, two samples); and with
    it on the frame differs while the samples, the queries and the rays do not"""
    room, glass, rec = PW.glass_room_two_lamps()
    two = NP.two_lamps()
    for sc, r, li, seg, spp in ((two, DS.records(two), NP.light_list(two), 5, 1), (room, rec, NP.light_list(room, 1, rec), 9, 2)):
        want = WK.recorded("nee_mis/PW", sc.name, seg, spp, power, sphere)
        got = WK.walk(oracle, sc, W1, H1, seg, r, li, mis=False, power=power, sphere=sphere, spp=spp)
        _same(got, want)
        on = WK.walk(oracle, sc, W1, H1, seg, r, li, mis=True, power=power, sphere=sphere, spp=spp)
        assert not np.array_equal(bits(on["IMAGE"]), bits(want["IMAGE"]))
        assert on["rays"] == want["rays"] and on["samples"] == want["samples"] and on["queries"] == want["queries"]
        assert np.array_equal(on["HIT_ID"], want["HIT_ID"]) and np.array_equal(on["picks"], want["picks"])


def test_one_segment_and_an_empty_list_ignore_the_flag(oracle):
    """max_segments = 1 with the flag is flag off (no hit samples, no bit is ever set); an empty list is the recorded
    nee_sphere.walk_nee_sphere, with the sphere sample and without; a batch of frames is the frames one by one"""
    room, glass, rec = PW.glass_room_two_lamps()
    lights = NP.light_list(room, 1, rec)
    one = WK.walk(oracle, room, W1, H1, 1, rec, lights, mis=True, power=True)
    _same(one, WK.recorded("nee_mis/DS", "one"), counts=False)
    assert one["samples"] == 0 and one["weighted"] == 0
    for sphere in (False, True):
        empty = WK.walk(oracle, room, W1, H1, 9, rec, NONE, mis=True, sphere=sphere, power=True)
        want = WK.recorded("nee_mis/NS", "empty", sphere)
        _same(empty, want, counts=False)
        assert empty["rays"] == want["rays"]
    sc = M.wall_lamp()
    r, li = DS.records(sc), NP.light_list(sc)
    batch = WK.walk(oracle, sc, W1, H1, 2, r, li, mis=True, frames=[0, 7, 3])
    for i, f in enumerate((0, 7, 3)):
        single = WK.walk(oracle, sc, W1, H1, 2, r, li, mis=True, frame=f)
        assert np.array_equal(bits(batch["IMAGE"][i]), bits(single["IMAGE"])) and np.array_equal(batch["HIT_ID"][i], single["HIT_ID"])


def test_every_scene_has_weighted_terminals(oracle):
    """the scenes of the frame tests, 64 x 48 at two segments: emissive triangles are met with the sampled bit set (the walker's
    `dropped`), with weights strictly between 0 and 1; the wall of nee_wall_lamp is never seen directly"""
    room, glass, rec = PW.glass_room_two_lamps()
    cases = [(sc, DS.records(sc), NP.light_list(sc)) for sc in (M.wall_lamp(), NP.two_lamps(), NP.occluder(), PW.unequal_lamps())]
    cases.append((room, rec, NP.light_list(room, 1, rec)))
    for sc, r, li in cases:
        got = WK.walk(oracle, sc, W0, H0, 2, r, li, mis=True)
        print(f"{sc.name}: {got['weighted']} weighted terminals, wb in [{got['wb_min']:.3g}, {got['wb_max']:.3g}]")
        assert got["dropped"] == got["weighted"] > 0 and 0 <= got["wb_min"] < got["wb_max"] < 1, sc.name
    wall = WK.walk(oracle, M.wall_lamp(), W0, H0, 2, *cases[0][1:], mis=True)
    lit = set(int(i) for i in cases[0][2])
    assert not lit & set(np.unique(wall["HIT_ID"]).tolist()), "the wall stands outside the view"
    nine = WK.walk(oracle, room, W0, H0, 9, rec, cases[-1][2], mis=True)
    assert nine["kept"] > 0 and nine["weighted"] > 0, "behind a mirror or glass hit the bit is clear"


# ------------------------------------------------------------------------------------------ the estimator is right
_var = {}


@pytest.mark.parametrize("name", ["nee_wall_lamp", "nee_two_lamps", "nee_occluder"])
def test_mis_estimates_what_the_path_tracer_estimates(oracle, name):
    """70 x 10, two segments, frames 0 .. 2047, uniform pick: the per-pixel mean of the walker's frames with `mis` against the mean of the
    flag-off walker's (the same walker on an empty list) within 5 standard errors of the difference at every pixel and channel,
    none left out — the bar of test_nee_paths_cpu.py, test_nee_sphere_cpu.py and test_nee_power_cpu.py; pixels whose two sides
    never vary have to differ by exactly 0.  On nee_wall_lamp the summed per-pixel variance with MIS is below plain next-event
    estimation's (the bar); the ratios elsewhere are printed as measurements.
    Measured (2,048 frames): nee_wall_lamp max |z| 3.45, variance MIS / NEE 0.300, MIS / flag-off 0.357, NEE / flag-off 1.190;
    nee_two_lamps max |z| 3.53, MIS / NEE 0.985; nee_occluder max |z| 3.30, MIS / NEE 0.997."""
    scene = {"nee_wall_lamp": M.wall_lamp, "nee_two_lamps": NP.two_lamps, "nee_occluder": NP.occluder}[name]()
    rec = DS.records(scene)
    lights = NP.light_list(scene)
    n = ESTIMATOR_FRAMES
    run = lambda li, mis: WK.walk(oracle, scene, W1, H1, 2, rec, li, mis=mis, frames=range(n))
    on_r = run(lights, True)
    on = on_r["IMAGE"][..., :3].reshape(n, -1)
    nee = run(lights, False)["IMAGE"][..., :3].reshape(n, -1)
    off = run(NONE, False)["IMAGE"][..., :3].reshape(n, -1)
    assert on_r["weighted"] > 0
    a, b, c = on.astype(np.float64), off.astype(np.float64), nee.astype(np.float64)
    se = np.sqrt(a.var(0, ddof=1) / n + b.var(0, ddof=1) / n)
    diff = a.mean(0) - b.mean(0)
    with np.errstate(all="ignore"):
        z = np.where(se > 0, diff / se, np.where(diff == 0, 0.0, np.inf))      # no pixel is left out
    va, vb, vc = a.var(0, ddof=1).sum(), b.var(0, ddof=1).sum(), c.var(0, ddof=1).sum()
    print(f"MIS vs flag-off, {name}, {W1} x {H1} x {n} frames: max |z| {np.abs(z).max():.2f} over {z.size} values (above 4: "
          f"{(np.abs(z) > 4).sum()}; {(se > 0).sum()} with a standard error above 0), {on_r['weighted']} weighted terminals, wb in "
          f"[{on_r['wb_min']:.3g}, {on_r['wb_max']:.3g}]; summed variance MIS / NEE {va / vc:.3f}, MIS / flag-off {va / vb:.3f}, "
          f"NEE / flag-off {vc / vb:.3f}")
    assert (se > 0).sum() > 100
    assert np.abs(z).max() <= 5.0
    if name == "nee_wall_lamp":
        assert va < vc, "with a close emitter MIS has less variance than next-event estimation alone"


# ------------------------------------------------------------------------------------------ the binding
def test_every_exported_symbol_has_a_signature(hip_lib):
    """the flag's value, the two new entry points with their ctypes signatures, and argtypes on every symbol of the binding"""
    abi = hip_lib
    assert abi.FLAG_EXT_NEE_MIS == 0x80000 and not abi.FLAG_EXT_NEE_MIS & abi.FLAG_EXT_MASK
    lib = abi.load()
    for name, n_args in (("rtpt_selftest_mis_weight", 4), ("rtpt_selftest_light_find", 6)):
        assert name in abi.SYMBOLS and len(getattr(lib, name).argtypes) == n_args, name
    for name in abi.SYMBOLS:
        assert getattr(lib, name).argtypes is not None, name
