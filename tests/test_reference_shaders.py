"""The oracle and the HIP path against the reference's own shader text.

oracle/refshader/ compiles the reference's three compute shaders (raytrace, temporalGradient, temporalFiltering) as C++
after a purely syntactic pre-pass and executes them on the CPU in two arithmetics: R32 (binary32, every operator
unfused and in the text's order, the numerics contract's builtins) and R64 (double, libm).  Executing the text cannot
misread it: a transcription slip shared by the oracle and the kernels (both written from one reading) shows here.

Bars are measured, not chosen (tests/golden/refshader_bars.json, written by tests/golden/make_refshader.py): for each float
observable the bar is 4 x the largest R32-vs-R64 error over the test inputs, i.e. the reference text's own binary32
rounding noise; integer observables are exact, up to the stated shares of pixels that sit on a rounding boundary.

Live tests need oracle/_ref/librefshader.so (built where the reference tree is; it travels to the GPU machine) and skip
by name without it.  The fixture tests read tests/golden/refshader_cornell_64x48.npz — recorded runs of the reference
text — and never skip.  K0 (rasterisation), the driver's ray-triangle arithmetic / tie rule (D4) and the vendor's
transcendental precision stay unpinned.

Not observed: the number of RNG draws per segment.  `rngState` is a by-value parameter of the bounce loop and no output
carries it; what is observed instead is its consequence, every bounce direction, through the id sequences.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, bits
from oracle.refshader import compare as X
from oracle.refshader import refshader as R

GOLDEN = os.path.join(ROOT, "tests", "golden")
BARS = json.load(open(os.path.join(GOLDEN, "refshader_bars.json")))["bars"]
FIXTURE = os.path.join(GOLDEN, "refshader_cornell_64x48.npz")
FILTER_TOL = 1e-5  # test_parity_gpu.py: the hardware-exp filter against the oracle

live = pytest.mark.skipif(not R.available(), reason="oracle/_ref/librefshader.so not built (needs the reference tree)")


def _reference_dir():
    import __graft_entry__ as g
    return g._reference_dir()


def _scene(name, cornell):
    return cornell[2] if name == "cornell" else X.sphere_scene()


def _noise(key, value, tag):
    """the bar really is 4 x the reference text's own noise on the test inputs: a stale or inflated bars file fails here"""
    assert value <= BARS[key] / 4.0 * (1 + 1e-9), (tag, key, value, BARS[key] / 4.0)


def _check_common(obs, tag):
    """the assertions every traced / gradient comparison shares"""
    for key in ("traced", "dir0", "lambda"):
        _noise(key, obs[key]["r32/r64"], tag)
    for pair in ("r32/r64", "oracle/r32", "oracle/r64"):  # R32/R64 — the reference text alone — first
        print(tag, pair, {k: obs[k].get(pair) for k in ("diverged", "traced", "dir0", "lambda")})
        assert obs["diverged"][pair] <= X.MAX_DIVERGED, (tag, pair, obs["diverged"][pair])
        assert obs["traced"][pair] <= BARS["traced"], (tag, pair, obs["traced"][pair])
        assert obs["dir0"][pair] <= BARS["dir0"], (tag, pair, obs["dir0"][pair])
        assert obs["lambda"][pair] <= BARS["lambda"], (tag, pair, obs["lambda"][pair])


# ------------------------------------------------------------------------------------------ the host itself
def test_bars_are_four_times_the_measured_noise_and_conditions_hold():
    doc = json.load(open(os.path.join(GOLDEN, "refshader_bars.json")))
    assert doc["factor"] == 4.0 and doc["colour_floor"] == X.COLOUR_FLOOR
    for key, bar in doc["bars"].items():
        assert bar == 4.0 * doc["measured"][key]["r32/r64"]["value"] > 0
        for pair in ("oracle/r32", "oracle/r64"):  # what the generator observed of the oracle lies inside
            assert doc["measured"][key][pair]["value"] <= bar, (key, pair)
    for pair in ("r32/r64", "oracle/r32", "oracle/r64"):
        assert doc["measured"]["diverged"][pair]["value"] <= X.MAX_DIVERGED
        assert doc["measured"]["pp_excluded"][pair]["value"] <= X.MAX_ON_INTEGER
        assert doc["measured"]["pp_mismatch"][pair]["value"] == 0


def test_prep_hook_table_is_the_stated_one():
    from oracle.refshader import prep
    assert sorted({(f, ln) for f, ln, _, _ in prep.HOOKS}) == [("raytrace.comp.glsl", n) for n in (91, 204, 256, 259, 306)]


def test_prep_wraps_every_floating_literal_and_nothing_else():
    from oracle.refshader import prep
    src = "x = 2.0 * a - 1.0f + 3 * b[2] + 0xFF + 1e-38 + v1.x + 374761393U + .5; // 2.0 stays\n/* 4.0 */ y = float[2](1, 4.0);"
    out = prep._outside_comments(src, prep._code)
    assert out == ("x = RL(2.0) * a - RLF(1.0f) + 3 * b[2] + 0xFF + RL(1e-38) + v1.x + 374761393U + RL(.5); // 2.0 stays\n"
                   "/* 4.0 */ y = {1, RL(4.0)};")


@live
def test_generated_units_differ_from_the_text_by_syntax_only():
    """every line of a generated unit that carries arithmetic is the shader's line with literals wrapped, `float` -> `Real`
    and parameter qualifiers rewritten; un-doing exactly those gives back the reference's line (hook lines excepted)"""
    ref = _reference_dir()
    if ref is None:
        pytest.skip("needs the reference tree")
    import re
    from oracle.refshader import prep
    for shader, name in (("raytrace", "raytrace"), ("temporalGradient", "temporal_gradient"), ("temporalFiltering", "temporal_filter")):
        gen = open(os.path.join(ROOT, "oracle", "_ref", name + ".gen.hpp")).read()
        undone = re.sub(r"RLF?\(([^()]*)\)", r"\1", gen).replace("Real", "float")
        undone = re.sub(r"(\w+)& (\w+)", r"\1 \2", undone)
        have = set(" ".join(ln.split()) for ln in undone.split("\n"))
        hooked = {ln for f, ln, _, _ in prep.HOOKS if f == shader + ".comp.glsl"}
        for i, line in enumerate(open(os.path.join(ref, "shaders", shader + ".comp.glsl"), errors="replace").read().split("\n"), 1):
            code = line.split("//")[0]
            if i in hooked or not re.search(r"[-+*/]|=", code) or re.match(r"\s*(#|layout|/\*|\*)", code) or "[](" in code:
                continue
            if re.search(r"\bfloat\[\d", code) or re.search(r"\b(inout|out)\b", code):
                continue  # array constructors -> braces, qualifiers -> references: covered by the prep unit test
            want = " ".join(re.sub(r"(\w+)& (\w+)", r"\1 \2", line).split())
            assert want in have, (shader, i, line)


@live
def test_r32_contains_no_double_operation(tmp_path):
    """the R32 unit is compiled with -Werror=double-promotion (oracle/Makefile); a bare `2.0` in it must be an error"""
    ref = _reference_dir()
    if ref is None:
        pytest.skip("needs the reference tree")
    env = dict(os.environ, REFOUT=str(tmp_path))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "ref", "REF=" + ref, "REFOUT=" + str(tmp_path)], env=env)
    gen = tmp_path / "raytrace.gen.hpp"
    text = gen.read_text()
    assert text.count("RL(2.0)") >= 4  # among them scalar sites such as :89 and :257
    gen.write_text(text.replace("RL(2.0)", "2.0"))
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-ffp-contract=off", "-Wdouble-promotion", "-Werror=double-promotion",
           "-DREFSHADER_REAL=float", "-DREFSHADER_SUF=f32", "-I" + os.path.join(ROOT, "oracle", "refshader"), "-I" + str(tmp_path),
           os.path.join(ROOT, "oracle", "refshader", "host.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode != 0 and "double" in p.stderr, p.stderr[-400:]


# ------------------------------------------------------------------------------------------ RNG and primary ray
@live
def test_rng_words_and_floats_bit_for_bit(oracle):
    for px, py, frame in ((0, 0, 0), (63, 47, 3), (99, 4, 1), (12345, 678, 4000000000)):
        seed = oracle.rng_seed(px, py, frame)
        words, floats, state = oracle.rng_steps(seed, 70)
        got, gstate = R.rng_floats("f32", seed, 70)
        assert gstate == state
        assert np.array_equal(bits(got), bits(np.array(floats, np.float32)))
        got64, _ = R.rng_floats("f64", seed, 70)
        assert np.array_equal(got64, np.array(words, np.float64) / 4294967296.0)  # 4294967295.0f IS 2^32


@live
def test_random_gaussian_is_the_contract_box_muller(oracle):
    """R32's randomGaussian (the text, with the contract's log / sqrt / sincos) against the same contract functions
    applied to the oracle's own draws, bit for bit; R64 (libm) within binary32 rounding of it"""
    for seed in (1, 0xDEADBEEF, oracle.rng_seed(5, 7, 2)):
        _, f, state = oracle.rng_steps(seed, 2)
        u1 = max(np.float32(1e-38), f[0])
        r = np.float32(oracle.lib().oracle_sqrt(np.float32(-2.0) * np.float32(oracle.lib().oracle_log(u1))))
        want = np.array([r * np.float32(oracle.lib().oracle_cos2pi(f[1])), r * np.float32(oracle.lib().oracle_sin2pi(f[1]))], np.float32)
        got, gstate = R.random_gaussian("f32", seed)
        assert gstate == state and np.array_equal(bits(got), bits(want)), (seed, got, want)
        got64, _ = R.random_gaussian("f64", seed)
        assert np.abs(got64 - want).max() <= 4e-6


# ------------------------------------------------------------------------------------------ path loop, in lockstep
@live
@pytest.mark.parametrize("seg", X.SEGMENTS)
@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: "%dx%d" % s)
def test_path_loop_in_lockstep(oracle, cornell, size, seg):
    _path_loop(oracle, cornell[2], size, seg, "cornell")


@live
def test_path_loop_in_lockstep_on_a_sphere(oracle, cornell):
    """normals of every direction: the three albedo branches of raytrace.comp.glsl:155-163, and paths that leave to the sky"""
    seen = _path_loop(oracle, X.sphere_scene(), (64, 48), 32, "sphere")
    assert {oracle.END_LIGHT, oracle.END_SKY} <= seen


def _path_loop(oracle, tris, size, seg, tag):
    seen = set()
    for f in X.oracle_frames(size[0], size[1], tris, seg, 1):
        obs = X.observe(f)
        _check_common(obs, f"{tag} {size} seg {seg} frame {f.pc.frameNumber}")
        tr, _ = obs["_runs"]
        for a in ("r32", "r64"):
            same = X.same_paths(tr[a]["seq_id"], tr[a]["seq_n"], f.seq_id, f.seq_n)
            # ray count: the sum of segments traced, after removing diverged pixels from both
            assert int(tr[a]["seq_n"][same].sum()) == int(f.seq_n[same].sum())
            if same.all():
                assert tr[a]["rays"] == f.rays
            # a diverged pixel agrees up to the segment where the ids first differ: its first query is the primary ray
            assert np.array_equal(tr[a]["seq_id"][..., 0], f.seq_id[..., 0]) or obs["diverged"]["oracle/" + a] > 0
            # how the path ended, where the record alone tells: a triangle hit short of the bound is the light test
            n, last = tr[a]["seq_n"], np.take_along_axis(tr[a]["seq_id"], np.maximum(tr[a]["seq_n"] - 1, 0)[..., None], -1)[..., 0]
            assert (f.seq_end[same & (n < seg) & (last != 0)] == oracle.END_LIGHT).all()
            assert np.isin(f.seq_end[same & (last == 0)], (oracle.END_SKY, oracle.END_LIGHT)).all()
            assert (n >= 1).all() and (n <= seg).all()
        # R32 against the oracle bit for bit where the path ends on the light or the segment bound: the colour is then a
        # product of the text's constants in the text's order
        same = X.same_paths(tr["r32"]["seq_id"], tr["r32"]["seq_n"], f.seq_id, f.seq_n)
        const = same & np.isin(f.seq_end, (oracle.END_LIGHT, oracle.END_BOUND))
        assert const.any()
        assert np.array_equal(bits(tr["r32"]["image"])[const], bits(f.traced)[const])
        assert (tr["r32"]["image"][..., 3] == 0).all() and np.array_equal(tr["r32"]["seq_id"][..., 0], f.hit_id)
        seen |= set(np.unique(f.seq_end).tolist())
    return seen


@live
def test_samples_per_pixel_is_an_extension(oracle, cornell):
    """raytrace.comp.glsl:200 takes rngState BY VALUE, so with NUM_SAMPLES > 1 the text replays sample 0's bounce draws and
    only the Gaussian jitter stream (drawn in main, :314) continues.  The project's samples_per_pixel > 1 carries the
    stream through the bounces instead: an extension, not the reference's behaviour.  Asserted here: what is true."""
    W, H, seg = 64, 48, 4
    f = next(iter(X.oracle_frames(W, H, cornell[2], seg, 1)))
    one = R.raytrace("f32", W, H, f.pc, f.tris, seg, 1)
    base = X.ref_raytrace("f32", f)
    assert np.array_equal(bits(one["image"]), bits(base["image"]))  # the hook at its default is the text
    four = R.raytrace("f32", W, H, f.pc, f.tris, seg, 4, want_rays=True)
    n1 = one["seq_n"]
    first = np.arange(seg * 4)[None, None, :] < n1[..., None]
    assert np.array_equal(np.where(first, four["seq_id"], 0)[..., :seg], one["seq_id"])  # sample 0 identical
    # the jitter stream continues: sample s starts at the camera with the direction of Gaussian draw s of the pixel's stream
    cam = np.array(f.pc.cameraPos[:], np.float32)
    slope = np.float32(f.cfg.fov_slope)
    for (x, y) in ((0, 0), (31, 20), (63, 47), (17, 5)):
        od = four["seq_od"][y, x][: four["seq_n"][y, x]]
        prim = od[(od[:, :3] == cam).all(-1)]
        assert len(prim) == 4
        state = oracle.rng_seed(x, y, f.pc.frameNumber)
        for s in range(4):
            g, state = R.random_gaussian("f32", state)
            c = np.array([x, y], np.float64) + 0.5 + 0.375 * g.astype(np.float64)
            d = np.array([slope * (2 * c[0] - W) / H, -slope * (2 * c[1] - H) / H, -1.0])
            assert np.abs(prim[s, 3:] - d / np.linalg.norm(d)).max() < 2e-6, (x, y, s)
    # ... and the bounce draws do not: every sample's first bounce leaves with sample 0's (theta, u), whereas the oracle
    # (and the kernel) draw fresh ones.  Both facts, so that neither side changes unnoticed.
    cfg4 = oracle.config_default(W, H)
    cfg4.max_segments, cfg4.samples_per_pixel = seg, 4
    o4 = oracle.raytrace_seq(cfg4, f.pc, f.tris)
    assert np.array_equal(o4[3][..., :seg][first[..., :seg]], one["seq_id"][first[..., :seg]])  # sample 0 agrees
    assert not np.array_equal(o4[3], four["seq_id"])  # later samples do not: spp > 1 is an extension


# ------------------------------------------------------------------------------------------ K1
@live
@pytest.mark.parametrize("scene", ("cornell", "sphere"))
def test_temporal_gradient(oracle, cornell, scene):
    for f in X.oracle_frames(64, 48, _scene(scene, cornell), 1, 1):
        obs = X.observe(f)
        _, gr = obs["_runs"]
        for pair in ("r32/r64", "oracle/r32", "oracle/r64"):
            assert obs["lambda"][pair] <= BARS["lambda"], (scene, f.pc.frameNumber, pair, obs["lambda"][pair])
        for a in ("r32", "r64"):
            g = gr[a]
            bg = f.fo.vis == 0
            assert (g[bg] == 0).all()  # :119 store-before-check cleared the host's sentinel, :131 returned
            assert np.array_equal(g[..., 0], g[..., 1], equal_nan=True) and np.array_equal(g[..., 0], g[..., 2], equal_nan=True)
            assert (g[..., 3] == 0).all()
            assert np.array_equal(np.isnan(g), np.isnan(f.fo.gradient))  # D7: 0/0 compared as NaN == NaN
        if f.pc.frameNumber in (1, 3):  # light moved / changed colour: the plane is not trivially zero
            assert np.nanmax(f.fo.gradient) > 1e-2


@live
def test_temporal_gradient_zero_over_zero(oracle, cornell):
    """both Phong colours 0 (light colour 0 in both frames): lambda = min(1, 0/0), D7"""
    f = next(iter(X.oracle_frames(16, 8, cornell[2], 1, 1)))
    f.pc.currentCameraColor[:] = (0, 0, 0)
    f.pc.previousCameraColor[:] = (0, 0, 0)
    want = oracle.temporal_gradient(f.cfg, f.pc, f.fo.vis, f.fo.worldpos, f.fo.lut, f.lut_prev)
    for a in ("f32", "f64"):
        got = X.ref_gradient(a, f)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and X.abs_err(got, want) <= BARS["lambda"]


# ------------------------------------------------------------------------------------------ K3
@live
@pytest.mark.parametrize("n_it", X.ITERATIONS)
@pytest.mark.parametrize("size", X.SIZES, ids=lambda s: "%dx%d" % s)
def test_filter_every_iteration(oracle, cornell, size, n_it):
    for f in X.oracle_frames(size[0], size[1], cornell[2], 8, 5):
        obs = X.observe(f, (n_it,))
        _noise("filtered", obs["filtered"]["r32/r64"], (size, n_it, f.pc.frameNumber))
        for pair in ("r32/r64", "oracle/r32", "oracle/r64"):
            print(size, n_it, f.pc.frameNumber, pair, obs["filtered"][pair], obs["pp_mismatch"].get(pair), obs["pp_excluded"].get(pair))
            assert obs["filtered"][pair] <= BARS["filtered"], (size, n_it, f.pc.frameNumber, pair, obs["filtered"][pair])
            if pair in obs["pp_mismatch"]:
                assert obs["pp_excluded"][pair] <= X.MAX_ON_INTEGER
                assert obs["pp_mismatch"][pair] == 0, (size, n_it, f.pc.frameNumber, pair)


@live
def test_filter_blend_history_and_frame_zero(oracle, cornell):
    W, H, n_it = 64, 48, 5
    frames = list(X.oracle_frames(W, H, cornell[2], 4, n_it))
    f0 = frames[0]
    for a in ("f32", "f64"):
        traced = f0.traced.astype(R._dt(a))
        outs, pp = X.ref_filter_chain(a, f0, traced, n_it)
        assert (pp == R.NO_LOAD).all()  # frame 0: previousFrameImage is never loaded (:251) ...
        before = X.ref_filter_chain(a, f0, traced, n_it - 1)[0][-1]
        pc = X.copy_struct(f0.pc)
        pc.waveletIteration = pc.maxWaveletIteration = n_it
        filtered, blend, _ = R.temporal_filter(a, W, H, pc, f0.ubo, before, f0.fo.depth, f0.fo.vis, f0.fo.lut, f0.lut_prev,
                                               f0.fo.worldpos, None)
        assert np.array_equal(blend, filtered) and np.array_equal(blend, outs[-1])  # ... and nothing is blended (:258)
    # history out of the image reads as 0 (D2): the first frame is drawn from inside the box, the second from further back,
    # so the walls near the opening were outside the previous view.  (z = 2.5 -> 6.0, tried first, left 0.62 % of the
    # foreground within 1e-3 px of an integer position, above the 0.5 % condition; 2.4 -> 6.0 leaves 0.04 %.)
    app = oracle.OracleApp(W, H, cornell[2], max_segments=2, iterations=n_it, camera=(-0.001, 1.0, 2.4))
    app.draw_scene()
    hist = app.history
    lut_prev = app.lut_prev
    fo = app.draw_scene(move_camera=(0.0, 0.0, 3.6))
    f = X.Frame()
    f.W, f.H, f.fo, f.pc, f.ubo, f.cfg, f.lut_prev, f.history, f.traced = W, H, fo, X.copy_struct(app.pc), X.copy_struct(app.ubo), app.cfg, lut_prev, hist, fo.traced
    o_outs, o_pp = X.oracle_filter_chain(f, fo.traced, n_it)
    outside = (o_pp[..., 0] < 0) | (o_pp[..., 0] >= W) | (o_pp[..., 1] < 0) | (o_pp[..., 1] >= H)
    assert outside.sum() > 50 and (~outside & (fo.vis > 0)).sum() > 50
    near = X.screen_pos_on_integer(f)
    for a in ("f32", "f64"):
        outs, pp = X.ref_filter_chain(a, f, fo.traced.astype(R._dt(a)), n_it)
        ok = ~near if a == "f64" else np.ones_like(near)
        assert near.sum() <= X.MAX_ON_INTEGER * (fo.vis > 0).sum()
        assert np.array_equal(pp[ok], o_pp[ok])
        assert X.colour_err(outs[-1], o_outs[-1]) <= BARS["filtered"]
        # where the history is outside, the blend is alpha * filtered + (1 - alpha) * 0: one product, so the two differ by at
        # most one binary32 rounding (6e-8 relative; 1e-6 of the largest value leaves room for nothing else)
        lit = outside & (outs[-1][..., :3].max(-1) > 0)
        plain = _unblended(a, f, fo, n_it)
        assert lit.sum() > 50
        assert np.abs(outs[-1][lit][..., :3] - np.float32(0.3) * plain[lit][..., :3]).max() <= 1e-6 * plain[lit][..., :3].max()


def _unblended(a, f, fo, n_it):
    """the same chain with maxWaveletIteration beyond n_it: no pass is the final one, nothing is blended"""
    pc = X.copy_struct(f.pc)
    cur = fo.traced.astype(R._dt(a))
    for k in range(1, n_it + 1):
        pc.waveletIteration, pc.maxWaveletIteration = k, n_it + 2
        cur, _, _ = R.temporal_filter(a, f.W, f.H, pc, f.ubo, cur, fo.depth, fo.vis, fo.lut, f.lut_prev, fo.worldpos, f.history)
    return cur


@live
def test_filter_with_nan_and_inf_pixels(oracle, cornell):
    """the traced planes of these scenes hold no NaN / Inf (asserted), so some are planted: they must spread through the
    taps the same way in the oracle and in the text (NaN stays NaN, kinds match), everything else within the bar"""
    frames = list(X.oracle_frames(64, 48, cornell[2], 4, 5))
    assert all(np.isfinite(f.traced).all() for f in frames)
    f = frames[2]
    traced = f.traced.copy()
    traced[10, 10, :3] = np.nan
    traced[30, 40, 0] = np.inf
    traced[5, 60, 1] = -np.inf
    traced[47, 0, :3] = np.nan
    for n_it in (1, 2, 5):
        want, _ = X.oracle_filter_chain(f, traced, n_it)
        assert np.isnan(want[-1]).any()
        for a in ("f32", "f64"):
            got, _ = X.ref_filter_chain(a, f, traced.astype(R._dt(a)), n_it)
            for k, (g, w) in enumerate(zip(got, want)):
                assert X.colour_err(g, w) <= BARS["filtered"], (n_it, a, k, X.colour_err(g, w))


@live
@pytest.mark.parametrize("size", ((7, 3), (1, 1)), ids=lambda s: "%dx%d" % s)
def test_filter_stride_wrap_at_the_border(oracle, cornell, size):
    """`pixel.x + i * k` with `uint k` is evaluated modulo 2^32 and converted back before the clamp (:135-136); strides far
    beyond the image on images a few pixels wide"""
    W, H = size
    f = list(X.oracle_frames(W, H, cornell[2], 2, 1))[1]
    rng = np.random.default_rng(5)
    traced = (f.traced + rng.uniform(0, 0.5, f.traced.shape).astype(np.float32)) * np.float32([1, 1, 1, 0])
    for k in (1, 2, 3, 6, 7, 255, 256):
        pc = X.copy_struct(f.pc)
        pc.waveletIteration, pc.maxWaveletIteration = k, 257
        want = oracle.atrous(f.cfg, pc, f.ubo, traced, f.fo.depth, f.fo.vis, f.fo.lut, f.lut_prev, f.fo.worldpos, f.history)
        for a in ("f32", "f64"):
            got, blend, _ = R.temporal_filter(a, W, H, pc, f.ubo, traced.astype(R._dt(a)), f.fo.depth, f.fo.vis, f.fo.lut, f.lut_prev,
                                              f.fo.worldpos, f.history)
            assert np.isnan(blend).all()  # k != maxIt: colorImage is not stored
            assert X.colour_err(got, want) <= BARS["filtered"], (size, k, a)


@live
def test_final_pass_race_is_documented_not_asserted(oracle, cornell):
    """D1: the final pass loads colorImage at neighbours and stores colorImage at its own pixel with no barrier.  The
    project (oracle and kernels) reads a pre-pass snapshot.  Run in plain serial raster order WITHOUT the snapshot, the
    reference text gives a different image: one possible outcome of the race the reference has.  Printed, not asserted."""
    f = list(X.oracle_frames(64, 48, cornell[2], 4, 1))[1]
    pc = X.copy_struct(f.pc)
    pc.waveletIteration = pc.maxWaveletIteration = 1
    args = (64, 48, pc, f.ubo, f.traced, f.fo.depth, f.fo.vis, f.fo.lut, f.lut_prev, f.fo.worldpos, f.history)
    _, snap, _ = R.temporal_filter("f32", *args)
    _, serial, _ = R.temporal_filter("f32", *args, serial_in_place=True)
    differ = (bits(snap) != bits(serial)).any(-1)
    print(f"D1: {int(differ.sum())} of {differ.size} pixels differ between the snapshot and the serial in-place order")
    assert not differ[0, 0]  # the first invocation has read nothing that was overwritten


# ------------------------------------------------------------------------------------------ whole frames
@live
def test_whole_frames(oracle, cornell):
    rows = X.whole_frames(cornell[2], **X.WHOLE)
    err = X.whole_errors(rows)
    print("whole frames", err)
    _noise("whole", err["r32/r64"], "whole frames")
    for pair in ("r32/r64", "oracle/r32", "oracle/r64"):
        assert err[pair] <= BARS["whole"], (pair, err[pair])
    for row in rows:
        f = row["f"]
        for a in ("f32", "f64"):
            assert X.abs_err(row[a]["gradient"], f.fo.gradient) <= BARS["lambda"]
            assert X.colour_err(row[a]["traced"]["image"], f.fo.traced) <= BARS["traced"]
            if f.pc.frameNumber > 0:
                ok = ~X.screen_pos_on_integer(f) if a == "f64" else np.ones(f.fo.vis.shape, bool)
                assert np.array_equal(row[a]["prev_pixel"][ok], f.fo.prev_pixel[ok])


# ------------------------------------------------------------------------------------------ the host is not vacuous
@live
@pytest.mark.parametrize("which", ("sigma_l", "pixel_jitter"))
def test_an_altered_constant_is_caught(oracle, cornell, tmp_path, which):
    """one constant of the text altered by 0.3 % / 2.5 % on its way through prep.py: the comparison it feeds must fail"""
    ref = _reference_dir()
    if ref is None:
        pytest.skip("needs the reference tree")
    mut = {"sigma_l": "REF_MUTATE_FILTER=--mutate '205:4.0:4.1'",
           "pixel_jitter": "REF_MUTATE_RAYTRACE=--mutate '314:0.375:0.376'"}[which]
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "-s", "ref", "REF=" + ref, "REFOUT=" + str(tmp_path), mut])
    path = str(tmp_path / "librefshader.so")
    f = list(X.oracle_frames(64, 48, cornell[2], 8, 5))[1]
    good, bad = X.observe(f, (5,)), X.observe(f, (5,), path=path)
    key = {"sigma_l": "filtered", "pixel_jitter": "dir0"}[which]
    for pair in ("oracle/r32", "oracle/r64"):
        assert good[key][pair] <= BARS[key] < bad[key][pair], (which, pair, good[key][pair], bad[key][pair])


# ------------------------------------------------------------------------------------------ recorded fixture
def _fixture_frames(oracle, cornell):
    meta, frames = X.load_fixture(FIXTURE)
    fs = list(X.oracle_frames(meta["W"], meta["H"], cornell[2], meta["seg"], meta["n_it"]))
    return meta, frames, fs


def test_oracle_against_the_recorded_reference_runs(oracle, cornell):
    """never skips: the reference text's recorded outputs (both arithmetics) against the oracle, same bars"""
    meta, frames, fs = _fixture_frames(oracle, cornell)
    wy, wx = X.fix_window(meta["H"], meta["W"])
    for f, fx in zip(fs, frames):
        i = f.pc.frameNumber
        assert bytes(f.pc) == fx["pc"] and bytes(f.ubo) == fx["ubo"], "the frame script no longer poses the recorded frames"
        outs, pp = X.oracle_filter_chain(f, f.traced, meta["n_it"])
        near = X.screen_pos_on_integer(f)
        for a in ("f32", "f64"):
            r = fx[a]
            same = X.same_paths(r["seq_id"], r["seq_n"].astype(np.int32), f.seq_id, f.seq_n)
            assert 1.0 - same.mean() <= X.MAX_DIVERGED
            assert np.array_equal(r["seq_id"][..., 0], f.hit_id)
            assert int(r["seq_n"][same].sum()) == int(f.seq_n[same].sum())
            assert X.colour_err(r["traced"][same], f.traced[..., :3][same]) <= BARS["traced"], (i, a)
            assert X.abs_err(r["lambda"], f.fo.gradient[..., 0]) <= BARS["lambda"], (i, a)
            assert X.colour_err(r["image"], outs[-1][..., :3]) <= BARS["filtered"], (i, a)
            if "stack" in r:
                for k, o in enumerate(outs):
                    assert X.colour_err(r["stack"][k], o[wy, wx, :3]) <= BARS["filtered"], (i, a, k)
            if i == 0:
                assert (r["prev_pixel"] == R.NO_LOAD).all()
            else:
                ok = ~near if a == "f64" else np.ones_like(near)
                assert near.sum() <= X.MAX_ON_INTEGER * (f.fo.vis > 0).sum()
                assert np.array_equal(r["prev_pixel"][ok], pp[ok]), (i, a)
        const = np.isin(f.seq_end, (oracle.END_LIGHT, oracle.END_BOUND)) & X.same_paths(fx["f32"]["seq_id"], fx["f32"]["seq_n"].astype(np.int32), f.seq_id, f.seq_n)
        assert np.array_equal(bits(fx["f32"]["traced"])[const], bits(f.traced[..., :3])[const])


@live
def test_live_library_reproduces_the_fixture(oracle, cornell):
    meta, frames, fs = _fixture_frames(oracle, cornell)
    for f, fx in zip(fs, frames):
        planes, ints = X.fixture_planes(f, meta["n_it"])
        for name, pair in planes.items():
            for a, v in zip(("f32", "f64"), pair):
                assert np.array_equal(bits(v), bits(fx[a][name])), (f.pc.frameNumber, name, a)
        for name, pair in ints.items():
            for a, v in zip(("f32", "f64"), pair):
                assert np.array_equal(v, fx[a][name]), (f.pc.frameNumber, name, a)


# ------------------------------------------------------------------------------------------ GPU: the HIP path
def _hip_frames(hip_lib, cornell, W, H, seg, n_it, flags, oracle_fs):
    """the HIP path through the C ABI on the frames the oracle posed (push constants / UBO bytes as recorded)"""
    abi = hip_lib
    cfg = abi.config_default(W, H)
    cfg.max_segments, cfg.flags = seg, flags
    with abi.Context(cfg) as ctx:
        ctx.enable_debug(abi.DEBUG_HIT_ID | abi.DEBUG_PREV_PIXEL)
        ctx.scene_upload(cornell[0], cornell[1])
        for f in oracle_fs:
            pc = abi.PushConstants.from_buffer_copy(bytes(f.pc))
            ubo = abi.Ubo.from_buffer_copy(bytes(f.ubo))
            ctx.reset_counters()
            ctx.gbuffer(ubo)
            ctx.temporal_gradient(pc)
            pc.sample_batch = 0
            ctx.raytrace(pc)
            out = dict(grad=ctx.readback(abi.PLANE_GRADIENT), traced=ctx.readback(abi.PLANE_IMAGE), hit=ctx.readback(abi.PLANE_HIT_ID),
                       rays=ctx.raycount())
            pc.maxWaveletIteration = n_it
            for k in range(1, n_it + 1):
                pc.waveletIteration = k
                ctx.temporal_filter(pc, ubo)
            out["image"] = ctx.readback(abi.PLANE_IMAGE)
            out["pp"] = ctx.readback(abi.PLANE_PREV_PIXEL)
            ctx.end_frame()
            yield f, out


def _hip_check(f, out, ref32, ref64, exact, tag):
    """ref32 / ref64: dict(seq_id, seq_n, traced[...,:3], lambda, image[...,:3], prev_pixel) — live runs or the fixture"""
    assert np.array_equal(out["hit"].reshape(f.H, f.W), ref32["seq_id"][..., 0]), tag  # first-hit ids: R32's, exactly
    traced, lam, img = out["traced"].reshape(f.H, f.W, 4), out["grad"].reshape(f.H, f.W, 4), out["image"].reshape(f.H, f.W, 4)
    same32 = X.same_paths(ref32["seq_id"], ref32["seq_n"].astype(np.int32), f.seq_id, f.seq_n)
    same64 = X.same_paths(ref64["seq_id"], ref64["seq_n"].astype(np.int32), f.seq_id, f.seq_n)
    assert 1 - same32.mean() <= X.MAX_DIVERGED and 1 - same64.mean() <= X.MAX_DIVERGED
    if same32.all():
        assert out["rays"] == int(ref32["seq_n"].sum()), tag
    assert out["rays"] - int(f.seq_n[~same32].sum()) == int(ref32["seq_n"][same32].sum()), tag
    assert X.colour_err(traced[..., :3][same64], ref64["traced"][same64]) <= BARS["traced"], tag
    assert X.colour_err(traced[..., :3][same32], ref32["traced"][same32]) <= BARS["traced"], tag
    const = same32 & np.isin(f.seq_end, (1, 3))
    assert np.array_equal(bits(traced[..., :3])[const], bits(ref32["traced"])[const]), tag
    assert X.abs_err(lam[..., 0], ref64["lambda"]) <= BARS["lambda"] and X.abs_err(lam[..., 0], ref32["lambda"]) <= BARS["lambda"], tag
    assert (lam[..., 3] == 0).all() and np.array_equal(lam[..., 0], lam[..., 1], equal_nan=True)
    for ref in (ref64, ref32):
        want = np.asarray(ref["image"], np.float64)
        err = np.abs(img[..., :3].astype(np.float64) - want)
        lim = BARS["filtered"] * np.maximum(np.abs(want), X.COLOUR_FLOOR)
        if not exact:  # the hardware-exp filter: the existing FILTER_TOL on top of the bar
            lim = lim + FILTER_TOL * (1.0 + np.linalg.norm(want, axis=-1, keepdims=True))
        print(tag, "final image: worst err / limit", float((err / lim).max()))
        assert (err <= lim).all(), (tag, float((err / lim).max()))
    if f.pc.frameNumber > 0:
        pp = out["pp"].reshape(f.H, f.W, 2)
        near = X.screen_pos_on_integer(f)
        assert near.sum() <= X.MAX_ON_INTEGER * (f.fo.vis > 0).sum()
        assert np.array_equal(pp, ref32["prev_pixel"]), tag
        assert np.array_equal(pp[~near], ref64["prev_pixel"][~near]), tag


@pytest.mark.gpu
@pytest.mark.parametrize("exact", (True, False), ids=("exact_filter", "hw_exp_filter"))
@pytest.mark.parametrize("bvh", (False, True), ids=("brute", "bvh"))
def test_hip_path_against_the_recorded_reference_runs(hip_lib, oracle, cornell, bvh, exact):
    """reads tests/golden/ only"""
    meta, frames, fs = _fixture_frames(oracle, cornell)
    flags = (hip_lib.FLAG_FORCE_BVH if bvh else 0) | (hip_lib.FLAG_EXACT_FILTER if exact else 0)
    for (f, out), fx in zip(_hip_frames(hip_lib, cornell, meta["W"], meta["H"], meta["seg"], meta["n_it"], flags, fs), frames):
        _hip_check(f, out, fx["f32"], fx["f64"], exact, f"fixture frame {f.pc.frameNumber} bvh {bvh} exact {exact}")


@pytest.mark.gpu
@live
@pytest.mark.parametrize("bvh", (False, True), ids=("brute", "bvh"))
@pytest.mark.parametrize("size", X.SIZES[1:], ids=lambda s: "%dx%d" % s)
def test_hip_path_against_the_reference_text_at_ragged_sizes(hip_lib, oracle, cornell, size, bvh):
    """reads oracle/_ref/ only (the library that was built where the reference tree is)"""
    W, H = size
    seg, n_it = 32, 5
    fs = list(X.oracle_frames(W, H, cornell[2], seg, n_it))
    for exact in (True, False):
        flags = (hip_lib.FLAG_FORCE_BVH if bvh else 0) | (hip_lib.FLAG_EXACT_FILTER if exact else 0)
        for f, out in _hip_frames(hip_lib, cornell, W, H, seg, n_it, flags, fs):
            refs = []
            for a in ("f32", "f64"):
                planes, ints = X.fixture_planes(f, n_it)
                k = 0 if a == "f32" else 1
                refs.append(dict(seq_id=ints["seq_id"][k], seq_n=ints["seq_n"][k], prev_pixel=ints["prev_pixel"][k],
                                 traced=planes["traced"][k], image=planes["image"][k], **{"lambda": planes["lambda"][k]}))
            _hip_check(f, out, refs[0], refs[1], exact, f"{W}x{H} frame {f.pc.frameNumber} bvh {bvh} exact {exact}")
