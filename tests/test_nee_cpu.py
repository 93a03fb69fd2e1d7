"""The light sample of next-event estimation (csrc/light_sample.hpp) without a device: its float32 restatement, which
tests/test_nee_gpu.py holds the device function to bit for bit, is itself held to float64 on seeded cases, to Lambert's closed
form through the mean of the weight on the contract's own draws, and to what each hostile operand is for; and the entry point
is in the header, the binding and the library."""
import os
import re

import numpy as np

import contract_cases as CC
import dielectric_scenes as DS
import nee_scenes as N
import path_walker as WK
from conftest import ROOT

from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi

F32, U32 = np.float32, np.uint32
HEADER = open(os.path.join(ROOT, "include", "rtpt.h")).read()


# ------------------------------------------------------------------------------------------ the restatement against float64
def test_sample32_against_float64(oracle):
    """4,096 seeded cases under the trapezoid: the same validity, wd within 2^-20 per component, g within 2^-16 relative wherever
    float64 has both cosines >= 1/16 (a dozen binary32 roundings, each amplified at most 16 times by the cosines' cancellation:
    12 * 16 * 2^-24 < 2^-16); at most a quarter of the cases are left out of the g bar"""
    cases, which = N.seeded_cases()
    assert 0.2 < which.mean() < 0.8, "both triangles are sampled"
    got = N.sample32(oracle, cases)
    gf = got[:, :8].view(F32)
    want = N.sample64(cases)
    assert np.array_equal(gf[:, 7] != 0, want["valid"])
    assert np.array_equal(got[:, 8], want["pick"].astype(U32))
    assert np.abs(gf[:, 3:6].astype(np.float64) - want["wd"]).max() <= 2.0 ** -20
    assert np.abs(gf[:, 0:3].astype(np.float64) - want["y"]).max() <= 2.0 ** -20
    held = want["valid"] & (want["cs"] >= 1 / 16) & (want["cl"] >= 1 / 16)
    left_out = 1 - held.mean()
    rel = np.abs(gf[held, 6].astype(np.float64) - want["g"][held]) / want["g"][held]
    print(f"sample32 vs float64: {left_out:.3%} of the cases outside the g bar, max rel err of g {rel.max():.3e} (bar {2.0 ** -16:.3e})")
    assert left_out <= 0.25
    assert rel.max() <= 2.0 ** -16


def test_hostile_operands(oracle):
    """what each hostile case is for, said of the restatement tests/test_nee_gpu.py compares the device's function with"""
    cases = N.hostile_cases()
    got = N.sample32(oracle, cases)
    gf = got[:, :8].view(F32)
    L, u_l, u_a = cases[:, 18], cases[:, 15].view(F32), cases[:, 16].view(F32)
    assert (got[:, 8] < L).all(), "the pick stays inside the list"
    top = u_l == N._draw(2 ** 24 - 1)
    assert (got[top, 8] == L[top] - 1).all() and set(L[top]) == {1, 3, N.MAX_LIGHTS}, "u_l next to 1 reaches the last entry"
    assert (got[u_l == 0, 8] == 0).all()
    n_grid = 3 * 4 * 4
    assert (gf[:n_grid, 7] == 1).all() and np.isfinite(gf[:n_grid, :7]).all(), "u_a on 0 and next to 1 are ordinary samples"
    tail = gf[n_grid:]
    assert (tail[:3, 7] == 0).all(), "a light without area is never valid"
    assert (tail[4:8, 7] == 0).all(), "on the light's plane, behind the surface, facing away"
    assert tail[8, 7] == 1 and np.isfinite(tail[8, 3:6]).all(), "r2 at the smallest normal still gives a direction"
    assert tail[10, 7] == 0, "r2 = 0"
    assert u_a.min() == 0 and u_a.max() == N._draw(2 ** 24 - 1)


# ------------------------------------------------------------------------------------------ unbiasedness
_receiver = {}


def receiver_draws(oracle, W, H, frames):
    """per pixel of the receiver scene (pixel_jitter 0: one hit point per pixel): the bounce origin x, the faced normal, and g
    (0 where the sample is not valid) of frames [0, frames) — the draws of the contract's PCG stream behind the jitter's two.
    Computed once"""
    key = (W, H, frames)
    if key in _receiver:
        return _receiver[key]
    scene = N.receiver()
    cfg = N.P.configure(oracle.config_default(W, H), scene, 1, 1)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xs, ys = xs.ravel().astype(U32), ys.ravel().astype(U32)
    k = W * H
    seeds0 = np.stack([xs, ys, np.zeros(k, U32), np.zeros(k, U32)], 1)
    rng0 = oracle.contract_array(CC.fn_index("rng_seed"), np.ascontiguousarray(seeds0))[:, 0].copy()
    _, d = DS._primary(oracle, cfg, rng0, xs, ys)
    tris = np.ascontiguousarray(scene.tris, F32)
    o = np.broadcast_to(F32(scene.cam), (k, 3)).astype(F32).copy()
    ids, _, b1, b2 = WK.closest_hits(oracle, tris, o, d, float(cfg.ray_tmax))
    assert (ids >= 1).all() and (ids <= 2).all(), "every primary ray meets the receiver"
    tri = tris[ids.astype(np.int64) - 1]
    b0 = ((F32(1.0) - b1).astype(F32) - b2).astype(F32)
    pos = DS.fma(oracle, tri[:, 6:9], b2[:, None], DS.fma(oracle, tri[:, 3:6], b1[:, None], (tri[:, 0:3] * b0[:, None]).astype(F32)))
    n = DS.stored_normals(oracle, tri)
    nf = np.where((DS.dot(oracle, n, d) < 0)[:, None], n, -n).astype(F32)
    x = DS.fma(oracle, F32(cfg.ray_offset), nf, pos)
    lights = tris[2:4]
    g = np.zeros((frames, k), F32)
    for f in range(frames):
        seeds = np.stack([xs, ys, np.full(k, f, U32), np.zeros(k, U32)], 1)
        r = oracle.contract_array(CC.fn_index("rng_seed"), np.ascontiguousarray(seeds))[:, 0].copy()
        r, _ = DS._rng_next(oracle, r)
        r, _ = DS._rng_next(oracle, r)
        r, u_l = DS._rng_next(oracle, r)
        r, u_a = DS._rng_next(oracle, r)
        r, u_b = DS._rng_next(oracle, r)
        lt = lights[N.pick(u_l, np.full(k, 2))]
        s = N.sample32(oracle, N.cases_of(lt[:, 0:3], lt[:, 3:6], lt[:, 6:9], x, nf, u_l, u_a, u_b, 2))[:, :8].view(F32)
        g[f] = np.where(s[:, 7] != 0, s[:, 6], F32(0))
    out = dict(x=x, nf=nf, g=g, ids=ids)
    for a in out.values():
        a.setflags(write=False)
    _receiver[key] = out
    return out


def z_scores(samples, want):
    """(mean - want) / standard error of the mean, per column, from the column's own samples"""
    s = np.asarray(samples, np.float64)
    se = s.std(0, ddof=1) / np.sqrt(len(s))
    return (s.mean(0) - want) / se


def test_mean_of_g_is_lamberts_form_factor(oracle):
    """3,072 receiver points, the first 256 frames' draws each: the mean of g against Lambert's polygon formula for the trapezoid,
    within 5 standard errors of the point's own sample.  Deterministic: the draws are the contract's"""
    W, H = N.SIZES[0]
    r = receiver_draws(oracle, W, H, 256)
    want = N.form_factor(N.RECEIVER_LAMP, r["x"], r["nf"])
    assert (want > 1e-3).all() and (r["g"] > 0).mean() > 0.99
    z = z_scores(r["g"], want)
    print(f"unbiasedness: {W * H} points x 256 frames, max |z| {np.abs(z).max():.2f}, above 4: {(np.abs(z) > 4).sum()}")
    assert np.abs(z).max() <= 5.0
    both = np.stack([N.form_factor(N.RECEIVER_LAMP[[0, 1, 2]], r["x"], r["nf"]), N.form_factor(N.RECEIVER_LAMP[[0, 2, 3]], r["x"], r["nf"])])
    assert np.allclose(both.sum(0), want, rtol=1e-12) and 1.5 < (both[0] / both[1]).mean(), "two unequal triangles"


# ------------------------------------------------------------------------------------------ plumbing
def test_entry_points_mirror_the_header(hip_lib):
    assert re.search(r"#define\s+RTPT_ABI_VERSION\s+5\b", HEADER), "additive"
    assert abi.PLANE_COUNT == 18 and abi.K_COUNT == 12
    sym = "rtpt_selftest_light_sample"
    assert sym in abi.SYMBOLS and re.search(r"\bint\s+%s\s*\(" % sym, HEADER) and hasattr(hip_lib.load(), sym)
    assert hip_lib.load().rtpt_selftest_light_sample(None, None, None, 1) == abi.RTPT_E_INVALID
