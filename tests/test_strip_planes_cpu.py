"""What tests/strip_planes.py claims, checked on the oracle alone (no GPU, no tolerance): the reprojected pixels of every
strip land in every class the GPU test relies on, restating the previous-frame planes is what a band of valid rows means,
the band changes the result, hostile values cross strip borders, and StripPlan stores what the oracle reads."""
import numpy as np
import pytest

import filter_planes as FP
import strip_planes as SP
import test_filter_planes_gpu as TF          # planes() and oracle_run(): the whole-frame reference and its cache (no GPU in either)
from filter_planes import same_bits

MOVED = ("own", "partial", "elsewhere")      # the bands that are not the stored rows and not the frame


def _planes(oracle, ci, rank, cls="bounded"):
    """ids without the all-identical-vertex triangle: its pixels are 0 / 0 and spread by the summed reach, which with one such
    pixel in 41 leaves no finite pixel to tell a band by"""
    W, H = SP.CASES[ci][:2]
    kind, roll = SP.landing_kind(ci, rank)
    return TF.planes(oracle, SP.T_PAIR, W, H, kind, cls, finite=True, roll=roll)


def _odd(N):
    return N if N & 1 else N + 1


@pytest.mark.parametrize("ci", range(len(SP.CASES)))
def test_landings_fill_every_class(oracle, ci):
    """floors: half of what this oracle measured (strip_planes.MEASURED), at least 1; a class that can occur has a floor"""
    case = SP.CASES[ci]
    for rank in range(case[2]):
        plan = SP.plan_of(case, rank)
        s0, s1 = plan.stored
        assert (plan.own[1] - plan.own[0]) + 2 * plan.halo < plan.height or rank != 1, "the middle strip is a strip"
        p = _planes(oracle, ci, rank)
        kind, roll = SP.landing_kind(ci, rank)
        if kind.startswith("pairs"):
            ids = np.roll(FP.id_plane(kind, SP.T_PAIR, *case[:2]), roll, axis=0)      # (before without_point)
            assert FP.pairs_read(ids[s0:s1], SP.T_PAIR, kind == "pairs_h").all(), "every pair inside the stored rows"
        for how in SP.BANDS:
            rows = SP.band(plan, how)
            assert 0 <= rows[0] < rows[1] <= plan.height
            got = SP.landing_counts(p["landing"], plan, rows)
            floors = SP.MEASURED[ci, rank, how]
            assert set(floors) == {c for c in SP.CLASSES if SP.possible(plan, rows, c)}, (ci, rank, how)
            for c, m in floors.items():
                assert m > 0 and got[c] >= max(1, (m + 1) // 2), (ci, rank, how, c, got[c], m)
        e = SP.band(plan, "elsewhere")
        assert e[1] <= s0 or e[0] >= s1, "disjoint from the stored rows"


def _blend_with_black(filtered, alpha):
    """temporal_blend(filtered, 0, alpha) = fma(filtered, alpha, 0 * (1 - alpha)): the product is exact in binary64, the
    sum with +0 too, one rounding to binary32"""
    out = np.array(filtered)
    with np.errstate(invalid="ignore", over="ignore"):
        out[..., :3] = (filtered[..., :3].astype(np.float64) * np.float64(np.float32(alpha)) + 0.0).astype(np.float32)
    return out


@pytest.mark.parametrize("ext,ci", [(0, 1), (0, 0), (0x80, 6), (0x100, 7)])
def test_the_restatement_is_what_a_band_means(oracle, ext, ci):
    case = SP.CASES[ci]
    N = _odd(case[3])
    for rank in range(case[2]):
        plan = SP.plan_of(case, rank)
        p = _planes(oracle, ci, rank)
        H, W = p["H"], p["W"]
        whole = TF.oracle_run(oracle, p, ext, N, 1)
        frame0 = TF.oracle_run(oracle, p, ext, N, 0)            # blend = filtered; moments (lum, lum^2, 1)
        px, py = p["landing"][..., 0], p["landing"][..., 1]
        in_frame = (px >= 0) & (px < W) & (py >= 0) & (py < H)
        for how in MOVED:
            rows = SP.band(plan, how)
            got = TF.oracle_run(oracle, SP.restate_prev(p, rows), ext, N, 1)
            inside = in_frame & (py >= rows[0]) & (py < rows[1])
            assert inside.any() and (~inside).any() and (in_frame & ~inside).any()
            tag = (hex(ext), ci, rank, how)
            if ext & 0x100:
                # (the image is guided by the neighbours' variance, so only the moments are a per-pixel statement)
                same_bits(got["moments"][~inside], frame0["moments"][~inside], tag + ("no-history moments",))
                same_bits(got["moments"][inside], whole["moments"][inside], tag + ("moments inside",))
                assert (got["moments"][~inside][:, 2] == 1).all()
                continue
            want = frame0["image"] if ext & 0x80 else _blend_with_black(frame0["image"], oracle.config_default(W, H).alpha)
            same_bits(got["image"][~inside], want[~inside], tag + ("outside the band",))
            same_bits(got["image"][inside], whole["image"][inside], tag + ("inside the band",))
            same_bits(got["prev_pixel"], whole["prev_pixel"], tag + ("landings do not depend on the band",))


@pytest.mark.parametrize("ext,ci", [(0, 0), (0, 1), (0, 3), (0x80, 6), (0x100, 7), (0x9F0, 8)])
def test_the_band_matters(oracle, ext, ci):
    case = SP.CASES[ci]
    N = _odd(case[3])
    for rank in range(case[2]):
        plan = SP.plan_of(case, rank)
        o0, o1 = plan.own
        p = _planes(oracle, ci, rank)
        whole = TF.oracle_run(oracle, p, ext, N, 1)
        assert np.isfinite(whole["image"][o0:o1]).mean() > 0.9, "a reference of NaNs would tell nothing"
        for how in MOVED:
            got = TF.oracle_run(oracle, SP.restate_prev(p, SP.band(plan, how)), ext, N, 1)
            a, b = got["image"][o0:o1], whole["image"][o0:o1]
            differ = (a != b) & ~(np.isnan(a) & np.isnan(b))
            assert differ.any(), (hex(ext), ci, rank, how)
            if ext & 0x100:
                assert not np.array_equal(got["moments"][o0:o1], whole["moments"][o0:o1]), (hex(ext), ci, rank, how)


@pytest.mark.parametrize("ci,ranks", [(0, (0, 1)), (1, (0, 1)), (3, (0,))])
def test_hostile_values_cross_strip_borders(oracle, ci, ranks):
    """planted class: take the planted NaN / Inf out of the rows a rank does not own, and non-finite pixels of its owned rows
    turn finite — they came from another rank's rows.  (The ranks named are those with a planted pixel of a neighbour
    within the summed reach of their border; planted_positions puts them at rows 0, H / 3, H / 2, 2 H / 3 and H - 1.)"""
    case = SP.CASES[ci]
    N = case[3]
    for rank in ranks:
        plan = SP.plan_of(case, rank)
        o0, o1 = plan.own
        p = _planes(oracle, ci, rank, "planted")
        ref = TF.oracle_run(oracle, p, 0, N, 0)["image"]
        q = dict(p, key=p["key"] + ("plants of rank", rank), img=np.array(p["img"]), depth=np.array(p["depth"]))
        moved = 0
        for (y, x, v) in FP.planted_positions(p["ids"], p["nt"]):
            if not (o0 <= y < o1):
                q["img"][y, x, :3] = np.where(np.isfinite(q["img"][y, x, :3]), q["img"][y, x, :3], np.float32(1.0))
                if not np.isfinite(q["depth"][y, x]):
                    q["depth"][y, x] = np.float32(1.0)
                moved += 1
        own_only = TF.oracle_run(oracle, q, 0, N, 0)["image"]
        bad, bad_own = ~np.isfinite(ref[o0:o1, :, :3]).all(-1), ~np.isfinite(own_only[o0:o1, :, :3]).all(-1)
        assert moved and (bad & ~bad_own).any(), (ci, rank, int(bad.sum()), int(bad_own.sum()))


def _reach(ext, k):
    """restated from temporalFiltering.comp.glsl:132-135 and include/rtpt.h, not from StripPlan: taps i, j in [-R, R] at
    `stride` pixels; R = 2 with RTPT_FLAG_EXT_GAUSS5, stride 2^(k-1) with RTPT_FLAG_EXT_POW2_STRIDE, else k"""
    return (2 if ext & 0x20 else 1) * (2 ** (k - 1) if ext & 0x40 else k)


@pytest.mark.parametrize("mode", ["redundant", "exchange"])
def test_the_plan_stores_what_the_oracle_reads(mode):
    """iteration k over filter_rows(k) reads those rows +- its reach, clamped to the frame (:136); at k = 1 with
    RTPT_FLAG_EXT_SVGF_VARIANCE the variance of every row read comes from traced rows 3 further out.  All of it lies inside
    the stored rows — rtpt_temporal_filter refuses a missing halo, so a plan that stored too little would only show as an
    error, and one that filtered too little as wrong pixels nobody could place.  Redundant mode: what iteration k reads,
    iteration k - 1 produced."""
    for case in SP.CASES:
        W, H, world, N, _, ext, splits = case
        for rank in range(world):
            plan = SP.plan_of(case, rank, mode)
            s0, s1 = plan.stored
            assert 0 <= s0 <= plan.own[0] < plan.own[1] <= s1 <= H
            for k in range(1, N + 1):
                f0, f1 = plan.filter_rows(k)
                assert f0 <= plan.own[0] and f1 >= plan.own[1]
                r = _reach(ext, k) + (3 if k == 1 and (ext & 0x900) == 0x900 else 0)
                lo, hi = max(0, f0 - r), min(H, f1 + r)
                assert s0 <= lo and hi <= s1, (case, rank, mode, k, (lo, hi), (s0, s1))
                if mode == "redundant" and k > 1:
                    p0, p1 = plan.filter_rows(k - 1)
                    assert p0 <= max(0, f0 - _reach(ext, k)) and min(H, f1 + _reach(ext, k)) <= p1, (case, rank, k)
                if mode == "exchange":
                    got = sorted(rows for _, _, rows in plan.exchange_rows(k))
                    want = sorted(x for x in ((lo, f0), (f1, hi)) if x[1] > x[0])
                    assert got == want, (case, rank, k, got, want)
            assert plan.filter_rows(N) == plan.own
