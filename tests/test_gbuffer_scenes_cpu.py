"""What tests/gbuffer_scenes.py claims about its generators, checked on the oracle (no GPU): the cull scenes exercise the
screen-bound culling (every pixel hits, dozens of ids in the frame, a few per 16 x 4 block, the named members are where their
rule applies), the K1 plane sets are not saturated, and the oracle's K1 agrees with a float64 restatement of the shader."""
import numpy as np
import pytest

import filter_planes as FP
import gbuffer_scenes as G

EYE = np.eye(4, dtype=np.float32).ravel()
# largest |oracle - float64 restatement| measured over the well-conditioned K1 sets of every shape: 1.17e-5 (130 x 33, perturbed
# previous LUT).  The bar is eight times that, rounded up to a power of two; it has to stay below 1e-3.
K1_FLOAT64_BAR = 2.0 ** -13


def _gbuffer(oracle, tris, cam, W, H):
    ubo = oracle.Ubo()
    ubo.model[:] = EYE
    ubo.view[:], ubo.proj[:] = G.k0_camera(oracle, cam, W, H)
    return oracle.gbuffer(oracle.config_default(W, H), tris, ubo)


def _block_counts(vis):
    H, W = vis.shape
    bw, bh = G.BLOCK
    return [len(np.unique(vis[y:y + bh, x:x + bw])) for y in range(0, H, bh) for x in range(0, W, bw)]


# ------------------------------------------------------------------------------------------ cull scenes
@pytest.mark.parametrize("T", [40, 63, 64])
def test_main_cull_cases_exercise_the_culling(oracle, T):
    W, H = G.MAIN_SHAPE
    tris = G.cull_scene(T)
    seen = set()
    for cam in G.MAIN_CAMERAS:
        vis, _, _ = _gbuffer(oracle, tris, cam, W, H)
        assert (vis > 0).all(), (T, cam, "the backdrop fills the frame")
        ids = set(np.unique(vis).tolist())
        assert len(ids) >= 20, (T, cam, len(ids))
        assert np.median(_block_counts(vis)) <= T / 4.0, (T, cam)
        seen |= ids
    for name_id in range(1, G.N_NAMED + 1):
        if name_id in seen:
            continue
        t = np.asarray(tris[name_id - 1], np.float64).reshape(3, 3)
        if name_id in G.ZERO_AREA_IDS:
            # neither: no ray can be asked to hit a triangle without area (its cross product is 0 or rounding residue)
            assert np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) == 0.0, name_id
            continue
        for cam in G.MAIN_CAMERAS:
            assert (G.view_space(cam, t)[:, 2] > 0).all(), (name_id, cam, "neither visible nor behind the camera")
    # where the rules of screen_bounds are met: the camera at EYE0
    vis, _, _ = _gbuffer(oracle, tris, "outside", W, H)
    for name_id in (G.ID_BACKDROP_A, G.ID_BACKDROP_B, G.ID_STRADDLE, G.ID_NEAR_BOUNDED, G.ID_NEAR_UNBOUNDED, G.ID_SLIVER, G.ID_CLOSE,
                    G.ID_BOUNDARY):
        assert (vis == name_id).any(), (T, name_id, "in view from EYE0")
    assert not (vis == G.ID_BEHIND).any()


def test_named_members_meet_their_rule():
    tris = np.asarray(G.cull_scene(40), np.float64).reshape(-1, 3, 3)
    W, H = G.MAIN_SHAPE
    p00, p11 = G.proj_scale(W, H)

    def in_front(v):     # screen_bounds' rule for one vertex, from EYE0
        r = G.view_space("outside", v)
        return -r[..., 2] > G.NEAR_RULE * (np.linalg.norm(r, axis=-1) + 1.0), r

    def pixels(r):
        return np.stack([(p00 * r[..., 0] / -r[..., 2] + 1.0) * 0.5 * W, (p11 * r[..., 1] / -r[..., 2] + 1.0) * 0.5 * H], -1)

    ok, r = in_front(tris[G.ID_STRADDLE - 1])
    assert ok.tolist() == [True, True, False] and r[2, 2] > 0.5
    assert not in_front(tris[G.ID_BEHIND - 1])[0].any()
    ok, r = in_front(tris[G.ID_NEAR_BOUNDED - 1])
    assert ok.all() and -r[0, 2] < 1.1 * G.NEAR_RULE * (np.linalg.norm(r[0]) + 1.0)
    assert np.abs(pixels(r)).max() > 32000, "its finite rectangle clamps as well"
    ok, r = in_front(tris[G.ID_NEAR_UNBOUNDED - 1])
    assert ok.tolist() == [False, True, True] and -r[0, 2] > 0 and -r[0, 2] > 0.9 * G.NEAR_RULE * (np.linalg.norm(r[0]) + 1.0)
    ok, r = in_front(tris[G.ID_CLOSE - 1])
    px = pixels(r)
    assert ok.all() and px[:, 0].min() < -32000 and px[:, 0].max() > 32000
    ok, r = in_front(tris[G.ID_SLIVER - 1])
    px = pixels(r)
    assert ok.all() and np.ptp(px[:, 0]) > 0.9 * W and np.ptp(px[:, 1]) > 0.8 * H
    ok, r = in_front(tris[G.ID_BOUNDARY - 1])
    px = pixels(r)
    assert ok.all() and np.abs(px[0] - G.BOUNDARY_PIXEL).max() < 1e-4 and (px[1:] > px[0]).all()
    assert G.BOUNDARY_PIXEL[0] % G.BLOCK[0] == 0 and G.BOUNDARY_PIXEL[1] % G.BLOCK[1] == 0
    small = tris[G.N_NAMED:]
    edges = np.linalg.norm(small - np.roll(small, 1, axis=1), axis=-1)
    assert edges.min() > 0.02 * G.EXTENT and edges.max() < 0.3 * G.EXTENT


def test_scene_list():
    counts = []
    for kind in G.SCENES:
        tris = G.scene(kind)
        counts.append(len(tris))
        assert tris.dtype == np.float32 and tris.shape == (len(tris), 9) and len(tris) <= 64
        assert G.is_all_fan_pairs(tris) == (kind[0] == "fan"), kind
    assert set(G.T_VALUES) <= set(counts) and 41 in counts
    assert len(G.K2_CAMERAS) == 9 and {(s, j) for _, s, j in G.K2_CAMERAS} == {(s, j) for s in G.K2_SLOPES for j in G.K2_JITTERS}


# ------------------------------------------------------------------------------------------ K1
def _k1(oracle, W, H, wcls, lcls, pcls):
    T = G.K1_T
    soup = FP.soup(T)
    lut = oracle.lut(soup, EYE)
    ids = np.array(G.k1_ids(T, W, H))
    wp = G.k1_worldpos(wcls, soup, ids)
    lut_prev = G.k1_lut_prev(lcls, soup)
    vals = G.k1_push_constants(pcls, ids, wp)
    pc = G.fill_push_constants(oracle.PushConstants(), vals)
    grad = oracle.temporal_gradient(oracle.config_default(W, H), pc, FP.check_ids(ids, T), wp, lut, lut_prev)
    assert np.array_equal(grad[..., 0], grad[..., 1]) and np.array_equal(grad[..., 0], grad[..., 2]) and not grad[..., 3].any()
    return ids, wp, lut, lut_prev, vals, grad[..., 0]


def test_lut_numpy_is_the_oracles_lut(oracle):
    soup = FP.soup(G.K1_T)
    assert oracle.lut(soup, EYE).tobytes() == G.lut_numpy(soup).tobytes()


@pytest.mark.parametrize("wcls", G.WP_CLASSES)
def test_k1_oracle_stays_in_the_unit_interval(oracle, wcls):
    """every class of world position x previous LUT x push constants, every shape: no NaN, nothing outside [0, 1]"""
    for (W, H) in G.SHAPES:
        for lcls in G.LUT_PREV_CLASSES:
            for pcls in G.PC_CLASSES:
                ids, _, _, _, _, lam = _k1(oracle, W, H, wcls, lcls, pcls)
                assert not np.isnan(lam).any() and lam.min() >= 0.0 and lam.max() <= 1.0, (W, H, wcls, lcls, pcls)
                assert not lam[ids == 0].any()
                if wcls == "huge":
                    assert (lam[ids > 0] == 1.0).all(), "positions of 1e18 saturate"
                if pcls == "both_black":
                    assert (lam[ids > 0] == 1.0).all(), "0 / 0 is 1 by the contract's min"


@pytest.mark.parametrize("lcls", ["equal", "perturbed"])
def test_k1_well_conditioned_sets_are_not_saturated_and_agree_with_float64(oracle, lcls):
    worst, inside, total = 0.0, 0, 0
    for (W, H) in G.SHAPES:
        ids, wp, lut, lut_prev, vals, lam = _k1(oracle, W, H, "on", lcls, "moved")
        good = (ids > 0) & ~np.isin(ids, G.DEGENERATE_IDS)
        inside += int(((lam > 0) & (lam < 1))[good].sum())
        total += int(good.sum())
        ref = G.gradient_numpy(ids, wp, lut, lut_prev, vals)
        sat = np.isnan(ref) | (ref >= 1.0)
        assert (lam[good & sat] == 1.0).all()
        diff = np.abs(lam.astype(np.float64) - ref)[good & ~sat]
        if diff.size:
            worst = max(worst, float(diff.max()))
    print(f"K1 oracle against float64, lut_prev {lcls}: largest difference {worst:.3e}, {inside} of {total} values inside (0, 1)")
    assert inside >= 0.9 * total
    assert K1_FLOAT64_BAR < 1e-3 and worst <= K1_FLOAT64_BAR, worst
