"""What tests/pathtrace_scenes.py claims about its scenes, checked on the oracle's path dump (no GPU) at the shapes
tests/test_pathtrace_scenes_gpu.py runs them at: the closed room keeps every path alive to the segment bound, the mask room's
emissive rectangles end exactly the paths of mask(), and the other scenes end paths in every way, at different segments of one
tile, with paths alive behind every window boundary (floors: half of what the oracle measured, pathtrace_scenes.MEASURED)."""
import numpy as np
import pytest

import filter_planes as FP
import gbuffer_scenes as G
import pathtrace_scenes as P

W0, H0 = P.MAIN_SHAPE


def _counts(oracle, r):
    seq_n, seq_end = r["seq_n"], r["seq_end"]
    by_end = {"light": oracle.END_LIGHT, "sky": oracle.END_SKY, "bound": oracle.END_BOUND, "emissive": oracle.END_EMISSIVE}
    out = {k: int((seq_end == v).sum()) for k, v in by_end.items()}
    out.update(tiles3=int(P.tiles_with_end_segments(seq_n)), alive4=int((seq_n > 4).sum()), alive8=int((seq_n > 8).sum()),
               self_hits=P.self_hits(r["seq_id"], seq_n))
    return out


def _checked(r, scene, tag):
    FP.check_ids(r["HIT_ID"], len(scene.tris))
    assert int(r["seq_id"].max()) <= len(scene.tris), tag
    assert not np.isnan(r["IMAGE"]).any(), tag
    assert r["rays"] == int(r["seq_n"].sum()), tag
    return r


# ------------------------------------------------------------------------------------------ forms
def test_forms_reach_the_kernels_they_are_meant_for():
    for name, form in P.MAIN_SCENES:
        s = P.scene(name, form)
        assert s.tris.dtype == np.float32 and s.tris.shape == (len(s.tris), 9) and not s.tris.flags.writeable
        assert len(s.tris) < 65536, "the dump's ids are 16 bits wide"
        if form == "small":
            assert len(s.tris) <= 64, (name, len(s.tris))
        else:
            assert len(s.tris) > 64 and P.is_all_fan_pairs(s.tris) == (form == "pairs"), (name, form)
        if s.materials is not None:
            assert len(s.tri_material) == len(s.tris) and int(s.tri_material.max()) < len(s.materials)
            kd = s.materials[:, :3]
            assert ((kd > 0) & (kd < 1)).all(), "no Kd component is 0 or 1"
    for W, H in (P.MAIN_SHAPE,) + P.EDGE_SHAPES:
        assert len(P.mask_room("small", W, H).tris) <= 64
    mats = P.mask_room("small").materials
    assert (np.log2(mats[:, :3]) % 1 == 0).all(), "powers of two: products of albedos are exact in any order"


# ------------------------------------------------------------------------------------------ 1. closed room
@pytest.mark.parametrize("segments", [9, 17])
def test_closed_room_keeps_every_path_to_the_bound(oracle, segments):
    s = P.closed_room("small")
    for W, H in (P.MAIN_SHAPE,) + P.EDGE_SHAPES:
        r = _checked(P.oracle_frame(oracle, s, W, H, segments), s, (W, H))
        assert (r["seq_n"] == segments).all() and (r["seq_end"] == oracle.END_BOUND).all(), (W, H, segments)
        assert (r["seq_id"] > 0).all() and r["rays"] == W * H * segments
    W, H, y0, y1 = P.STRIP
    r = P.oracle_frame(oracle, s, W, H, segments, rows=(y0, y1))
    assert (r["seq_n"][y0:y1] == segments).all() and r["rays"] == W * (y1 - y0) * segments
    u = P.scene("closed_room_unjittered")
    for W, H in (P.MAIN_SHAPE, P.RESIZED_SHAPE):
        assert u.jitter == 0.0 and (P.oracle_frame(oracle, u, W, H, segments)["seq_n"] == segments).all(), (W, H)


# ------------------------------------------------------------------------------------------ 2. mask room
def _mask_cases():
    W, H, y0, y1 = P.STRIP
    return [(W0, H0, None), (W, H, (y0, y1))] + [(w, h, None) for (w, h) in P.EDGE_SHAPES + (P.RESIZED_SHAPE,)]


@pytest.mark.parametrize("form", P.FORMS)
def test_mask_room_ends_exactly_the_masked_paths_at_segment_0(oracle, form):
    for W, H, rows in _mask_cases():
        s = P.scene("mask_room", form, W, H, rows)
        y0, y1 = rows or (0, H)
        r = _checked(P.oracle_frame(oracle, s, W, H, rows=rows), s, (form, W, H, rows))
        want = P.mask(W, H, y0, y1 if rows else None, tess=(form != "small"))[y0:y1]
        ended = (r["seq_n"] == 1)[y0:y1]
        assert np.array_equal(ended, want), (form, W, H, rows, np.argwhere(ended != want)[:4].tolist())
        assert (r["seq_end"][y0:y1][want] == oracle.END_EMISSIVE).all()
        assert not np.isin(r["seq_end"], (oracle.END_LIGHT, oracle.END_SKY)).any(), "the room is closed, nothing sees the light"
        # a pixel of a colour Ke exactly is one that ended at segment 0
        ke = s.materials[s.tri_material[r["HIT_ID"][y0:y1][want] - 1], 3:]
        assert np.array_equal(r["IMAGE"][y0:y1][want][:, :3], ke) and (ke > 1).all()
        others = r["IMAGE"][y0:y1][~want][:, :3]
        assert not (others[:, None, :] == s.materials[None, :, 3:]).all(-1).any(), "no other pixel has a colour Ke"


def test_mask_room_tiles_have_the_named_survivors(oracle):
    """main shape, after segment 0: a tile whose only survivor is its first pixel (wave 0, lane 0), one whose only survivor is
    its last (wave 3, lane 63), one with 255 survivors, one that lost a 16 x 4 block (a whole wave), one that lost two rows, one
    with no survivor, untouched tiles and the 2-pixel-wide partial tile; tessellated also a checkerboard and one lane per wave"""
    for form in ("small", "pairs"):
        tess = form != "small"
        s = P.mask_room(form)
        alive = P.oracle_frame(oracle, s, W0, H0)["seq_n"] > 1
        tiles = P.tile_patterns(W0, H0, tess=tess)
        seen = set()
        for (x0, y0), p in tiles.items():
            if x0 + P.TILE[0] > W0 or y0 + P.TILE[1] > H0:
                if x0 == 128 and p != "untouched":
                    seen.add("partial")
                    assert alive[y0:y0 + 4, x0:].size in (8, 2)
                continue
            t = alive[y0:y0 + 4, x0:x0 + 64]
            seen.add(p)
            if p == "only_first":
                assert t.sum() == 1 and t[0, 0]
            elif p == "only_last":
                assert t.sum() == 1 and t[3, 63]
            elif p == "all_but_one":
                assert t.sum() == 255 and not t[P.ALL_BUT_ONE_AT[1], P.ALL_BUT_ONE_AT[0]]
            elif p == "block":
                assert t.sum() == 192 and not t[:, 32:48].any()
            elif p == "two_rows":
                assert t.sum() == 128 and not t[1:3].any()
            elif p == "empty":
                assert t.sum() == 0
            elif p == "untouched":
                assert t.all()
            elif p == "checker":
                assert t.sum() == 128 and t[0, 0] and not t[0, 1] and t[1, 1]
            elif p == "one_lane":
                per_wave = [t[:, 16 * w:16 * w + 16] for w in range(4)]
                assert [int(w.sum()) for w in per_wave] == [1, 1, 1, 1]
                assert len({int(np.flatnonzero(w.ravel())[0]) for w in per_wave}) == 4, "another lane in every wave"
        assert seen == set(P.TESS_PATTERNS if tess else P.SMALL_PATTERNS) | {"partial"}, seen


def test_mask_room_edges_are_half_a_pixel_from_every_centre():
    """rectangle corners of the small form lie on pixel edges as seen from the camera: the nearest centre is 0.5 px away (at
    least 0.25 px after the corners' rounding to binary32)"""
    for W, H in (P.MAIN_SHAPE,) + P.EDGE_SHAPES:
        s = P.mask_room("small", W, H)
        v = np.asarray(s.tris[12:], np.float64).reshape(-1, 3)
        if not len(v):
            continue
        dz = s.cam[2] - v[:, 2]
        px = ((v[:, 0] - s.cam[0]) / (P.REF_SLOPE * dz) * H + W) / 2.0
        py = (-(v[:, 1] - s.cam[1]) / (P.REF_SLOPE * dz) * H + H) / 2.0
        for c in (px, py):
            assert np.abs(c - np.round(c)).max() < 0.25, (W, H)
        assert np.allclose(dz, P.MASK_DZ) and s.jitter == 0.0


# ------------------------------------------------------------------------------------------ 3 - 5. measured floors
@pytest.mark.parametrize("name,form", sorted(P.MEASURED))
def test_scenes_end_paths_in_every_way_they_claim(oracle, name, form):
    s = P.scene(name, form)
    r = _checked(P.oracle_frame(oracle, s, W0, H0), s, (name, form))
    got = _counts(oracle, r)
    print(name, form, got)
    for k, measured in P.MEASURED[name, form].items():
        assert measured > 0, "no floor may be met by nothing"
        assert got[k] >= max(1, (measured + 1) // 2), (name, form, k, got[k], measured)
    if name.startswith("three_ends"):
        assert {"light", "sky", "bound", "emissive", "tiles3", "alive4", "alive8"} <= set(P.MEASURED[name, form])
    if name.endswith(("_far", "_huge")):
        assert "self_hits" in P.MEASURED[name, form], "bounce rays start on or behind their surface there"


def test_every_main_scene_is_accounted_for():
    for key in P.MAIN_SCENES:
        assert key in P.MEASURED or key[0] in ("closed_room", "mask_room"), key


def test_edge_shapes_and_three_samples_keep_paths_alive(oracle):
    """what the GPU test's edge shapes and spp = 3 cases rely on: three_ends has paths of different length at 65 x 7, and at
    3 spp seq_n is the total over the samples"""
    s = P.three_ends("small")
    r = _checked(P.oracle_frame(oracle, s, 65, 7), s, "65x7")
    assert len(np.unique(r["seq_n"])) >= 3 and (r["seq_n"] > 4).any()
    for sc in (s, P.mask_room("small")):
        one = P.oracle_frame(oracle, sc, W0, H0)
        three = P.oracle_frame(oracle, sc, W0, H0, spp=3)
        assert three["rays"] == int(three["seq_n"].sum()) and (three["seq_n"] >= 3).all()
        assert (three["seq_n"] >= one["seq_n"] + 2).all(), "the first sample is the 1 spp path"
        assert not np.isnan(three["IMAGE"]).any()
        # paths of different length in one tile: a thread finishes a path of another pixel than the one it started on
        assert P.tiles_with_end_segments(three["seq_n"]) >= 6


@pytest.mark.parametrize("name,form", P.WINDOW_SCENES)
def test_paths_are_alive_behind_every_window_boundary(oracle, name, form):
    """the GPU test's window cases: at every max_segments of every window some path crosses each boundary (the closed room: every
    path), so no queue launch of those cases is idle"""
    s = P.scene(name, form)
    crossed = 0
    for window in P.WINDOWS:
        w = P.window_of(window, form)
        assert P.segment_values(w)[0] == w and max(P.segment_values(w)) <= 17
        for segments in P.segment_values(w):
            r = P.oracle_frame(oracle, s, W0, H0, segments)
            alive = P.alive_after(r["seq_n"], P.window_boundaries(w, segments))
            assert all(a > 0 for a in alive), (name, form, w, segments, alive)
            if (name, form) == ("closed_room", "small"):
                assert all(a == W0 * H0 for a in alive)
            crossed += len(alive)
    assert crossed >= 20
    assert P.segment_values(1) == [1, 2, 3, 4, 5, 9, 17] and P.window_boundaries(1, 17) == [1, 2, 4, 8, 16]
