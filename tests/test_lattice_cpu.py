"""The walker (tests/path_walker.py) held on the CPU over the whole lattice before tests/test_lattice_gpu.py judges a GPU frame by it.  All
comparisons are bit for bit (filter_planes.same_bits) unless a bar is named:

  1. against the C oracle (oracle_raytrace_ext) on the scenes of tests/shading_scenes.py — SPEC 0 and 1, no glass, no list — IMAGE,
     HIT_ID, ALBEDO and the ray count for TEX 0 / 1 / 2, DEMOD off / on, forms small and odd, budgets 1, 2 and 9, three samples at
     budgets 1 and 2, a chain no box filter made, and a strip: the restatement of the mip level and of the ALBEDO plane is the
     oracle's, and the t it takes from oracle_closest_hit is the t the oracle's level takes;
  2. against the recorded frames of the older walkers (tests/golden/walker_frames.npz, IMAGE by its SHA-256): with level-0 textures
     and DEMOD off it is nee_power.walk_nee_power for every combination of sphere and power; with an empty list and the sphere off
     it is dielectric_scenes.walk;
  3. against float64: every recorded hit of the new scenes (tests/lattice_scenes.py) at 9 segments, its level replayed from the
     record's own ray by texture_mip_scenes.lod_of_rays, with the bar and the exclusions of
     test_shading_ext_cpu.test_recorded_hits_against_float64; hits behind the first glass hit are reported separately;
  4. what the scenes exercise (lattice_scenes.MEASURED), so that a scene that stops exercising something fails here first.

The estimator check of the composition (the mean over frames 0 .. 8191 of IMAGE x ALBEDO against the samplers-off walker, the N of
the test_nee_*_cpu.py tests) is left out: at about 0.05 s a walker frame, 2 x 8192 frames take ten minutes, not well under one."""
import numpy as np
import pytest

import dielectric_scenes as DS
import path_walker as WK
import lattice_scenes as LS
import nee_power as PW
import pathtrace_scenes as P
import shading_scenes as SS
import texture_mip_scenes as MS
from conftest import bits
from filter_planes import same_bits

W0, H0 = LS.SHAPES[0]


def same_frame(got, want, tag, demod=False):
    same_bits(got["HIT_ID"], want["HIT_ID"], tag + ("HIT_ID",))
    if "IMAGE" in want:
        same_bits(got["IMAGE"], want["IMAGE"], tag + ("IMAGE",))
    else:
        assert WK.same_image(got, want), tag + ("IMAGE", "SHA-256")
    if demod:
        same_bits(got["ALBEDO"], want["ALBEDO"], tag + ("ALBEDO",))
    assert got["rays"] == want["rays"], tag + ("rays", got["rays"], want["rays"])


# ------------------------------------------------------------------------------------------ 1. against the C oracle
@pytest.mark.parametrize("form", ["small", "odd"])
@pytest.mark.parametrize("name", SS.SCENES)
def test_walker_equals_the_oracle(oracle, name, form):
    sh = SS.world(oracle, SS.scene(name, form))
    rec = DS.records(sh.scene, sh.spec)
    for tex in (0, 1, 2):
        tx = WK.textures(sh, tex)
        for segments, spp, demod in [(s, 1, d) for s in (1, 2, SS.SEGMENTS) for d in (False, True)] + [(1, 3, False), (2, 3, False)]:
            tag = (name, form, tex, segments, spp, demod)
            ref = SS.oracle_frame(oracle, sh, W0, H0, segments, spp, tex, True, demod, records=False)
            got = WK.walk(oracle, sh.scene, W0, H0, segments, rec, spp=spp, tex=tx, demod=demod)
            same_frame(got, ref, tag, demod)
            if spp == 1:
                assert np.array_equal(got["seq_n"], ref["seq_n"]), tag
    if name == "glossy_textured_room":
        W, H = SS.SHAPES[1]
        for demod in (False, True):
            same_frame(WK.walk(oracle, sh.scene, W, H, SS.SEGMENTS, rec, tex=WK.textures(sh, 2), demod=demod),
                       SS.oracle_frame(oracle, sh, W, H, demod=demod, records=False), (name, form, W, H, demod), demod)


def test_walker_reads_a_given_chain_and_walks_a_strip(oracle):
    """a chain no box filter made (every level random), and rows [5, 21) of 130 x 33: segment 0's footprint takes the FULL frame's height"""
    sh = SS.scene("glossy_textured_room", "small")
    rec = DS.records(sh.scene, sh.spec)
    chains = SS.random_chains(sh)
    for demod in (False, True):
        ref = SS.oracle_frame(oracle, sh, W0, H0, demod=demod, textures=SS.given_atlas(sh, chains), records=False)
        got = WK.walk(oracle, sh.scene, W0, H0, SS.SEGMENTS, rec, tex=WK.textures(sh, 2, chains), demod=demod)
        same_frame(got, ref, ("given", demod), demod)
        generated = WK.walk(oracle, sh.scene, W0, H0, SS.SEGMENTS, rec, tex=WK.textures(sh, 2), demod=demod)
        assert not np.array_equal(bits(got["IMAGE"]), bits(generated["IMAGE"]))
    W, H, y0, y1 = P.STRIP
    for demod in (False, True):
        ref = SS.oracle_frame(oracle, sh, W, H, demod=demod, rows=(y0, y1), records=False)
        got = WK.walk(oracle, sh.scene, W, H, SS.SEGMENTS, rec, tex=WK.textures(sh, 2), demod=demod, rows=(y0, y1))
        for plane in ("IMAGE", "HIT_ID") + (("ALBEDO",) if demod else ()):
            same_bits(got[plane][y0:y1], ref[plane][y0:y1], ("strip", demod, plane))
        assert got["rays"] == ref["rays"]


# ------------------------------------------------------------------------------------------ 2. against the older walkers
OLD_COUNTS = ("rays", "samples", "queries", "lit", "kept", "dropped", "sphere_samples", "sphere_taken", "sphere_valid", "sphere_dropped", "sphere_kept")


@pytest.mark.parametrize("form", ["small", "odd"])
@pytest.mark.parametrize("name", LS.SCENES)
def test_walker_equals_the_older_walkers_at_level_0(oracle, name, form):
    c = LS.case(oracle, name, form)
    sc = c.sh.scene
    s = LS.setup(oracle, c, 6)
    rec, lights = s["rec"], s["lights"]
    level0 = WK.textures(c.sh, 1)
    assert level0.chains is None and len(lights) > 0
    for segments, spp in ((2, 1), (LS.SEGMENTS, 1), (2, 3)):
        for tx in (None, level0):
            for sphere in (False, True):
                for power in (False, True):
                    tag = (name, form, segments, spp, tx is not None, sphere, power)
                    want = WK.recorded("lattice/PW", *tag)      # walk_nee_power's, with the level-0 tuple (tri_uv, tri_texture, desc, texels)
                    got = WK.walk(oracle, sc, W0, H0, segments, rec, lights, sphere=sphere, power=power, spp=spp, tex=tx)
                    same_frame(got, want, tag)
                    assert all(got[k] == want[k] for k in OLD_COUNTS) and np.array_equal(got["picks"], want["picks"]), tag
        tag = (name, form, segments, spp, "no list")
        same_frame(WK.walk(oracle, sc, W0, H0, segments, rec, spp=spp), WK.recorded("lattice/DS", *tag), tag)
    # a mixed atlas whose flagged textures hold one value per channel at every level: any level reads what level 0 reads
    flat = c.sh._replace(images=tuple(np.broadcast_to(im[:1, :1], im.shape).copy() for im in c.sh.images))
    a = WK.walk(oracle, sc, W0, H0, LS.SEGMENTS, rec, lights, sphere=True, power=True, tex=WK.textures(flat, 2))
    b = WK.walk(oracle, sc, W0, H0, LS.SEGMENTS, rec, lights, sphere=True, power=True, tex=WK.textures(flat, 1))
    same_frame(a, b, (name, form, "constant images"))
    assert a["lod_levels"] >= 3 and a["lod_fraction"] > 0, "levels were chosen"


# ------------------------------------------------------------------------------------------ 3. against float64
@pytest.mark.parametrize("form", P.FORMS)
@pytest.mark.parametrize("name", LS.SCENES)
def test_recorded_hits_against_float64(oracle, name, form):
    """the level of every recorded hit of a 9-segment frame with every sampler on (SPEC 6), replayed in float64 from the record's
    own ray — behind or inside glass that is the refracted ray: within MS.BAR of MS.lod_of_rays wherever the float64 level is not
    within MS.BAR of a clamp, the uv triangle has area and float64 names the same triangle; next to a clamp within 2 MS.BAR.
    Conditions, not measurements: id agreement above 0.995, at least 300 judged levels, at least 100 of them behind glass"""
    c = LS.case(oracle, name, form)
    sh, sc = c.sh, c.sh.scene
    hits = []
    WK.walk(oracle, sc, W0, H0, LS.SEGMENTS, tex=WK.textures(sh, 2), hits=hits, **LS.setup(oracle, c, 6))
    h = WK.hit_table(hits)
    tris = MS.posed(sh.mesh[0], sh.mesh[1], sh.xforms) if sh.mesh else np.asarray(sc.tris, np.float64).reshape(-1, 3, 3)
    assert np.abs(tris - np.asarray(sc.tris, np.float64).reshape(-1, 3, 3)).max() < 1e-5
    rays = np.concatenate([h["o"], h["d"]], 1).astype(np.float64)
    dims = [(im.shape[1], im.shape[0]) for im in sh.images]
    levels = [len(MS.chain_dims(*d)) if f & MS.MIPMAP else 1 for d, f in zip(dims, sh.tex_flags)]
    ids, want = np.zeros(len(rays), np.int64), np.zeros(len(rays))
    for primary, spread in ((True, MS.primary_spread(sc.slope, H0)), (False, MS.BOUNCE_SPREAD)):
        m = (h["seg"] == 0) == primary
        with np.errstate(invalid="ignore"):      # the emitter without area has no determinant
            ids[m], want[m] = MS.lod_of_rays(rays[m], tris, sh.tri_uv, sh.tri_texture, dims, levels, spread)
    same = ids == h["id"]
    assert same.mean() > 0.995, (name, form, same.mean())
    rec = (h["id"] - 1) % SS.n_base(sh)
    tex = sh.tri_texture[rec].astype(np.int64)
    assert np.array_equal(tex > 0, h["textured"])
    top = np.array([l - 1.0 for l in levels] + [0.0])[tex - 1]
    assert np.array_equal((tex > 0) & (top > 0), h["mipped"])
    uv6 = sh.tri_uv[rec].astype(np.float64)
    area = np.abs((uv6[:, 2] - uv6[:, 0]) * (uv6[:, 5] - uv6[:, 1]) - (uv6[:, 4] - uv6[:, 0]) * (uv6[:, 3] - uv6[:, 1]))
    judged = same & (tex > 0) & (top > 0) & (want > MS.BAR) & (want < top - MS.BAR) & (area > 1e-6)
    err = np.abs(h["lod"] - want)
    behind = judged & h["behind"]
    print(f"{name} {form}: {judged.sum()} levels judged of {int((same & (tex > 0)).sum())} textured hits, max error {err[judged].max():.3e}; "
          f"behind glass {behind.sum()} judged, max error {err[behind].max():.3e} (bar {MS.BAR:.3e}); id agreement {same.mean():.4f}")
    assert judged.sum() >= 300 and behind.sum() >= 100
    assert err[judged].max() <= MS.BAR
    clamped = same & (tex > 0) & ~judged
    assert (err[clamped] <= 2 * MS.BAR).all(), "next to a clamp both sides are within the bar of it"
    assert (h["lod"][~h["mipped"]] == 0).all()


# ------------------------------------------------------------------------------------------ 4. what the scenes exercise
@pytest.mark.parametrize("form", P.FORMS)
@pytest.mark.parametrize("name", LS.SCENES)
def test_scenes_exercise_what_they_claim(oracle, name, form):
    c = LS.case(oracle, name, form)
    sh, sc = c.sh, c.sh.scene
    assert sc.tris.dtype == np.float32 and not sc.tris.flags.writeable
    if form == "small":
        assert len(sc.tris) <= 64
    else:
        assert len(sc.tris) > 64 and P.is_all_fan_pairs(sc.tris) == (form == "pairs")
    assert len(sh.tri_uv) == len(sh.tri_texture) == len(sc.tri_material) == SS.n_base(sh)
    assert len(sc.tris) == SS.n_base(sh) * LS.n_instances(c)
    got = LS.measure(oracle, name, form)
    print((name, form), got)
    measured = LS.MEASURED[name, form]
    assert set(LS.REQUIRED) == set(measured), "every precondition has a recorded count"
    for k, m in measured.items():
        assert m > 0, "no floor may be met by nothing"
        assert got[k] >= max(1, (m + 1) // 2), (name, form, k, got[k], m)
    assert got["lod_levels_behind"] >= LS.MIN_LEVELS_BEHIND
    # two emitters of unequal weight, so that the weighted pick is not the uniform one
    w = np.unique(PW.counted(PW.weights(oracle, sc.tris, LS.setup(oracle, c, 5)["rec"], LS.setup(oracle, c, 5)["lights"])))
    assert len(w) >= 3 and w[0] == 0
    # the frames of the six SPEC values differ pairwise, and real mips differ from level 0
    tex = WK.textures(sh, 2)
    frames = {s: WK.walk(oracle, sc, W0, H0, LS.SEGMENTS, tex=tex, **LS.setup(oracle, c, s)) for s in LS.SPECS}
    for i, a in enumerate(LS.SPECS):
        assert not np.isnan(frames[a]["IMAGE"]).any()
        for b in LS.SPECS[i + 1:]:
            assert not np.array_equal(bits(frames[a]["IMAGE"]), bits(frames[b]["IMAGE"])), (a, b)
    for s in (2, 6, "4-without-list"):
        level0 = WK.walk(oracle, sc, W0, H0, LS.SEGMENTS, tex=WK.textures(sh, 1), **LS.setup(oracle, c, s))
        assert not np.array_equal(bits(frames[s]["IMAGE"]), bits(level0["IMAGE"])), s
        plain = WK.walk(oracle, sc, W0, H0, LS.SEGMENTS, **LS.setup(oracle, c, s))
        assert not np.array_equal(bits(level0["IMAGE"]), bits(plain["IMAGE"])), s
    # the ALBEDO plane holds texels, ones where a path ends at segment 0, and the demodulated image is another image
    d = WK.walk(oracle, sc, W0, H0, LS.SEGMENTS, tex=tex, demod=True, **LS.setup(oracle, c, 6))
    ended = (d["ALBEDO"][..., :3] == 1).all(-1)
    assert 0 < ended.sum() < ended.size and not d["ALBEDO"][..., 3].any()
    assert len(np.unique(bits(d["ALBEDO"][..., :3]).reshape(-1, 3), axis=0)) > 100
    same_bits(d["IMAGE"][ended], frames[6]["IMAGE"][ended], (name, form, "ended at segment 0"))
    assert not np.array_equal(bits(d["IMAGE"]), bits(frames[6]["IMAGE"]))
    same_bits(d["HIT_ID"], frames[6]["HIT_ID"], (name, form, "HIT_ID"))
    assert d["rays"] == frames[6]["rays"]
    if sh.mesh:      # the moved instances of the GPU test: still glass, light samples and levels behind glass
        moved = LS.case(oracle, name, form, SS.box_xforms(moved=True))
        r = WK.walk(oracle, moved.sh.scene, W0, H0, LS.SEGMENTS, tex=tex, **LS.setup(oracle, moved, 6))
        assert r["transmitted"] and r["lit"] and r["mip_behind"] and r["sphere_valid"], (name, form, "moved")
        assert not np.array_equal(moved.sh.scene.tris, sc.tris)
