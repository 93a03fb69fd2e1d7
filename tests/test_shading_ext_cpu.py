"""The oracle's statement of K2's shading extensions (oracle_raytrace_ext: albedo textures, mip levels by ray footprint, specular
bounces, the ALBEDO plane), checked without a GPU before tests/test_shading_ext_gpu.py compares the HIP kernels with it:

  1. its sampler, its sampler at a level, its footprint and its bounce, item by item, bit for bit against the numpy restatements
     the device is pinned to (texture_scenes.sample, texture_mip_scenes.sample_lod / footprint_lod32, specular_scenes.bounce32);
  2. without extensions it is oracle_raytrace_seq_mat: image, hit id, ray count and dump;
  3. the properties the GPU suite ties the extended path to the plain one with hold for it too;
  4. every recorded hit of the scenes of tests/shading_scenes.py against float64: the level, the albedo's texel, the reflection;
  5. what the GPU test relies on in those scenes (shading_scenes.MEASURED), so that a scene that stops exercising something fails
     here first."""
import os
import subprocess

import numpy as np
import pytest

import gbuffer_scenes as G
import pathtrace_scenes as P
import shading_scenes as SS
import specular_scenes as S
import texture_mip_scenes as MS
import texture_scenes as TS
from conftest import ROOT
from filter_planes import same_bits

F32 = np.float32
W0, H0 = SS.SHAPES[0]
FILTERS = ((0, "bilinear"), (TS.NEAREST, "nearest"))


# ------------------------------------------------------------------------------------------ 1. function by function
@pytest.mark.parametrize("flags,_id", FILTERS, ids=[f[1] for f in FILTERS])
def test_sampler_equals_the_numpy_restatement(oracle, flags, _id):
    desc, texels = TS.four_sizes(flags)
    uv = TS.sampler_uvs()
    for d in desc:
        got = oracle.texture_sample(d, texels, uv)
        same_bits(got, TS.sample(texels, d, uv), ("sample", tuple(d)))
        assert (got > -999).all(), "no tap outside the rectangle"
    nan = oracle.texture_sample(desc[2], texels, F32([[np.nan, np.inf], [-np.inf, 0.25]]))
    assert (nan > -999).all() and np.isfinite(nan).all(), "a NaN coordinate reads inside the rectangle"


def hostile_levels(L):
    """at and around every integer of the chain, negative, NaN, infinite, beyond the chain"""
    ints = np.arange(-1, L + 2, dtype=F32)
    return np.concatenate([ints, np.nextafter(ints, F32(-np.inf)), np.nextafter(ints, F32(np.inf)), ints + F32(0.5), ints + F32(0.25),
                           F32([-0.0, np.nan, np.inf, -np.inf, 1e-30, -1e-30, 1e30])]).astype(F32)


@pytest.mark.parametrize("flags,_id", FILTERS, ids=[f[1] for f in FILTERS])
def test_level_sampler_equals_the_numpy_restatement(oracle, flags, _id):
    chains = [MS.random_chain(w, h, k + 1) for k, (w, h) in enumerate(MS.CHAIN_SIZES)]
    desc, texels = MS.chain_atlas(chains, flags, True)
    desc, texels, rows = SS.oracle_textures(desc, texels, oracle.level_row)
    uv = TS.sampler_uvs()[::5]
    for t, ch in enumerate(chains):
        assert rows[t, oracle.TEX_MAX_LEVELS] == len(ch)
        for lam in hostile_levels(len(ch)):
            got = oracle.texture_sample_lod(desc[t], rows[t], texels, uv, lam)
            same_bits(got, MS.sample_lod(ch, flags, uv, lam), ("sample_lod", MS.CHAIN_SIZES[t], float(lam)))
            assert (got > -999).all(), "no tap outside the chain"
        lam = np.random.default_rng(t).uniform(-1.0, len(ch) + 1.0, len(uv)).astype(F32)
        same_bits(oracle.texture_sample_lod(desc[t], rows[t], texels, uv, lam), MS.sample_lod(ch, flags, uv, lam), ("per item", t))


def test_generated_chain_table_reads_the_levels_of_build_chain(oracle):
    """oracle_textures: a texture with the mip flag alone reads MS.build_chain's levels, one without reads level 0 at every lambda"""
    images = [MS.random_image(w, h, k + 11) for k, (w, h) in enumerate(MS.CHAIN_SIZES)]
    desc, texels = TS.atlas(images)
    desc[::2, 3] = MS.MIPMAP
    desc, texels, rows = SS.oracle_textures(desc, texels, oracle.level_row)
    uv = TS.sampler_uvs()[::7]
    for t, im in enumerate(images):
        ch = MS.build_chain(im) if desc[t, 3] & MS.MIPMAP else [im]
        assert rows[t, oracle.TEX_MAX_LEVELS] == len(ch)
        for lam in (0.0, 0.75, 2.5, 40.0):
            same_bits(oracle.texture_sample_lod(desc[t], rows[t], texels, uv, lam), MS.sample_lod(ch, 0, uv, lam), ("generated", t, lam))


def test_footprint_equals_the_numpy_restatement(oracle):
    rng = np.random.default_rng(5)
    n = 4096
    p = rng.uniform(-3.0, 3.0, (n, 3, 3)).astype(F32)
    uv6 = rng.uniform(-2.5, 3.5, (n, 6)).astype(F32)
    w = (rng.uniform(0.001, 2.0, n) * 2.0 ** rng.integers(-6, 6, n)).astype(F32)
    nd = rng.uniform(-1.0, 1.0, n).astype(F32)
    # the degenerate operands: zero world area, zero texel area, n . d = 0, w = 0, infinite and NaN operands
    p[:64, 2] = p[:64, 1]
    uv6[64:128, 4:6] = uv6[64:128, 2:4]
    nd[128:192], w[192:256] = 0.0, 0.0
    w[256:264], nd[264:272] = F32(np.inf), F32(np.nan)
    p[272:280] *= F32(1e20)
    for W, H in ((64, 32), (1, 1), (33, 17), (65536, 1)):
        got = oracle.texture_footprint(w, nd, p, uv6, W, H)
        with np.errstate(all="ignore"):      # the operands of 1e20 overflow on purpose
            want = MS.footprint_lod32(w, nd, p, uv6, W, H)
        same_bits(got, want, ("footprint", W, H))
        assert (got[:280] == 0).all(), "level 0 by rule"
        assert len(np.unique(np.floor(got[280:]))) > 6 and (got[280:] != 0).mean() > 0.9


def test_bounce_equals_the_numpy_restatement(oracle):
    cases = np.concatenate([S.hostile_cases(), S.seeded_cases()])
    got, want = oracle.bounce(cases), S.bounce32(oracle, cases)
    same_bits(got[:, :3], want[:, :3], ("bounce", "d'"))
    same_bits(got[:, 3], want[:, 3], ("bounce", "absorbed"))
    assert 0 < (got[:, 3] != 0).sum() < len(got)


def test_new_oracle_code_under_sanitizers(tmp_path):
    """`make -C oracle shading-ext-check`: the path loop with every extension and every dump plane, and the array entry points on
    hostile operands, under the address and undefined-behaviour sanitizers in a program of its own; the atlas is allocated to the
    texel, so a tap outside it is an error"""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "shading-ext-check", f"OBJDIR={tmp_path}"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "shading_ext_check: ok" in out.stdout


# ------------------------------------------------------------------------------------------ 2. no extensions
def _same_frame(a, b, tag, keys=("IMAGE", "HIT_ID", "seq_id", "seq_n", "seq_end", "dir0")):
    for k in keys:
        same_bits(a[k], b[k], tag + (k,))
    assert a["rays"] == b["rays"], tag


@pytest.mark.parametrize("name,form", P.MAIN_SCENES, ids=[f"{n}-{f}" for n, f in P.MAIN_SCENES])
def test_without_extensions_it_is_raytrace_seq_mat(oracle, name, form):
    O = oracle
    W, H = P.MAIN_SHAPE
    sc = P.scene(name, form)
    tri_mat = None if sc.materials is None else O.material_records(sc.tri_material, sc.materials)
    for spp in (1, 3):
        cfg = P.configure(O.config_default(W, H), sc, P.SEGMENTS, spp)
        pc = G.fill_push_constants(O.PushConstants(), P.push_constants(sc), 0)
        image, rays, hit, seq_id, seq_n, seq_end, dir0 = O.raytrace_seq_mat(cfg, pc, sc.tris, tri_mat)
        want = dict(IMAGE=image, HIT_ID=hit, rays=rays, seq_id=seq_id, seq_n=seq_n, seq_end=seq_end, dir0=dir0)
        for null_ext in (False, True):
            got = O.raytrace_ext(cfg, pc, sc.tris, tri_mat, records=False, null_ext=null_ext)
            _same_frame(got, want, (name, form, spp, null_ext))


# ------------------------------------------------------------------------------------------ 3. properties
def _shading_of(sc, tri_uv, tri_texture, images, flags, spec=None):
    return SS.Shading(sc, spec, tri_uv, np.asarray(tri_texture, np.uint32), tuple(images), tuple(flags), None, None)


TEX_FLAGS = (0, TS.NEAREST, MS.MIPMAP, MS.MIPMAP | TS.NEAREST)


@pytest.mark.parametrize("name", SS.SCENES)
def test_an_all_ones_atlas_is_the_identity(oracle, name):
    sh = SS.world(oracle, SS.scene(name, "small"))
    want = SS.oracle_frame(oracle, sh, W0, H0, tex=0, records=False)
    for flags in TEX_FLAGS:
        ones = sh._replace(images=tuple(np.ones_like(im) for im in sh.images), tex_flags=(flags,) * len(sh.images))
        _same_frame(SS.oracle_frame(oracle, ones, W0, H0, tex=2, records=False), want, (name, flags))


@pytest.mark.parametrize("name", ["three_ends", "mask_room", "closed_room"])
def test_the_atlas_of_constants_is_the_material_table(oracle, name):
    """white materials under texture p = the constant colour Kd_p at random uv; with the mip flag the generated chain of equal texels
    is that texel at every level.  1, 2 and 9 segments"""
    sc = P.scene(name, "small", W0, H0)
    white = np.array(sc.materials, F32)
    white[:, :3] = 1.0
    kd = np.asarray(sc.materials)[:, :3]
    images = [TS.constant_image(*TS.TEX_SIZES[p % len(TS.TEX_SIZES)], c) for p, c in enumerate(kd)]
    for segments in (1, 2, 9):
        want = P.oracle_frame(oracle, sc, W0, H0, segments)
        for flags in TEX_FLAGS:
            sh = _shading_of(sc._replace(materials=white), TS.random_uv(len(sc.tris), 7), np.asarray(sc.tri_material) + 1, images,
                             (flags,) * len(images))
            _same_frame(SS.oracle_frame(oracle, sh, W0, H0, segments, records=False), want, (name, segments, flags), ("IMAGE", "HIT_ID", "seq_n"))


def test_a_chain_of_equal_texels_is_that_texel_at_every_level(oracle):
    for (w, h) in MS.CHAIN_SIZES:
        im = TS.constant_image(w, h, (0.3, 0.6, 0.9))
        desc, texels, rows = SS.oracle_textures(*TS.atlas([im], MS.MIPMAP), oracle.level_row)
        for lam in hostile_levels(len(MS.chain_dims(w, h))):
            got = oracle.texture_sample_lod(desc[0], rows[0], texels, TS.sampler_uvs()[::9], lam)
            same_bits(got, np.broadcast_to(im[0, 0], got.shape), ("equal texels", w, h, float(lam)))


@pytest.mark.parametrize("form", P.FORMS)
def test_room_of_mirrors_closed_form(oracle, form):
    """test_specular_gpu's closed form: every wall a mirror with Ks = (1/2, 1/4, 1/8): nothing is absorbed, every path lives n
    segments, every pixel is exactly (2^-n, 2^-2n, 2^-3n); demodulated IMAGE x ALBEDO is the value and ALBEDO is Ks"""
    sc, spec = S.mirror_room(form)
    sh = _shading_of(sc, np.zeros((len(sc.tris), 6), F32), np.zeros(len(sc.tris)), (), (), spec)
    for n in (1, 4, 9):
        value = F32([2.0 ** -n, 2.0 ** -(2 * n), 2.0 ** -(3 * n)])
        for spp, demod in ((1, False), (3, False), (1, True)):
            r = SS.oracle_frame(oracle, sh, W0, H0, n, spp, tex=0, demod=demod)
            assert r["rays"] == n * W0 * H0 * spp and (r["seq_end"] == oracle.END_BOUND).all()
            rgb = r["IMAGE"][..., :3]
            if demod:
                same_bits(r["ALBEDO"][..., :3], np.broadcast_to(F32(S.MIRROR_KS), rgb.shape), (form, n, "ALBEDO"))
                rgb = (rgb * r["ALBEDO"][..., :3]).astype(F32)
            same_bits(rgb, np.broadcast_to(value, rgb.shape), (form, n, spp, demod))


@pytest.mark.parametrize("name", SS.SCENES)
def test_the_demodulated_frame_factorises(oracle, name):
    """test_specular_trace_factorises' bound: IMAGE x ALBEDO against the plain frame within (segments + 2) 2^-23 |value|; the plane
    is (1, 1, 1) exactly where segment 0 ended the path, and the image is the plain one there"""
    for form in ("small", "odd"):
        sh = SS.world(oracle, SS.scene(name, form))
        for segments in (1, 2, 9):
            a = SS.oracle_frame(oracle, sh, W0, H0, segments, demod=True)
            b = SS.oracle_frame(oracle, sh, W0, H0, segments)
            _same_frame(a, b, (name, form, segments), ("HIT_ID", "seq_id", "seq_n", "seq_end"))
            alb, on_img, off_img = a["ALBEDO"][..., :3], a["IMAGE"][..., :3], b["IMAGE"][..., :3]
            assert (a["ALBEDO"][..., 3] == 0).all()
            went_on = (a["rec_code"][..., 0] & (oracle.REC_HIT | oracle.REC_ABSORBED)) != 0
            assert went_on.any() and (alb[~went_on] == 1).all()
            same_bits(on_img[~went_on], off_img[~went_on], (name, form, segments, "ended at the first query"))
            same_bits(alb[went_on], a["rec_albedo"][..., 0, :][went_on], (name, form, segments, "ALBEDO"))
            prod = (on_img * alb).astype(F32).astype(np.float64)
            bound = (segments + 2) * 2.0 ** -23 * np.abs(off_img.astype(np.float64))
            assert (np.abs(prod - off_img)[went_on] <= bound[went_on]).all(), (name, form, segments)


# ------------------------------------------------------------------------------------------ 4. against float64
def _hits64(rays, tris):
    """(id + 1 or 0, t, b1, b2) of the closest hit of rays [n, 6] against tris [t, 3, 3], float64 Moeller-Trumbore"""
    o, d = rays[:, None, :3], rays[:, None, 3:]
    e1, e2 = (tris[:, 1] - tris[:, 0])[None], (tris[:, 2] - tris[:, 0])[None]
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(-1)
    with np.errstate(all="ignore"):
        tv = o - tris[None, :, 0]
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1)
        v = (d * qv).sum(-1) / det
        t = (e2 * qv).sum(-1) / det
    hit = (np.abs(det) > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
    t = np.where(hit, t, np.inf)
    best = t.argmin(1)
    i = np.arange(len(rays))
    return np.where(np.isfinite(t[i, best]), best + 1, 0), t[i, best], u[i, best], v[i, best]


def _rng_floats(W, H, n):
    """[H, W, n] float64: the first n floats of every pixel's stream at frame 0 (raytrace.comp.glsl:71-78, :297)"""
    M = np.uint64(0xFFFFFFFF)
    x, y = np.meshgrid(np.arange(W, dtype=np.uint64), np.arange(H, dtype=np.uint64))
    s = ((x * np.uint64(3266489917) + y * np.uint64(668265263)) & M)
    out = []
    for _ in range(n):
        s = (s * np.uint64(747796405) + np.uint64(1)) & M
        w = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & M
        w = (w >> np.uint64(22)) ^ w
        out.append(w.astype(np.float32).astype(np.float64) * 2.0 ** -32)
    return np.stack(out, -1)


@pytest.mark.parametrize("form", ["small", "odd"])
@pytest.mark.parametrize("name", SS.SCENES)
def test_recorded_hits_against_float64(oracle, name, form):
    """every closest-hit record of a 9-segment frame, replayed in float64 from the record's own ray: the geometry from MS.posed,
    the hit and its barycentrics from a float64 intersection, the level from MS.lod_of_rays, the texel from uv of the float64
    barycentrics, the next record's direction from S.bounce64 with the pixel's own two draws.
      level       within MS.BAR of a level wherever the float64 level is not within MS.BAR of a clamp and the uv triangle has area
      albedo      of a bilinear hit within 2^-10, sampled at the level the oracle recorded: the binary32 barycentrics are a few rounded
                  operations on values in [0, 1] (within 2^-18 of the float64 ones), uv is their sum weighted by |uv| <= 3.5 (2^-15
                  with its own roundings), a unit of u spans at most 33 texels (2^-10 of a texel) and neighbouring texels differ
                  by less than 1.  A uv record with two vertices exchanged moves the sample by whole texels
      direction   within 2^-16 per component (the bar of test_specular_gpu's mirror quad for the same chain) wherever the lobe
                  vector is longer than 1/4 (its normalisation amplifies by at most 4)"""
    O = oracle
    sh = SS.world(O, SS.scene(name, form))
    sc, nb = sh.scene, SS.n_base(sh)
    r = SS.oracle_frame(O, sh, W0, H0)
    tris = MS.posed(sh.mesh[0], sh.mesh[1], sh.xforms) if sh.mesh else np.asarray(sc.tris, np.float64).reshape(-1, 3, 3)
    assert np.abs(tris - np.asarray(sc.tris, np.float64).reshape(-1, 3, 3)).max() < 1e-5
    code, seq_id = r["rec_code"], r["seq_id"].astype(np.int64)
    shaded = (code & (O.REC_HIT | O.REC_ABSORBED)) != 0
    py, px, pk = np.nonzero(shaded)
    rays = r["rec_ray"][shaded].astype(np.float64)
    ids, t, b1, b2 = _hits64(rays, tris)
    same = ids == seq_id[shaded]
    assert same.mean() > 0.995, (name, form, same.mean())
    rec = (ids - 1) % nb
    dims = [(im.shape[1], im.shape[0]) for im in sh.images]
    chains = [MS.build_chain(im) if f & MS.MIPMAP else [np.asarray(im)] for im, f in zip(sh.images, sh.tex_flags)]
    # ---- the level
    want = np.zeros(len(rays))
    for primary, spread in ((True, MS.primary_spread(sc.slope, H0)), (False, MS.BOUNCE_SPREAD)):
        m = (pk == 0) == primary
        ids2, lam = MS.lod_of_rays(rays[m], tris, sh.tri_uv, sh.tri_texture, dims, [len(c) for c in chains], spread)
        assert np.array_equal(ids2, ids[m])
        want[m] = lam
    tex = sh.tri_texture[rec].astype(np.int64)
    top = np.array([len(c) - 1.0 for c in chains] + [0.0])[tex - 1]
    uv6 = sh.tri_uv[rec].astype(np.float64)
    area = np.abs((uv6[:, 2] - uv6[:, 0]) * (uv6[:, 5] - uv6[:, 1]) - (uv6[:, 4] - uv6[:, 0]) * (uv6[:, 3] - uv6[:, 1]))
    judged = same & (tex > 0) & (top > 0) & (want > MS.BAR) & (want < top - MS.BAR) & (area > 1e-6)
    err = np.abs(r["rec_lod"][shaded] - want)
    print(f"{name} {form}: {judged.sum()} levels judged of {int((same & (tex > 0)).sum())} textured hits, max error {err[judged].max():.3e} (bar {MS.BAR:.3e})")
    assert judged.sum() > 300 and err[judged].max() <= MS.BAR
    clamped = same & (tex > 0) & ~judged
    assert (err[clamped] <= 2 * MS.BAR).all(), "next to a clamp both sides are within the bar of it"
    # ---- the albedo
    colour = np.array(sc.materials[:, :3], np.float64)
    for m_, (ks, _) in (sh.spec or {}).items():
        colour[m_] = ks
    b0 = 1.0 - b1 - b2
    uv = (b0[:, None] * uv6[:, 0:2] + b1[:, None] * uv6[:, 2:4] + b2[:, None] * uv6[:, 4:6]).astype(F32)
    worst = 0.0
    for k, ch in enumerate(chains):
        m = same & (tex == k + 1)
        if sh.tex_flags[k] & TS.NEAREST or not m.any():
            continue
        texel = MS.sample_lod(ch, 0, uv[m], r["rec_lod"][shaded][m])[:, :3].astype(np.float64)
        e = np.abs(texel * colour[sc.tri_material[rec[m]]] - r["rec_albedo"][shaded][m]).max()
        worst = max(worst, float(e))
    untextured = same & (tex == 0)
    same_bits(r["rec_albedo"][shaded][untextured], colour[sc.tri_material[rec[untextured]]].astype(F32), (name, form, "untextured albedo"))
    print(f"{name} {form}: bilinear albedo max error {worst:.3e} (bar {2.0 ** -10:.3e})")
    assert worst <= 2.0 ** -10
    # ---- the reflection
    is_spec = (code[shaded] & O.REC_SPECULAR) != 0
    g = np.zeros(len(sc.materials))
    for m_, (_, gm) in (sh.spec or {}).items():
        g[m_] = gm
    nxt = same & is_spec & ((code[shaded] & O.REC_ABSORBED) == 0) & (pk + 1 < r["seq_n"][py, px])
    if sh.spec:
        u = _rng_floats(W0, H0, 2 + 2 * SS.SEGMENTS)
        n = np.cross(tris[ids - 1, 1] - tris[ids - 1, 0], tris[ids - 1, 2] - tris[ids - 1, 0])
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        cases = np.concatenate([rays[:, 3:], n, u[py, px, 2 + 2 * pk][:, None], u[py, px, 3 + 2 * pk][:, None], g[sc.tri_material[rec]][:, None]], 1)
        dn, ndn, ln = S.bounce64(cases)
        d_next = r["rec_ray"][py, px, np.minimum(pk + 1, SS.SEGMENTS - 1), 3:].astype(np.float64)
        judged = nxt & (ln > 0.25) & (ndn > 1e-3)
        err = np.abs(d_next - dn).max(1)
        print(f"{name} {form}: {judged.sum()} reflections judged, max error {err[judged].max():.3e} (bar {2.0 ** -16:.3e})")
        assert judged.sum() > 300 and err[judged].max() <= 2.0 ** -16
        absorbed = same & ((code[shaded] & O.REC_ABSORBED) != 0)
        assert (ndn[absorbed] < 1e-5).all(), "an absorbed path's lobe left the surface"
    else:
        assert not is_spec.any()


# ------------------------------------------------------------------------------------------ 5. what the GPU test relies on
@pytest.mark.parametrize("form", P.FORMS)
@pytest.mark.parametrize("name", SS.SCENES)
def test_scenes_exercise_what_they_claim(oracle, name, form):
    sh = SS.world(oracle, SS.scene(name, form))
    sc = sh.scene
    assert sc.tris.dtype == np.float32 and not sc.tris.flags.writeable and len(sc.tris) < 65536
    if form == "small":
        assert len(sc.tris) <= 64
    else:
        assert len(sc.tris) > 64 and P.is_all_fan_pairs(sc.tris) == (form == "pairs")
    assert len(sh.tri_uv) == len(sh.tri_texture) == len(sc.tri_material) == SS.n_base(sh)
    assert len(sc.tris) == SS.n_base(sh) * (len(sh.xforms) if sh.mesh else 1)
    r = SS.oracle_frame(oracle, sh, W0, H0)
    assert not np.isnan(r["IMAGE"]).any() and r["rays"] == int(r["seq_n"].sum())
    got = SS.counts(oracle, sh, r, P.window_of(None, form))
    print((name, form), {k: v for k, v in got.items() if v})
    measured = SS.MEASURED[name, form]
    assert set(SS.REQUIRED[name]) <= set(measured), "every precondition of the scene has a recorded count"
    for k, m in measured.items():
        assert m > 0, "no floor may be met by nothing"
        assert got[k] >= max(1, (m + 1) // 2), (name, form, k, got[k], m)
    assert got["lod_levels"] >= SS.MIN_LOD_LEVELS
    assert got["albedos"] > len(sc.materials), "more albedos among bounce hits than materials: texels were read"
    if name == "textured_room":
        uv6 = sh.tri_uv.astype(np.float64)
        area = (uv6[:, 2] - uv6[:, 0]) * (uv6[:, 5] - uv6[:, 1]) - (uv6[:, 4] - uv6[:, 0]) * (uv6[:, 3] - uv6[:, 1])
        flat = np.flatnonzero((area == 0) & (sh.tri_texture > 0))
        assert len(flat) and np.isin(r["seq_id"][..., 1:], flat + 1).any(), "bounce hits on the uv triangle of zero area"
        assert (sh.tri_texture == 0).any() and (sc.materials[:, 3:] != 0).any()
    if sh.mesh:
        moved = SS.world(oracle, sh, SS.box_xforms(moved=True))
        c = SS.counts(oracle, moved, SS.oracle_frame(oracle, moved, W0, H0), P.window_of(None, form))
        assert all(c[f"instance{i}"] > 0 for i in range(3)) and c["mirror"] and c["glossy"], c
        assert not np.array_equal(moved.scene.tris, sc.tris)


@pytest.mark.parametrize("name", SS.SCENES)
def test_budgets_and_windows_of_the_gpu_test_are_crossed(oracle, name):
    """the GPU test's budgets 1, 2, window + 1 and 9, and RTPT_PT_WINDOW = 1 at 9 segments: paths are alive behind every boundary"""
    for form in P.FORMS:
        sh = SS.world(oracle, SS.scene(name, form))
        w = P.window_of(None, form)
        for segments in (w + 1, SS.SEGMENTS):
            n = SS.oracle_frame(oracle, sh, W0, H0, segments, records=False)["seq_n"]
            assert all(a > 0 for a in P.alive_after(n, P.window_boundaries(w, segments))), (name, form, segments)
            assert all(a > 0 for a in P.alive_after(n, P.window_boundaries(1, segments))), (name, form, segments)
    W, H, y0, y1 = P.STRIP
    sh = SS.scene("glossy_textured_room", "small")
    strip = SS.oracle_frame(oracle, sh, W, H, rows=(y0, y1), records=False)
    assert 0 < strip["rays"] == int(strip["seq_n"][y0:y1].sum()) and (strip["seq_n"][:y0] == 0).all()
