"""Mip-mapped albedo textures on the device (RTPT_TEX_MIPMAP, RTPT_TEX_MIPS_GIVEN): the generated chain and the level sampler
bit for bit against the numpy restatement of tests/texture_mip_scenes.py, the level selection against a float64 restatement
from the ray, the mesh and the uvs alone, the path-trace kernels tied to both, then accounting, refusals and the hosts.

Frames are 64 x 48 and 70 x 10, as in test_textures_gpu.py, whose helpers this file uses."""
import gc
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import test_demodulate_gpu as D
import test_textures_gpu as T
import texture_mip_scenes as MS
import texture_scenes as TS
from conftest import ROOT, SCENE, bits

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = D.SIZES
VARIANT_IDS = D.VARIANT_IDS
FILTERS = T.FILTERS
MODES = [(0, "brute"), (0x2, "bvh")]      # 0x2: RTPT_FLAG_FORCE_BVH


@pytest.fixture(scope="module")
def mesh(hip_lib):
    return hip_lib.load_obj(SCENE)


def plain_context(abi, mesh, desc, texels):
    ctx = abi.Context(abi.config_default(64, 48))
    ctx.scene_upload(*mesh)
    n = len(mesh[1])
    ctx.set_textures(np.zeros((n, 6), F32), np.zeros(n, np.uint32), desc, texels)
    return ctx


# ------------------------------------------------------------------------------------------------ 1. the generated chain
def test_generated_chain_equals_numpy(hip_lib, mesh):
    """every texel of every level of the generated chains of random images of every size of GEOMETRY_SIZES, read through
    rtpt_selftest_texture_lod with RTPT_TEX_NEAREST, integer lambda and texel-centre uv"""
    abi = hip_lib
    assert abi.FLAG_FORCE_BVH == 0x2
    chains = [MS.build_chain(MS.random_image(w, h, k + 1)) for k, (w, h) in enumerate(MS.GEOMETRY_SIZES)]
    desc, texels = MS.chain_atlas(chains, MS.NEAREST, given=False)
    with plain_context(abi, mesh, desc, texels) as ctx:
        for t, ch in enumerate(chains):
            assert len(ch) == abi.texture_chain(*MS.GEOMETRY_SIZES[t])[0]
            for l, level in enumerate(ch):
                h, w = level.shape[:2]
                x, y = np.meshgrid(np.arange(w), np.arange(h))
                uv = np.stack([(x + 0.5) / w, (y + 0.5) / h], -1).reshape(-1, 2).astype(F32)
                got = ctx.selftest_texture_lod(t, uv, float(l)).reshape(h, w, 4)
                assert np.array_equal(bits(got), bits(level)), (MS.GEOMETRY_SIZES[t], l)
            assert np.array_equal(bits(ctx.selftest_texture(t, F32([[0.0, 0.0]]))[0]), bits(ch[0][0, 0])), "rtpt_selftest_texture reads level 0"


# ------------------------------------------------------------------------------------------------ 2. the sampler
@pytest.mark.parametrize("given", [False, True], ids=["generated", "given"])
@pytest.mark.parametrize("filt", FILTERS, ids=[f[0] for f in FILTERS])
def test_level_sampler_equals_the_numpy_restatement(hip_lib, mesh, filt, given):
    abi = hip_lib
    if given:
        chains = [MS.random_chain(w, h, k + 1) for k, (w, h) in enumerate(MS.CHAIN_SIZES)]
    else:
        chains = [MS.build_chain(MS.random_image(w, h, k + 11)) for k, (w, h) in enumerate(MS.CHAIN_SIZES)]
    desc, texels = MS.chain_atlas(chains, filt[1], given)
    uv = TS.sampler_uvs()
    with plain_context(abi, mesh, desc, texels) as ctx:
        for t, ch in enumerate(chains):
            L = len(ch)
            for lam in (-1.0, 0.0, 0.25, 1.0, 1.5, L - 1.0, L + 3.0, np.nan):
                got = ctx.selftest_texture_lod(t, uv, lam)
                want = MS.sample_lod(ch, filt[1], uv, lam)
                bad = np.flatnonzero((bits(got) != bits(want)).any(1))
                assert bad.size == 0, (filt[0], given, MS.CHAIN_SIZES[t], lam, uv[bad[:4]], got[bad[:4]], want[bad[:4]])
                assert (got > -999).all(), "no tap outside the chain"
            # a per-ray lambda: random levels across the chain and beyond both ends
            lam = np.random.default_rng(t).uniform(-1.0, L + 1.0, len(uv)).astype(F32)
            assert np.array_equal(bits(ctx.selftest_texture_lod(t, uv, lam)), bits(MS.sample_lod(ch, filt[1], uv, lam)))


def test_textures_without_the_flag_have_one_level(hip_lib, mesh):
    """in a scene without any chain, and next to a mip-mapped texture: every lambda reads level 0"""
    abi = hip_lib
    uv = TS.sampler_uvs()[::7]
    for flags in (0, TS.NEAREST):
        desc, texels = TS.four_sizes(flags)
        with plain_context(abi, mesh, desc, texels) as ctx:
            for t in range(len(desc)):
                for lam in (0.0, 2.5, np.nan):
                    assert np.array_equal(bits(ctx.selftest_texture_lod(t, uv, lam)), bits(TS.sample(texels, desc[t], uv)))
        mixed = desc.copy()
        mixed[3, 3] |= MS.MIPMAP          # the 8 x 8 texture gets a generated chain; the others keep one level
        with plain_context(abi, mesh, mixed, texels) as ctx:
            for t in range(3):
                assert np.array_equal(bits(ctx.selftest_texture_lod(t, uv, 2.5)), bits(TS.sample(texels, desc[t], uv)))
            ch = MS.build_chain(texels[desc[3, 2]:desc[3, 2] + 64].reshape(8, 8, 4))
            assert np.array_equal(bits(ctx.selftest_texture_lod(3, uv, 1.5)), bits(MS.sample_lod(ch, flags, uv, 1.5)))


# ------------------------------------------------------------------------------------------------ 3. lambda from geometry
TEX_W, TEX_H = 64, 32            # 7 levels


def footprint_app(abi, size, vflags, uv_scale, xforms=None, tex_flags=MS.MIPMAP):
    app = D.make(abi, size, vflags, 2, TS.quad_mesh(), cameraOrigin=TS.QUAD_CAM, instance_xforms=xforms)
    tri_uv = (TS.quad_tri_uv() * F32(uv_scale)).astype(F32)
    desc = np.array([[TEX_W, TEX_H, 0, tex_flags]], np.uint32)
    T.set_textures(app, tri_uv, np.ones(2, np.uint32), desc, MS.random_image(TEX_W, TEX_H, 1).reshape(-1, 4))
    return app, tri_uv


def check_footprint(ctx, rays, bounce, tris, tri_uv, spread, what, ids_exact=True):
    ids, lam = ctx.selftest_texture_footprint(rays, bounce)
    want_ids, want = MS.lod_of_rays(rays, tris, tri_uv, np.ones(len(tri_uv), np.uint32), [(TEX_W, TEX_H)], [7], spread)
    if ids_exact:
        assert np.array_equal(ids, want_ids), what
    else:       # rays that may run along the quad's diagonal: both triangles have the one density of the affine uv map
        assert np.array_equal(ids > 0, want_ids > 0), what
    on = ids > 0
    assert on.sum() >= 100 and (lam[~on] == 0).all()
    inside = (want[on] > 0.05) & (want[on] < 5.95)
    assert inside.mean() > 0.9, (what, "the rays stay away from the clamps")
    if ids_exact:
        assert want[on].max() - want[on].min() > 1.0, (what, "the rays span more than a level")
    err = float(np.abs(lam[on].astype(np.float64) - want[on]).max())
    print(f"footprint {what} bounce {bounce}: {on.sum()} hits, lambda {want[on].min():.3f} .. {want[on].max():.3f}, "
          f"max error {err:.3e} of a level (bar {MS.BAR:.3e})")
    assert err <= MS.BAR, what
    return err


@pytest.mark.parametrize("vflags,mode", MODES, ids=[m[1] for m in MODES])
def test_lambda_follows_the_geometry(hip_lib, vflags, mode):
    """rtpt_selftest_texture_footprint against the float64 restatement (texture_mip_scenes.lod_of_rays: its own closest hit, its
    own areas, the piecewise-linear log2 in float64) on the sheared quad, on two instances of it with different — one of them
    non-uniform — scale, and after a changed model matrix; both rules; the bar is 2^-10 of a level = 9.766e-04.
    Measured on an MI355X, brute force and forced BVH alike: max error 5.893e-07 of a level over all cases."""
    abi = hip_lib
    xyz, idx = TS.quad_mesh()
    xf = np.zeros((2, 3, 4), F32)
    xf[0, 0, 0] = xf[0, 1, 1] = xf[0, 2, 2] = 1
    xf[0, :, 3] = (-4.0, 0.0, 0.0)
    xf[1] = [[0.5, 0.2, 0, 4.0], [0, 0.7, 0, 0.5], [0, 0, 0.5, 0]]
    model = np.eye(4, dtype=F32)
    model[0, 0], model[1, 1], model[3, 0], model[3, 1] = 1.5, 0.8, 0.3, -0.2      # [column, row]: scales and a translation
    worst = 0.0
    for size in SIZES:
        pix = MS.primary_spread(abi.config_default(*size).fov_slope, size[1])
        # uv scales that put lambda mid-chain: the pixel's footprint is 1 / 15 (64 x 48) or 1 / 3 (70 x 10) of the bounce's
        for bounce, spread, uv_scale in ((0, pix, 32.0 if size[1] == 48 else 7.0), (1, MS.BOUNCE_SPREAD, 2.0)):
            for what, xforms in (("quad", None), ("instances", xf)):
                app, tri_uv = footprint_app(abi, size, vflags, uv_scale, xforms)
                ctx = app.backend.ctx
                tris = MS.posed(xyz, idx, xforms)
                worst = max(worst, check_footprint(ctx, MS.rays_into(tris, 1500, 3), bounce, tris, tri_uv, spread, (size, mode, what)))
                if xforms is None and bounce == 0:       # the frame's own primary rays
                    rays = MS.pixel_centre_rays(size, ctx.cfg.fov_slope, TS.QUAD_CAM)
                    worst = max(worst, check_footprint(ctx, rays, 0, tris, tri_uv, spread, (size, mode, "pixel centres"), ids_exact=False))
                # a changed model: posed inside the next rtpt_gbuffer
                app.modelMatrix = model.ravel()
                D.trace(app, ())
                D.finish(app)
                tris = MS.posed(xyz, idx, xforms, model)
                worst = max(worst, check_footprint(ctx, MS.rays_into(tris, 1500, 4), bounce, tris, tri_uv, spread, (size, mode, what, "model")))
                app.backend.close()
    print(f"lambda from geometry, {mode}: max error {worst:.3e} of a level over all cases (bar {MS.BAR:.3e})")


@pytest.mark.parametrize("vflags,mode", MODES, ids=[m[1] for m in MODES])
def test_four_texels_to_the_pixel_read_level_two(hip_lib, vflags, mode):
    """closed form: a camera-facing quad whose texel density makes the centre ray's pixel 4 texels wide: rho^2 = 16, and the
    piecewise-linear log2 is exact there: lambda = 2.  Untextured hits, textures without the flag and misses return 0."""
    abi = hip_lib
    xyz, idx = TS.quad_mesh()
    ray = F32([list(TS.QUAD_CAM) + [0, 0, -1], list(TS.QUAD_CAM) + [0, 0, 1]])       # the second one leaves the scene
    for size in SIZES:
        pix = MS.primary_spread(abi.config_default(*size).fov_slope, size[1])
        per_unit = 4.0 / (TS.QUAD_CAM[2] * pix)              # texels per world unit
        tri_uv = (xyz[idx][:, :, :2].astype(np.float64) * per_unit / 64).reshape(-1, 6).astype(F32)
        for tex_flags, tri_texture, want in ((MS.MIPMAP, 1, 2.0), (MS.MIPMAP | MS.NEAREST, 1, 2.0), (0, 1, 0.0), (MS.MIPMAP, 0, 0.0)):
            app = D.make(abi, size, vflags, 2, TS.quad_mesh(), cameraOrigin=TS.QUAD_CAM)
            desc, texels = np.array([[64, 64, 0, tex_flags]], np.uint32), MS.random_image(64, 64, 2).reshape(-1, 4)
            T.set_textures(app, tri_uv, np.full(2, tri_texture, np.uint32), desc, texels)
            ids, lam = app.backend.ctx.selftest_texture_footprint(ray, 0)
            assert ids[0] > 0 and ids[1] == 0 and lam[1] == 0
            print(f"closed form {size} {mode} flags {tex_flags:#x} texture {tri_texture}: lambda {lam[0]!r} (want {want})")
            assert abs(float(lam[0]) - want) <= MS.BAR
            # the bounce rule at the same hit: w = t / 8 instead of t pix
            ids, lam = app.backend.ctx.selftest_texture_footprint(ray, 1)
            want1 = min(6.0, max(0.0, 0.5 * MS.plog2_f64(16.0 * (MS.BOUNCE_SPREAD / pix) ** 2))) if want else 0.0
            assert abs(float(lam[0]) - want1) <= MS.BAR
            app.backend.close()
    with abi.Context(abi.config_default(64, 48)) as ctx:       # a scene without textures
        ctx.scene_upload(*TS.quad_mesh())
        ids, lam = ctx.selftest_texture_footprint(ray, 0)
        assert ids[0] > 0 and (lam == 0).all()
        with pytest.raises(abi.RtptError) as e:
            ctx.selftest_texture_footprint(ray, 2)
        assert e.value.code == abi.RTPT_E_INVALID


# ------------------------------------------------------------------------------------------------ 4. K2 uses it
def floor_app(abi, size, vflags, chain, tex_flags, given, seg=2, per_unit=3.0 / 64, **kw):
    app = D.make(abi, size, vflags, seg, MS.floor_mesh(), (np.zeros(2, np.uint32), np.array([[1, 1, 1, 0, 0, 0]], F32)),
                 cameraOrigin=MS.FLOOR_CAM, **kw)
    desc, texels = MS.chain_atlas([chain], tex_flags, given)
    T.set_textures(app, MS.floor_tri_uv(per_unit), np.ones(2, np.uint32), desc, texels)
    return app


@pytest.mark.parametrize("variant", range(6), ids=VARIANT_IDS)
def test_first_hit_albedo_is_the_level_of_the_footprint(hip_lib, monkeypatch, variant):
    """a given chain whose level l is the constant l / 8, bilinear, no jitter, demodulation: ALBEDO.r x 8 of every pixel that
    hits the floor is the lambda rtpt_selftest_texture_footprint returns for the restated pixel-centre ray, within 2^-10.
    Measured on an MI355X, every variant alike: max difference 1.073e-06 of a level; the 64 x 48 frame spans lambda 0.394 to 5.191,
    70 x 10 2.892 to 6 (the clamp)."""
    abi = hip_lib
    _, vflags, seg = D.variants()[variant]
    T.quad_config(abi, monkeypatch)
    chain = [np.full((h, w, 4), l / 8.0, F32) for l, (w, h) in enumerate(MS.chain_dims(64, 64))]
    for size in SIZES:
        app = floor_app(abi, size, vflags | abi.FLAG_EXT_DEMODULATE, chain, 0, True, seg=seg, debug_mask=abi.DEBUG_HIT_ID)
        ctx = app.backend.ctx
        D.trace(app, ())
        alb, hit = ctx.readback(abi.PLANE_ALBEDO), ctx.readback(abi.PLANE_HIT_ID)
        ids, lam = ctx.selftest_texture_footprint(MS.pixel_centre_rays(size, ctx.cfg.fov_slope, MS.FLOOR_CAM), 0)
        app.backend.close()
        on = hit > 0
        assert np.array_equal(on, ids.reshape(hit.shape) > 0), "the restated rays and K2 agree on the pixels that hit the floor"
        assert on.sum() >= 0.25 * on.size
        lam = lam.reshape(hit.shape)[on].astype(np.float64)
        got = alb[on][:, 0].astype(np.float64) * 8
        assert lam.max() - lam.min() >= 1.0, "the frame spans at least one whole level"
        assert ((lam > 0) & (lam < 6)).mean() > 0.5
        err = float(np.abs(got - lam).max())
        print(f"{VARIANT_IDS[variant]} {size}: {on.sum()} pixels, lambda {lam.min():.3f} .. {lam.max():.3f}, "
              f"max |ALBEDO.r x 8 - lambda| = {err:.3e} (bar {MS.BAR:.3e})")
        assert err <= MS.BAR
        assert (alb[~on][:, :3] == 1).all()


# ------------------------------------------------------------------------------------------------ 5. equal constants
@pytest.mark.parametrize("variant", range(6), ids=VARIANT_IDS)
def test_chain_of_equal_constants_is_the_material_table(hip_lib, mesh, variant):
    """test_textures_gpu.py::test_atlas_of_constants_is_the_material_table with RTPT_TEX_MIPMAP on every texture: the box mean
    of equal values and a lerp of equal taps are exact, so frames, ALBEDO and ray counts stay those of the material table"""
    abi = hip_lib
    _, vflags, seg = D.variants()[variant]
    vflags |= abi.FLAG_EXT_DEMODULATE
    n = len(mesh[1])

    def frames(app):
        out, ctx = [], app.backend.ctx
        for frame in range(2):
            D.trace(app, ("J",) if frame else ())
            out.append((ctx.readback(abi.PLANE_IMAGE), ctx.readback(abi.PLANE_HIT_ID), ctx.raycount(), ctx.readback(abi.PLANE_ALBEDO)))
            D.finish(app)
        app.backend.close()
        return out
    for size in SIZES:
        plain, white, _ = T.constants_setup(n, 0)
        want = frames(D.make(abi, size, vflags, seg, mesh, plain, debug_mask=abi.DEBUG_HIT_ID))
        for name, flags in FILTERS:
            uv, tri_texture, desc, texels = T.constants_setup(n, flags)[2]
            desc = desc.copy()
            desc[:, 3] |= MS.MIPMAP
            app = D.make(abi, size, vflags, seg, mesh, white, debug_mask=abi.DEBUG_HIT_ID)
            T.set_textures(app, (uv * F32(40)).astype(F32), tri_texture, desc, texels)       # minified: levels above 0 are read
            got = frames(app)
            T.assert_same_frames(got, want, (size, name))
            for f in range(2):
                assert np.array_equal(bits(got[f][3]), bits(want[f][3])), (size, name, f, "ALBEDO")


# ------------------------------------------------------------------------------------------------ 6. magnified first hit
@pytest.mark.parametrize("vflags,mode", MODES, ids=[m[1] for m in MODES])
def test_magnified_first_hit_reads_level_zero(hip_lib, monkeypatch, vflags, mode):
    """every first-hit footprint is below one texel: ALBEDO is the un-mipped texture's, bit for bit"""
    abi = hip_lib
    T.quad_config(abi, monkeypatch)
    image = TS.distinct_image(8, 8, 3)
    for size in SIZES:
        for name, flags in FILTERS:
            alb = {}
            for mip in (0, MS.MIPMAP):
                app = T.quad_app(abi, size, vflags | abi.FLAG_EXT_DEMODULATE, TS.quad_tri_uv(), image, flags | mip, debug_mask=abi.DEBUG_HIT_ID)
                ctx = app.backend.ctx
                D.trace(app, ())
                alb[mip] = ctx.readback(abi.PLANE_ALBEDO)
                if mip:
                    ids, lam = ctx.selftest_texture_footprint(MS.pixel_centre_rays(size, ctx.cfg.fov_slope, TS.QUAD_CAM), 0)
                    assert (ids > 0).sum() >= 0.3 * ids.size and (lam == 0).all(), "every footprint is below one texel"
                app.backend.close()
            assert np.array_equal(bits(alb[0]), bits(alb[MS.MIPMAP])), (size, name)
            assert len(np.unique(alb[0][..., 0])) > (8 if flags & TS.NEAREST else 50), "the plane shows the texture's detail"


# ------------------------------------------------------------------------------------------------ 7. accounting and refusals
def mip_setup(n_tris):
    """three generated chains, one given chain and one plain texture"""
    chains = [MS.build_chain(MS.random_image(w, h, k)) for k, (w, h) in enumerate(((5, 3), (8, 8), (33, 17)))]
    d1, t1 = MS.chain_atlas(chains, 0, False)
    d2, t2 = MS.chain_atlas([MS.random_chain(16, 4, 9)], MS.NEAREST, True)
    d3, t3 = TS.atlas([TS.distinct_image(3, 5, 1)], 0)
    d2[:, 2] += len(t1)
    d3[:, 2] += len(t1) + len(t2)
    desc, texels = np.concatenate([d1, d2, d3]), np.concatenate([t1, t2, t3])
    generated = sum(sum(l.shape[0] * l.shape[1] for l in ch[1:]) for ch in chains)
    tri_texture = (np.arange(n_tris) % (len(desc) + 1)).astype(np.uint32)
    return (TS.random_uv(n_tris, 17), tri_texture, desc, texels), generated


def test_device_bytes_follow_the_mip_formula(hip_lib, mesh):
    """32 n_tris + 16 n_textures + 16 n_texels + 16 G + 80 n_textures with a mip flag on any texture (G: the generated texels);
    the first three terms alone without"""
    abi = hip_lib
    gc.collect()
    n = len(mesh[1])
    args, generated = mip_setup(n)
    uv, tri_texture, desc, texels = args
    assert generated == (2 + 1) + (16 + 4 + 1) + (128 + 32 + 8 + 2 + 1)
    want = 32 * n + 16 * len(desc) + 16 * len(texels) + 16 * generated + 80 * len(desc)
    before = abi.live_device_bytes()
    ctx = abi.Context(abi.config_default(64, 48))
    ctx.scene_upload(*mesh)
    base = abi.live_device_bytes()
    ctx.set_textures(*args)
    assert abi.live_device_bytes() == base + want
    plain = desc.copy()
    plain[:, 3] &= MS.NEAREST
    ctx.set_textures(uv, tri_texture, plain, texels)                       # replaced by a set without chains: the plain formula
    assert abi.live_device_bytes() == base + 32 * n + 16 * len(desc) + 16 * len(texels)
    given_only = desc[3:4].copy()                                           # a given chain alone: a table, nothing generated
    ctx.set_textures(uv, np.minimum(tri_texture, 1), given_only, texels)
    assert abi.live_device_bytes() == base + 32 * n + 16 + 16 * len(texels) + 80
    ctx.set_textures(*args)
    assert abi.live_device_bytes() == base + want
    ctx.set_textures(None, None, None, None)
    assert abi.live_device_bytes() == base
    ctx.set_textures(*args)
    ctx.scene_upload(*mesh)                                                 # a new scene drops them, chains and table included
    assert abi.live_device_bytes() == base
    ctx.set_textures(*args)
    ctx.resize(70, 10)
    ctx.resize(64, 48)
    assert ctx.selftest_texture_lod(2, F32([[0.5, 0.5]]), 3.0).shape == (1, 4), "a resize keeps the chains"
    ctx.close()
    assert abi.live_device_bytes() == before


def test_mip_refusals_leave_the_scene_untouched(hip_lib, mesh):
    abi = hip_lib
    n = len(mesh[1])
    args, _ = mip_setup(n)
    uv, tri_texture, desc, texels = args

    def bad_calls():
        d = desc.copy(); d[4, 3] = MS.MIPS_GIVEN
        yield "MIPS_GIVEN without MIPMAP", (uv, tri_texture, d, texels)
        d = desc.copy(); d[4, 3] = MS.MIPS_GIVEN | MS.NEAREST
        yield "MIPS_GIVEN | NEAREST without MIPMAP", (uv, tri_texture, d, texels)
        d = desc.copy(); d[4, 3] = MS.MIPMAP | MS.MIPS_GIVEN        # the last texture: level 0 fits, the chain ends beyond n_texels
        yield "a given chain beyond n_texels", (uv, tri_texture, d, texels)
        yield "a given chain cut short", (uv, np.minimum(tri_texture, 4), desc[:4], texels[:desc[3, 2] + 64 + 16 + 4 + 2])
        for bit in (0x2, 0x4, 0x8):
            for keep in (0, MS.MIPMAP):
                d = desc.copy(); d[1, 3] = bit | keep
                yield f"flag {bit:#x}", (uv, tri_texture, d, texels)

    for size in SIZES:
        for textured in (False, True):
            ref = D.make(abi, size, 0, 4, mesh, debug_mask=abi.DEBUG_HIT_ID)
            app = D.make(abi, size, 0, 4, mesh, debug_mask=abi.DEBUG_HIT_ID)
            if textured:
                for a in (ref, app):
                    T.set_textures(a, *args)
            held = abi.live_device_bytes()
            for what, bad in bad_calls():
                with pytest.raises(abi.RtptError) as e:
                    app.backend.ctx.set_textures(*bad)
                assert e.value.code == abi.RTPT_E_INVALID, what
            assert abi.live_device_bytes() == held
            T.assert_same_frames(T.two_frames(abi, app), T.two_frames(abi, ref), (size, textured))
            ref.backend.close()
            app.backend.close()
    # the given chain that was cut short is accepted with its last texel
    with abi.Context(abi.config_default(64, 48)) as ctx:
        ctx.scene_upload(*mesh)
        ctx.set_textures(uv, np.minimum(tri_texture, 4), desc[:4], texels[:desc[3, 2] + 64 + 16 + 4 + 2 + 1])


# ------------------------------------------------------------------------------------------------ 8. what it is for
def test_minified_checker_stops_shimmering(hip_lib, monkeypatch):
    """a 64 x 64 checker of one-texel cells, bilinear, minified on the quad so that a pixel covers at least 4 x 4 texels
    (asserted: every first-hit lambda >= 2); demodulation, N = 5, frame 8, the default pixel jitter.  RMS of the shaded frame
    against the mean of 256 traced frames of the un-mipped texture, and the mean absolute difference of ALBEDO between frames
    7 and 8: both smaller with RTPT_TEX_MIPMAP than without.  Only the order is asserted.
    Measured on an MI355X: 64 x 48 RMS 0.01313 with mips against 0.04760 without, ALBEDO difference 0.00000 against 0.09964;
    70 x 10 (ten rows, most of the frame sky, whose noise both share) RMS 0.28183 against 0.28332, ALBEDO difference 0.00782
    (pixels on the quad's border, where the jittered ray sometimes meets the sky) against 0.04573."""
    abi = hip_lib
    default = abi.config_default

    def cfg_of(w, h):     # every path is quad then sky; the pixel jitter stays
        cfg = default(w, h)
        cfg.light_radius = 0.0
        return cfg
    monkeypatch.setattr(abi, "config_default", cfg_of)
    tri_uv = (TS.quad_tri_uv() * F32(16)).astype(F32)
    image = MS.checker64()
    for W, H in SIZES:
        app = T.quad_app(abi, (W, H), 0, tri_uv, image, 0, seg=4)
        ctx = app.backend.ctx
        app.updateScene(())
        acc = np.zeros((H, W, 3), np.float64)
        for f in range(256):
            app.pushConstants.frameNumber = 1000 + f
            ctx.raytrace(app.pushConstants)
            acc += ctx.readback(abi.PLANE_IMAGE)[..., :3]
        G = acc / 256
        app.backend.close()
        rms, flicker = {}, {}
        for mip in (MS.MIPMAP, 0):
            app = T.quad_app(abi, (W, H), abi.FLAG_EXT_DEMODULATE, tri_uv, image, mip, seg=4)
            ctx = app.backend.ctx
            if mip:
                ids, lam = ctx.selftest_texture_footprint(MS.pixel_centre_rays((W, H), ctx.cfg.fov_slope, TS.QUAD_CAM), 0)
                assert (ids > 0).sum() >= 0.3 * ids.size and lam[ids > 0].min() >= 2.0, "a pixel covers at least 4 x 4 texels"
            for _ in range(7):
                app.drawScene(())
            alb7 = ctx.readback(abi.PLANE_ALBEDO)[..., :3].astype(np.float64)
            app.drawScene(())
            alb8 = ctx.readback(abi.PLANE_ALBEDO)[..., :3].astype(np.float64)
            out = app.backend.final_image_rows(0, H)[..., :3].astype(np.float64)
            app.backend.close()
            rms[mip] = float(np.sqrt(np.mean((out - G) ** 2)))
            flicker[mip] = float(np.abs(alb8 - alb7).mean())
        print(f"minified checker {W}x{H}: RMS against the 256-frame mean {rms[MS.MIPMAP]:.5f} with mips, {rms[0]:.5f} without; "
              f"mean |ALBEDO(8) - ALBEDO(7)| {flicker[MS.MIPMAP]:.5f} with, {flicker[0]:.5f} without")
        assert rms[MS.MIPMAP] < rms[0]
        assert flicker[MS.MIPMAP] < flicker[0]


# ------------------------------------------------------------------------------------------------ 9. hosts
KEYS = T.KEYS


@pytest.fixture(scope="module")
def room(tmp_path_factory):
    return MS.write_mip_room(str(tmp_path_factory.mktemp("mip_room")))


@pytest.fixture(scope="module")
def serial_host(hip_lib, room):
    """size -> (frames, rays) of the serial Python host with textures=True, texture_mips=True"""
    return {size: T.host_frames(room, size, texture_mips=True) for size in SIZES}


@pytest.mark.parametrize("size", SIZES, ids=T.SIZE_IDS)
def test_python_host_option_is_the_flag(hip_lib, room, serial_host, size):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.textures import load_obj_textures
    t = load_obj_textures(room, mips=True)
    assert (t.textures[:, 3] == MS.MIPMAP).all() and len(t.texels) == 64 * 64 + 33 * 17, "level 0 only: the library generates the chains"
    app = make_app(*size, max_segments=3, iterations=5, scene=room)
    app.backend.ctx.set_materials(t.tri_material, t.materials)
    app.backend.ctx.set_textures(t.tri_uv, t.tri_texture, t.textures, t.texels)
    app.drawScene(())
    assert np.array_equal(bits(app.backend.final_image_rows(0, size[1])), bits(serial_host[size][0][0]))
    app.backend.close()
    plain, _ = T.host_frames(room, size)
    assert not np.array_equal(bits(plain[-1]), bits(serial_host[size][0][-1])), "the room's walls are minified: the chains are read"


@pytest.mark.parametrize("size", SIZES, ids=T.SIZE_IDS)
def test_two_frames_in_flight_equal_the_serial_host(hip_lib, room, serial_host, size):
    frames, rays = T.host_frames(room, size, in_flight=2, texture_mips=True)
    for f in range(len(KEYS)):
        assert np.array_equal(bits(frames[f]), bits(serial_host[size][0][f])), f
    assert rays == serial_host[size][1]


@pytest.mark.parametrize("size", SIZES, ids=T.SIZE_IDS)
def test_cpp_host_equals_the_python_host(hip_lib, room, serial_host, tmp_path, size):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.output import read_pfm
    app_binary = os.path.join(D.PKG, "rtpt_app")
    assert os.path.exists(app_binary), "build() leaves rtpt_app next to the package"
    W, H = size
    pfm = tmp_path / "out.pfm"
    cmd = [app_binary, "--width", str(W), "--height", str(H), "--segments", "3", "--iterations", "5", "--frames", str(len(KEYS)),
           "--script", ",".join(KEYS), "--dump", str(pfm), "--scene", room, "--textures", "--texture-mips"]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    stats = json.loads(out.stdout.strip().splitlines()[-1])
    frames, rays = serial_host[size]
    assert np.array_equal(bits(read_pfm(str(pfm))), bits(np.ascontiguousarray(frames[-1][..., :3])))
    assert stats["rays"] == rays


@pytest.mark.parametrize("mode", ["redundant", "exchange"])
def test_two_strip_contexts_equal_one_context(hip_lib, room, serial_host, tmp_path, mode):
    """two ranks on GPU 0 at 64 x 48, gloo as the carrier (tests/texture_mips_worker.py): the footprint of segment 0 uses the
    FULL frame's height, so every strip equals the single context's rows"""
    W, H = 64, 48
    worker = os.path.join(ROOT, "tests", "texture_mips_worker.py")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), worker, str(tmp_path), mode, ",".join(KEYS), str(W), str(H), room],
                         cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    parts = [np.load(tmp_path / f"w2_r{r}.npz") for r in range(2)]
    frames, rays = serial_host[(W, H)]
    for f in range(len(KEYS)):
        got = np.concatenate([p[f"arr_{f}"] for p in parts], axis=0)
        assert np.array_equal(bits(got), bits(frames[f])), (mode, f)
    assert sum(int(p["rays"][0]) for p in parts) == rays
