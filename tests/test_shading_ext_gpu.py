"""K2 with its three shading extensions — albedo textures (csrc/texture.hpp), mip levels by ray footprint (hit_texture_lod,
tex::sample_lod) and specular bounces (csrc/specular.hpp) — and the ALBEDO plane, whole frames against the oracle's path loop with
the same extensions (oracle_raytrace_ext), bit for bit: IMAGE, HIT_ID, the ray count and, where stored, ALBEDO (same_bits of
filter_planes.py: bits, NaNs by position).  No tolerance appears anywhere.

The scenes (tests/shading_scenes.py) are rooms seen from inside: bounce hits read distinct texels at several levels and meet
diffuse, glossy and mirror surfaces, which constants, closed forms and agreement between schedules cannot tell apart.  What the
oracle's new code states is pinned on the CPU (tests/test_shading_ext_cpu.py), function by function against the numpy
restatements the device is pinned to, and against float64; what the scenes exercise is asserted there on the oracle's dump
(shading_scenes.MEASURED), and again here where a case relies on it.

launch_pathtrace picks the tile kernel from scene mode x DEMOD x TEX x SPEC x {fused, unfused compact, unfused non-compact}, and
k_pathtrace_queue from scene mode x TEX x SPEC: test_every_instantiation is parametrised over (form, TEX, SPEC) and loops over
DEMOD and the launch kinds inside."""
import numpy as np
import pytest

import filter_planes as FP
import pathtrace_scenes as P
import shading_scenes as SS
import test_pathtrace_scenes_gpu as T
from filter_planes import same_bits
from test_gbuffer_scenes_gpu import K012

pytestmark = pytest.mark.gpu

W0, H0 = SS.SHAPES[0]
DEMODULATE = 0x8000
# name -> (flags, environment read by rtpt_create, launches of K012)
KINDS = {k: T.ROUTES[k] for k in ("default", "no_trace_fusion", "no_path_compaction", "single_launch")}
KINDS["window_1"] = (0, {"RTPT_PT_WINDOW": "1"}, (0, 0, 0, 0, 1))      # the queue kernel after every power of two of segments
ENV = ("RTPT_NO_TRACE_FUSION", "RTPT_PT_WINDOW")

_ref_cache = {}


# ------------------------------------------------------------------------------------------ one frame, both sides
def reference(oracle, sh, W, H, segments=SS.SEGMENTS, spp=1, tex=2, spec=True, demod=False, rows=None, textures=None, frame=0, key=()):
    k = (sh.scene.name, sh.scene.form, W, H, segments, spp, tex, spec, demod, rows, frame) + key
    if k not in _ref_cache:
        r = SS.oracle_frame(oracle, sh, W, H, segments, spp, tex, spec, demod, rows, textures, frame, records=False)
        FP.check_ids(r["HIT_ID"], len(sh.scene.tris))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ref_cache[k] = r
    return _ref_cache[k]


def upload(abi, ctx, sh, tex=2, spec=True, textures=None, xforms=None):
    """the scene, its materials (specular ones only with `spec`: otherwise the same table with flags 0) and its textures (tex 0:
    none; 1: the atlas without any mip flag; 2: the mixed atlas; `textures`: another atlas).  An upload drops what the scene before it had"""
    if sh.mesh is not None:
        ctx.scene_upload(sh.mesh[0], sh.mesh[1], sh.xforms if xforms is None else xforms)
    else:
        ctx.scene_upload(*FP.mesh_of(sh.scene.tris))
    ctx.set_materials_ext(sh.scene.tri_material, abi.materials_ext(sh.scene.materials, sh.spec if spec else None))
    if tex:
        ctx.set_textures(sh.tri_uv, sh.tri_texture, *(textures or SS.atlas(sh, tex)))


def context(abi, sh, W, H, segments, flags=0, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, sh.scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def frame(abi, oracle, ctx, sh, W, H, demod, frame_no=0):
    got = T.frame_on_gpu(abi, oracle, ctx, sh.scene, W, H, frame_no)
    if demod:
        got["ALBEDO"] = ctx.readback(abi.PLANE_ALBEDO)
    return got


def compare(got, ref, rows, tag):
    T.compare(got, ref, rows, tag)
    if "ALBEDO" in got:
        y0, y1 = rows or (0, len(ref["ALBEDO"]))
        same_bits(got["ALBEDO"], ref["ALBEDO"][y0:y1], tag + ("ALBEDO",))


def _env(monkeypatch, kind):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in KINDS[kind][1].items():
        monkeypatch.setenv(k, v)


def _check_form(ctx, sh, tag):
    if sh.scene.form != "small":      # more than 64 triangles: the BVH kernels, over pairs or over triangles
        assert bool(ctx.scene_build_info()["leaf_pairs"]) == (sh.scene.form == "pairs"), tag
    else:
        assert len(sh.scene.tris) <= 64, tag


# ------------------------------------------------------------------------------------------ 1. every instantiation
def _scenes(oracle, form, spec):
    names = ("glossy_textured_room", "mirror_corridor", "instanced_pair") if spec else ("textured_room", "mirror_corridor", "instanced_pair")
    return [SS.world(oracle, SS.scene(n, form)) for n in names]


def _budgets(form):
    """the textured or specular hit is the last; 2; one beyond the first window; 9"""
    return sorted({1, 2, P.window_of(None, form) + 1, SS.SEGMENTS})


def _cases(form):
    """(kind, shape, segments, spp, demodulated)"""
    out = []
    for kind in KINDS:
        for segments in _budgets(form):
            if kind == "window_1" and segments == 1:
                continue      # no boundary inside one segment: the default kind's frame
            for demod in (False, True):
                out.append((kind, SS.SHAPES[0], segments, 1, demod))
                if kind == "default":
                    out.append((kind, SS.SHAPES[1], segments, 1, demod))
        # three samples: rtpt_create refuses them only together with RTPT_FLAG_EXT_DEMODULATE, so every kind runs them with the flag
        # off.  Not window_1: launch_pathtrace hands paths to the queue only with one sample, so that would be the default kind again
        if kind != "window_1":
            out += [(kind, SS.SHAPES[0], 1, 3, False), (kind, SS.SHAPES[0], 2, 3, False)]
    return out


@pytest.mark.parametrize("spec", [False, True], ids=["diffuse", "specular"])
@pytest.mark.parametrize("tex", [0, 1, 2], ids=["untextured", "level0", "mips"])
@pytest.mark.parametrize("form", P.FORMS)
def test_every_instantiation(hip_lib, oracle, monkeypatch, form, tex, spec):
    """form: brute force / the BVH over fan pairs / over triangles (asserted on scene_build_info); tex 0: no rtpt_scene_set_textures, 1:
    an atlas without any mip flag, 2: the mixed atlas (TEX == 2 then also meets textures without the flag); spec off:
    rtpt_scene_set_materials_ext with flags 0 on the same scene.  Inside: DEMOD off / on and the launch kinds — fused with K0 / K1,
    RTPT_NO_TRACE_FUSION=1, RTPT_FLAG_NO_PATH_COMPACTION, RTPT_FLAG_SINGLE_LAUNCH_PATHS, and the queue behind the first window and
    behind RTPT_PT_WINDOW=1.  The timing table's launch counts, asserted for every frame, tell the fused tile kernel from the unfused
    one; they do not count k_pathtrace_queue, so that the queue ran rests on the library's rule (one sample, a budget beyond the
    window, no single-launch flag) and on the oracle's paths alive behind the window, asserted here.  Budgets 1, 2, window + 1 and
    9; three samples per pixel at 1 and 2 in every kind that differs from another with them (not with DEMOD: the library refuses)"""
    abi = hip_lib
    scenes = _scenes(oracle, form, spec)
    w = P.window_of(None, form)
    for kind, (W, H), segments, spp, demod in _cases(form):
        flags, _, launches = KINDS[kind]
        _env(monkeypatch, kind)
        with context(abi, scenes[0], W, H, segments, flags | (DEMODULATE if demod else 0), spp) as ctx:
            ctx.timing_enable(1)
            for sh in scenes:
                tag = (kind, sh.scene.name, form, tex, spec, W, H, segments, spp, demod)
                ref = reference(oracle, sh, W, H, segments, spp, tex, spec, demod)
                upload(abi, ctx, sh, tex, spec)
                _check_form(ctx, sh, tag)
                got = frame(abi, oracle, ctx, sh, W, H, demod)
                tm = ctx.timing_collect()      # (collecting empties the table: the counts are this frame's)
                assert tuple(tm[k][1] for k in K012) == launches, (tag, {k: v[1] for k, v in tm.items()})
                compare(got, ref, None, tag)
                if spp == 1 and segments > w and kind != "single_launch":
                    assert P.alive_after(ref["seq_n"], [w])[0] > 0, (tag, "nothing reaches the queue kernel")
                if spp == 1 and segments > 1:
                    assert P.alive_after(ref["seq_n"], [1])[0] > 0, tag
    assert all(s.scene.jitter == scenes[0].scene.jitter and s.scene.light_radius == scenes[0].scene.light_radius for s in scenes), \
        "one context serves the scenes: they share its configuration"


# ------------------------------------------------------------------------------------------ 2. generated and given chains
@pytest.mark.parametrize("form", ["small", "odd"])
def test_generated_and_given_chains(hip_lib, oracle, monkeypatch, form):
    """every texture of the room mip-mapped: the chain the device generates against the oracle fed MS.build_chain's levels; a chain no
    box filter made (every level random), given to both sides"""
    abi = hip_lib
    _env(monkeypatch, "default")
    base = SS.scene("glossy_textured_room", form)
    all_mips = base._replace(tex_flags=tuple(f | SS.MIPMAP for f in base.tex_flags))
    given = SS.given_atlas(base, SS.random_chains(base))
    assert (given[0][:, 3] & SS.MIPS_GIVEN).all() and (SS.atlas(all_mips, 2)[0][:, 3] & (SS.MIPMAP | SS.MIPS_GIVEN) == SS.MIPMAP).all()
    for what, sh, textures in (("generated", all_mips, None), ("given", base, given)):
        for demod in (False, True):
            for segments in (2, SS.SEGMENTS):
                tag = ("chains", what, form, demod, segments)
                ref = reference(oracle, sh, W0, H0, segments, demod=demod, textures=textures, key=(what,))
                with context(abi, sh, W0, H0, segments, DEMODULATE if demod else 0) as ctx:
                    upload(abi, ctx, sh, 2, True, textures)
                    _check_form(ctx, sh, tag)
                    compare(frame(abi, oracle, ctx, sh, W0, H0, demod), ref, None, tag)
    plain = reference(oracle, base, W0, H0, SS.SEGMENTS)
    assert not np.array_equal(plain["IMAGE"], reference(oracle, base, W0, H0, SS.SEGMENTS, textures=given, key=("given",))["IMAGE"])
    assert not np.array_equal(plain["IMAGE"], reference(oracle, all_mips, W0, H0, SS.SEGMENTS, key=("generated",))["IMAGE"])


# ------------------------------------------------------------------------------------------ 3. a strip
@pytest.mark.parametrize("form", ["small", "pairs"])
def test_a_strip_equals_the_rows_of_the_full_frame(hip_lib, oracle, monkeypatch, form):
    """rows [5, 21) of 130 x 33: the footprint of segment 0 uses the FULL frame's height, the stored planes are relative to the first
    stored row, and the counted rays are those rtpt_set_count_rows gives the full frame"""
    abi = hip_lib
    W, H, y0, y1 = P.STRIP
    sh = SS.scene("glossy_textured_room", form)
    for kind in ("default", "window_1"):
        _env(monkeypatch, kind)
        for demod in (False, True):
            tag = ("strip", form, kind, demod)
            full = reference(oracle, sh, W, H, demod=demod)
            counted = reference(oracle, sh, W, H, demod=demod, rows=(y0, y1))["rays"]
            assert 0 < counted < full["rays"]
            with context(abi, sh, W, H, SS.SEGMENTS, DEMODULATE if demod else 0, rows=(y0, y1)) as ctx:
                upload(abi, ctx, sh)
                got = frame(abi, oracle, ctx, sh, W, H, demod)
            compare(got, dict(full, rays=counted), (y0, y1), tag)
            with context(abi, sh, W, H, SS.SEGMENTS, DEMODULATE if demod else 0) as ctx:
                upload(abi, ctx, sh)
                compare(frame(abi, oracle, ctx, sh, W, H, demod), full, None, tag + ("full",))
                ctx.set_count_rows(y0, y1)
                assert frame(abi, oracle, ctx, sh, W, H, demod)["rays"] == counted, tag


# ------------------------------------------------------------------------------------------ 4. moved instances
@pytest.mark.parametrize("flags", [0, 0x7000], ids=["host", "device"])
@pytest.mark.parametrize("form", ["small", "odd"])
def test_moved_instances(hip_lib, oracle, monkeypatch, form, flags):
    """instanced_pair after rtpt_scene_set_instances with other transforms, flattened, posed and refit on the host (RTPT_HOST_REFIT=1)
    and, with 0x7000 (the device builder with RTPT_FLAG_DEVICE_FLATTEN), on the device — rtpt_debug_upload_info says which: the upload
    of the small form is flattened on the host under either, its move follows the flags like the other form's — against the oracle's frame of the re-flattened triangles: the uv, texture and material
    records stay those of the base mesh, the density follows the posed triangles"""
    abi = hip_lib
    _env(monkeypatch, "default")
    monkeypatch.setenv("RTPT_HOST_REFIT", "0" if flags else "1")
    first = SS.world(oracle, SS.scene("instanced_pair", form))
    moved = SS.world(oracle, first, SS.box_xforms(moved=True))
    for demod in (False, True):
        for segments in (2, SS.SEGMENTS):
            with context(abi, first, W0, H0, segments, flags | (DEMODULATE if demod else 0)) as ctx:
                upload(abi, ctx, first)
                if form != "small":
                    assert not ctx.scene_build_info()["leaf_pairs"]
                    assert ctx.debug_upload_info()["device_flatten"] == int(bool(flags))
                else:      # at most 64 triangles: the upload is flattened on the host whatever the flags
                    assert ctx.debug_upload_info()["device_flatten"] == 0
                tag = ("moved", form, flags, demod, segments)
                compare(frame(abi, oracle, ctx, first, W0, H0, demod), reference(oracle, first, W0, H0, segments, demod=demod), None, tag + (0,))
                ctx.end_frame()
                ctx.scene_set_instances(moved.xforms)
                assert ctx.debug_upload_info()["device_flatten"] == int(bool(flags)), tag
                ref = reference(oracle, moved, W0, H0, segments, demod=demod, frame=1, key=("moved",))
                compare(frame(abi, oracle, ctx, moved, W0, H0, demod, 1), ref, None, tag + (1,))
    assert not np.array_equal(ref["HIT_ID"], reference(oracle, first, W0, H0, SS.SEGMENTS, demod=True)["HIT_ID"])


# ------------------------------------------------------------------------------------------ 5. preconditions
@pytest.mark.parametrize("form", P.FORMS)
@pytest.mark.parametrize("name", SS.SCENES)
def test_preconditions_hold_on_the_oracles_dump(oracle, name, form):
    """what the comparisons above rely on, counted by the oracle on the CPU (never by the GPU): conditions, not tolerances"""
    sh = SS.world(oracle, SS.scene(name, form))
    got = SS.counts(oracle, sh, SS.oracle_frame(oracle, sh, W0, H0), P.window_of(None, form))
    for k in SS.REQUIRED[name]:
        m = SS.MEASURED[name, form][k]
        assert m > 0 and got[k] >= max(1, (m + 1) // 2), (name, form, k, got[k], m)
    assert got["lod_levels"] >= SS.MIN_LOD_LEVELS and got["lod_fraction"] > 0
    assert got["albedos"] > len(sh.scene.materials)
