"""Every dielectric and light-sampling tile kernel of K2 against one walker, whole frames bit for bit: IMAGE, HIT_ID, the ray count
and, with RTPT_FLAG_EXT_DEMODULATE, ALBEDO (same_bits of filter_planes.py: bits, NaNs by position).  No tolerance appears anywhere.

launch_pathtrace picks the tile kernel from scene mode (3) x DEMOD (2) x TEX (3) x SPEC (7) x {fused, unfused compact, unfused
non-compact}, and k_pathtrace_queue from scene mode x TEX x SPEC 0 .. 2.  tests/test_shading_ext_gpu.py covers SPEC 0 and 1 cell by
cell against the C oracle, which knows neither glass nor a light sample; this file covers SPEC 2 .. 6 the same way against the walker
of tests/path_walker.py, which tests/test_lattice_cpu.py holds to that oracle (SPEC 0 / 1), to the older walkers (level 0) and to
float64.  The scenes (tests/lattice_scenes.py) put mip-mapped, textured hits inside and behind glass and take light samples of
every kind at textured hits, so that a wrong level, a wrong texel in ALBEDO or a gain demodulated twice shows in the bits.

Which axis value each parameter and loop reaches:

  scene mode   `form`: small = brute force, pairs = the BVH over fan pairs, odd = the BVH over triangles (asserted on
               rtpt_scene_build_info's leaf_pairs, and on the triangle count of the small form)
  TEX          `tex`: 0 no rtpt_scene_set_textures, 1 the atlas without any mip flag, 2 the mixed atlas with generated chains
               (textures without the flag among them)
  SPEC         `spec`: 2 rtpt_scene_set_materials_ext with the glass and the glossy materials and no sampling flag; 3 / 4 / 5 / 6 the
               same upload under 0x10000 / 0x30000 / 0x50000 / 0x70000 (asserted on rtpt_debug_light_list, and for 5 / 6 on
               rtpt_debug_light_table); "4-without-list" 0x20000 on a scene without a material table: the SPEC 4 kernels with an
               empty list and the normal-keyed colours
  DEMOD        inside every test: off and on
  launch kind  inside test_every_cell: fused with K0 / K1 (default), RTPT_NO_TRACE_FUSION=1 (unfused, compacting),
               RTPT_FLAG_NO_PATH_COMPACTION (unfused, not compacting) — told apart by the timing table's launch counts, asserted
               for every frame; for SPEC 2 also RTPT_FLAG_SINGLE_LAUNCH_PATHS and the queue behind the first window and behind
               RTPT_PT_WINDOW=1 (k_pathtrace_queue: scene mode x TEX x SPEC 2; the walker's paths alive behind the window are
               asserted).  A launch that samples lights takes no queue: the single-launch flag changes nothing there, asserted
               once per form
  budgets      1, 2 and 9 (SPEC 2: also one beyond the form's first window); three samples per pixel at 1 and 2, DEMOD off (the
               library refuses the two together); 96 x 12 everywhere and 97 x 13 in the default kind

Both scenes run in every cell; lattice_instances reads material, texture and light records through % n_base_tris.  Beside the
cells: a strip context and moved instances (device flatten) per form and spec."""
import numpy as np
import pytest

import filter_planes as FP
import path_walker as WK
import lattice_scenes as LS
import pathtrace_scenes as P
import shading_scenes as SS
import test_pathtrace_scenes_gpu as T
from filter_planes import same_bits
from test_gbuffer_scenes_gpu import K012

pytestmark = pytest.mark.gpu

W0, H0 = LS.SHAPES[0]
DEMODULATE, SINGLE_LAUNCH, DEVICE_FLATTEN = 0x8000, 0x200, 0x7000
# name -> (flags, environment read by rtpt_create, launches of K012)
KINDS = {k: T.ROUTES[k] for k in ("default", "no_trace_fusion", "no_path_compaction", "single_launch")}
KINDS["window_1"] = (0, {"RTPT_PT_WINDOW": "1"}, (0, 0, 0, 0, 1))      # the queue kernel after every power of two of segments
SAMPLING_KINDS = ("default", "no_trace_fusion", "no_path_compaction")
ENV = ("RTPT_NO_TRACE_FUSION", "RTPT_PT_WINDOW")
STRIP = (96, 24, 5, 21)                       # W, H and the stored rows

_ref_cache = {}
_case_cache = {}


# ------------------------------------------------------------------------------------------ one frame, both sides
def case(oracle, name, form, moved=False):
    k = (name, form, moved)
    if k not in _case_cache:
        _case_cache[k] = LS.case(oracle, name, form, SS.box_xforms(moved=True) if moved else None)
    return _case_cache[k]


def reference(oracle, c, W, H, tex, spec, segments=LS.SEGMENTS, spp=1, demod=False, rows=None, frame=0, key=()):
    """the walker's frame, computed once, shared by all launch kinds and left unchanged"""
    sc = c.sh.scene
    k = (sc.name, sc.form, tex, spec, segments, spp, demod, W, H, rows, frame) + key
    if k not in _ref_cache:
        r = WK.walk(oracle, sc, W, H, segments, spp=spp, tex=WK.textures(c.sh, tex), demod=demod, rows=rows, frame=frame, **LS.setup(oracle, c, spec))
        FP.check_ids(r["HIT_ID"], len(sc.tris))
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ref_cache[k] = r
    return _ref_cache[k]


def upload(abi, ctx, c, tex, spec, xforms=None):
    """the scene, its materials — glass and glossy ones through rtpt_scene_set_materials_ext; none at all for "4-without-list" —
    and its textures.  An upload drops what the scene before it had"""
    sh = c.sh
    if sh.mesh is not None:
        ctx.scene_upload(sh.mesh[0], sh.mesh[1], sh.xforms if xforms is None else xforms)
    else:
        ctx.scene_upload(*FP.mesh_of(sh.scene.tris))
    if spec != "4-without-list":
        ctx.set_materials_ext(sh.scene.tri_material, abi.materials_ext(sh.scene.materials, sh.spec, c.glass))
    if tex:
        ctx.set_textures(sh.tri_uv, sh.tri_texture, *SS.atlas(sh, tex))


def context(abi, c, W, H, segments, flags=0, spp=1, rows=None):
    ctx = abi.Context(T._config(abi, c.sh.scene, W, H, segments, spp, flags, rows))
    ctx.enable_debug(abi.DEBUG_HIT_ID)
    return ctx


def frame(abi, oracle, ctx, c, W, H, demod, frame_no=0):
    got = T.frame_on_gpu(abi, oracle, ctx, c.sh.scene, W, H, frame_no)
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


def check_scene_state(oracle, ctx, c, spec, tag):
    """the form's kernels, and the list and the table the SPEC's kernels read"""
    sc = c.sh.scene
    if sc.form != "small":      # more than 64 triangles: the BVH kernels, over pairs or over triangles
        assert bool(ctx.scene_build_info()["leaf_pairs"]) == (sc.form == "pairs"), tag
    else:
        assert len(sc.tris) <= 64, tag
    s = LS.setup(oracle, c, spec)
    got = ctx.debug_light_list()
    assert np.array_equal(got, s["lights"]), tag
    assert (len(got) > 0) == (spec in (3, 4, 5, 6)), tag
    table = ctx.debug_light_table()
    if spec in (5, 6):
        assert table.dtype == np.uint64 and np.array_equal(table, LS.table(oracle, c)), tag
    else:
        assert len(table) == 0, tag


def check_reference(ref, c, spec, segments, spp, window, queue, tag):
    """what a case relies on, counted by the walker on the CPU"""
    if spp != 1:
        return
    if segments > 1:
        assert P.alive_after(ref["seq_n"], [1])[0] > 0, tag
    if queue and segments > window:
        assert P.alive_after(ref["seq_n"], [window])[0] > 0, (tag, "nothing reaches the queue kernel")
    if segments == LS.SEGMENTS:
        if spec != "4-without-list":
            assert ref["transmitted"] > 0 and ref["reflected"] > 0, tag
        if spec in (3, 4, 5, 6):
            assert ref["lit"] > 0 and ref["queries"] > ref["lit"] and ref["kept"] > 0 and ref["dropped"] > 0, tag
        if spec in (4, 6, "4-without-list"):
            assert ref["sphere_valid"] > 0 and ref["sphere_dropped"] > 0, tag
            # (without a table every hit is diffuse and samples the sphere: hardly a path meets it with the bit clear)
            assert ref["sphere_kept"] > 0 or spec == "4-without-list", tag


# ------------------------------------------------------------------------------------------ 1. every cell
def _budgets(form, spec):
    """the textured, dielectric or sampling hit is the last; 2; (where a queue follows) one beyond the first window; 9"""
    return sorted({1, 2, LS.SEGMENTS} | ({P.window_of(None, form) + 1} if spec == 2 else set()))


def _cases(form, spec):
    """(kind, shape, segments, spp, demodulated)"""
    out = []
    for kind in (KINDS if spec == 2 else SAMPLING_KINDS):
        for segments in _budgets(form, spec):
            if kind == "window_1" and segments == 1:
                continue      # no boundary inside one segment: the default kind's frame
            for demod in (False, True):
                out.append((kind, LS.SHAPES[0], segments, 1, demod))
                if kind == "default":
                    out.append((kind, LS.SHAPES[1], segments, 1, demod))
        if kind != "window_1":      # (the queue takes paths only with one sample: that would be the default kind again)
            out += [(kind, LS.SHAPES[0], 1, 3, False), (kind, LS.SHAPES[0], 2, 3, False)]
    return out


@pytest.mark.parametrize("spec", LS.SPECS, ids=[str(s) for s in LS.SPECS])
@pytest.mark.parametrize("tex", [0, 1, 2], ids=["untextured", "level0", "mips"])
@pytest.mark.parametrize("form", P.FORMS)
def test_every_cell(hip_lib, oracle, monkeypatch, form, tex, spec):
    """see the module text for what form, tex and spec select.  Inside: both scenes, DEMOD off / on, the launch kinds, the budgets,
    both shapes and three samples per pixel; per frame IMAGE, HIT_ID, the ray count and ALBEDO against the walker bit for bit, the
    timing table's launch counts (they tell the fused tile kernel from the unfused one; they do not count k_pathtrace_queue, so that
    the queue ran rests on the library's rule — one sample, a budget beyond the window, no single-launch flag, no light sampling —
    and on the walker's paths alive behind the window, asserted here), the form, the light list and the table"""
    abi = hip_lib
    cases = [case(oracle, n, form) for n in LS.SCENES]
    w = P.window_of(None, form)
    for kind, (W, H), segments, spp, demod in _cases(form, spec):
        flags, _, launches = KINDS[kind]
        _env(monkeypatch, kind)
        with context(abi, cases[0], W, H, segments, flags | LS.SPEC_FLAGS[spec] | (DEMODULATE if demod else 0), spp) as ctx:
            ctx.timing_enable(1)
            for c in cases:
                tag = (kind, c.sh.scene.name, form, tex, spec, W, H, segments, spp, demod)
                ref = reference(oracle, c, W, H, tex, spec, segments, spp, demod)
                upload(abi, ctx, c, tex, spec)
                check_scene_state(oracle, ctx, c, spec, tag)
                got = frame(abi, oracle, ctx, c, W, H, demod)
                tm = ctx.timing_collect()      # (collecting empties the table: the counts are this frame's)
                assert tuple(tm[k][1] for k in K012) == launches, (tag, {k: v[1] for k, v in tm.items()})
                compare(got, ref, None, tag)
                check_reference(ref, c, spec, segments, spp, w, spec == 2 and kind != "single_launch", tag)
    assert all(c.sh.scene.jitter == cases[0].sh.scene.jitter and c.sh.scene.light_radius == cases[0].sh.scene.light_radius for c in cases), \
        "one context serves the scenes: they share its configuration"


# ------------------------------------------------------------------------------------------ 2. the single-launch flag where lights are sampled
@pytest.mark.parametrize("form", P.FORMS)
def test_single_launch_flag_changes_nothing_where_lights_are_sampled(hip_lib, oracle, monkeypatch, form):
    """a sampling launch runs every segment in the tile kernel: with RTPT_FLAG_SINGLE_LAUNCH_PATHS it is the default kind's frame,
    with the default kind's launch counts (SPEC 6, the mixed atlas, DEMOD off / on, 9 segments)"""
    abi = hip_lib
    _env(monkeypatch, "default")
    for c in [case(oracle, n, form) for n in LS.SCENES]:
        for demod in (False, True):
            tag = ("single launch", c.sh.scene.name, form, demod)
            ref = reference(oracle, c, W0, H0, 2, 6, demod=demod)
            with context(abi, c, W0, H0, LS.SEGMENTS, SINGLE_LAUNCH | LS.SPEC_FLAGS[6] | (DEMODULATE if demod else 0)) as ctx:
                ctx.timing_enable(1)
                upload(abi, ctx, c, 2, 6)
                got = frame(abi, oracle, ctx, c, W0, H0, demod)
                tm = ctx.timing_collect()
            assert tuple(tm[k][1] for k in K012) == KINDS["default"][2], (tag, {k: v[1] for k, v in tm.items()})
            compare(got, ref, None, tag)


# ------------------------------------------------------------------------------------------ 3. a strip
@pytest.mark.parametrize("spec", LS.SPECS, ids=[str(s) for s in LS.SPECS])
@pytest.mark.parametrize("form", P.FORMS)
def test_a_strip_equals_the_rows_of_the_full_frame(hip_lib, oracle, monkeypatch, form, spec):
    """rows [5, 21) of 96 x 24, the mixed atlas, DEMOD on: the footprint of segment 0 uses the FULL frame's height, the stored
    planes (ALBEDO too) are relative to the first stored row, and the counted rays are the strip's"""
    abi = hip_lib
    _env(monkeypatch, "default")
    W, H, y0, y1 = STRIP
    c = case(oracle, "lattice_room", form)
    full = reference(oracle, c, W, H, 2, spec, demod=True)
    counted = reference(oracle, c, W, H, 2, spec, demod=True, rows=(y0, y1))["rays"]
    assert 0 < counted < full["rays"]
    with context(abi, c, W, H, LS.SEGMENTS, LS.SPEC_FLAGS[spec] | DEMODULATE, rows=(y0, y1)) as ctx:
        upload(abi, ctx, c, 2, spec)
        check_scene_state(oracle, ctx, c, spec, ("strip", form, spec))
        got = frame(abi, oracle, ctx, c, W, H, True)
    compare(got, dict(full, rays=counted), (y0, y1), ("strip", form, spec))


# ------------------------------------------------------------------------------------------ 4. moved instances
@pytest.mark.parametrize("spec", LS.SPECS[1:], ids=[str(s) for s in LS.SPECS[1:]])
@pytest.mark.parametrize("form", ["small", "odd"])
def test_moved_instances(hip_lib, oracle, monkeypatch, form, spec):
    """lattice_instances after rtpt_scene_set_instances with other transforms under the device builder with
    RTPT_FLAG_DEVICE_FLATTEN (0x7000), the mixed atlas, DEMOD off / on: the frame against the walker on the re-posed triangles — the
    uv, texture, material and light records stay the base mesh's — and for SPEC 5 / 6 the table rebuilt on the posed triangles"""
    abi = hip_lib
    _env(monkeypatch, "default")
    first, moved = case(oracle, "lattice_instances", form), case(oracle, "lattice_instances", form, moved=True)
    assert not np.array_equal(moved.sh.scene.tris, first.sh.scene.tris)
    for demod in (False, True):
        with context(abi, first, W0, H0, LS.SEGMENTS, DEVICE_FLATTEN | LS.SPEC_FLAGS[spec] | (DEMODULATE if demod else 0)) as ctx:
            upload(abi, ctx, first, 2, spec)
            tag = ("moved", form, spec, demod)
            check_scene_state(oracle, ctx, first, spec, tag + (0,))
            compare(frame(abi, oracle, ctx, first, W0, H0, demod), reference(oracle, first, W0, H0, 2, spec, demod=demod), None, tag + (0,))
            ctx.end_frame()
            ctx.scene_set_instances(moved.sh.xforms)
            assert ctx.debug_upload_info()["device_flatten"] == 1, tag
            check_scene_state(oracle, ctx, moved, spec, tag + (1,))
            ref = reference(oracle, moved, W0, H0, 2, spec, demod=demod, frame=1, key=("moved",))
            compare(frame(abi, oracle, ctx, moved, W0, H0, demod, 1), ref, None, tag + (1,))
    assert not np.array_equal(ref["HIT_ID"], reference(oracle, first, W0, H0, 2, spec, demod=True)["HIT_ID"])
