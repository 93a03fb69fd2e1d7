"""The deferred final filter pass (include/rtpt.h: rtpt_debug_defer_info): a final pass that qualifies is prepared where
it is recorded and launched inside the next frame's tracing launch, or alone by whatever entry point would see the difference.
Every check here renders one frame sequence twice — in a default context and with RTPT_NO_FINAL_DEFER=1 — and asks for equal
bits in every readable plane, equal ray counts and equal reuse counters.

Which passes are deferred: the id-pair final pass that LOADS its reprojected pixels, i.e. from the fourth frame at rest on (the
reprojection is keyed on planes that frame reuse knows the content of, which it does from the third frame on: that one stores,
the next loads); which are launched inside a trace: those followed by an rtpt_raytrace with K0 and K1 served from the planes,
one sample per pixel, over all stored rows.  Eight frames at rest therefore record five passes (frames 3 to 7), launch four
inside the traces of frames 4 to 7 and leave the last to the first observer."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

SEG = 4
REST8 = [()] * 8
RECORDED8, IN_TRACE8 = 5, 4   # of REST8, see above


def _planes(P):
    return (P.PLANE_IMAGE, P.PLANE_FILTERED, P.PLANE_PREVIOUS, P.PLANE_WORLDPOS, P.PLANE_GRADIENT, P.PLANE_DEPTH, P.PLANE_VIS_ID,
            P.PLANE_PREV_VIS_ID, P.PLANE_LUT, P.PLANE_LUT_PREV)


def _contexts(app):
    be = app.backend
    return [b.ctx for b in be.be] if hasattr(be, "be") else [be.ctx]


def _observe(P, app):
    return [c.readback(p) for c in _contexts(app) for p in _planes(P)] + [np.array([c.raycount() for c in _contexts(app)], np.uint64)]


def _pending(ctx):
    d = ctx.defer_info()
    return d["recorded"] - d["launched_in_trace"] - d["launched_alone"]


def _run(P, monkeypatch, defer, size=(200, 83), n=5, script=REST8, every_frame=False, between=None, env=(), close_early=False, **kw):
    """-> (observations, counters).  between = (frame, fn): fn(app, ctx) runs after that many frames ended, before the next
    frame's passes, with a final pass pending in a deferring context; what it returns is the first observation"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    monkeypatch.setenv("RTPT_NO_FINAL_DEFER", "0" if defer else "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    kw.setdefault("max_segments", SEG)
    app = make_app(size[0], size[1], iterations=n, **kw)
    seen = []
    for f, keys in enumerate(script):
        ctx = app.backend.ctx
        if between and between[0] == f:
            if defer:
                assert _pending(ctx) == 1, "no final pass is pending where the entry point under test is called"
            seen.append(between[1](app, ctx))
            assert _pending(ctx) == 0 or isinstance(seen[-1], str)   # (a call refused for its arguments looked at nothing)
        app.updateScene(keys)
        app.drawVisbilityBuffer()
        app.computeTemporalGradient()
        app.drawSceneToImage()
        app.applyTemporalFiltering()
        app.copyImageToSwapChainsCurrentImage()
        app.frameCount += 1
        if every_frame:
            seen.append(_observe(P, app))
    info = None
    if close_early:  # rtpt_destroy with the last pass still pending
        info = [(c.defer_info(),) for c in _contexts(app)]
    else:
        seen.append(_observe(P, app))
        info = [(c.defer_info(), c.reuse_info(), c.reproj_info()) for c in _contexts(app)]
    app.backend.close()
    for o in getattr(app, "_kept", []):
        if hasattr(o, "close"):
            o.close()
    return seen, info


def _flat(x):
    if isinstance(x, (list, tuple)):
        return [y for v in x for y in _flat(v)]
    return [x]


def _same(a, b):
    a, b = _flat(a), _flat(b)
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.dtype == y.dtype, f"observation {i}"
            assert np.array_equal(bits(x) if x.dtype.itemsize == 4 else x, bits(y) if y.dtype.itemsize == 4 else y), f"observation {i} differs"
        else:
            assert x == y, f"observation {i}: {x!r} != {y!r}"


def _both(P, monkeypatch, **kw):
    on, info = _run(P, monkeypatch, True, **kw)
    off, info_off = _run(P, monkeypatch, False, **kw)
    _same(on, off)
    for (d, *rest), (d_off, *rest_off) in zip(info, info_off):
        assert rest == rest_off, "reuse / reprojection counters differ"
        assert d_off == dict(recorded=0, launched_in_trace=0, launched_alone=0, spare_bytes=0)
        assert d["recorded"] == d["launched_in_trace"] + d["launched_alone"]
    return [i[0] for i in info]


# the comb kernel's edges: a width that is no multiple of 64, heights below and just above one chunk group (40 rows at k = 5),
# a single tile
@pytest.mark.parametrize("size", [(200, 37), (257, 83), (64, 4)])
def test_eight_frames_at_rest_seen_after_the_last(hip_lib, monkeypatch, size):
    d, = _both(hip_lib, monkeypatch, size=size)
    print(size, d)
    assert d["recorded"] == RECORDED8 and d["launched_in_trace"] == IN_TRACE8 and d["launched_alone"] == 1
    assert d["spare_bytes"] == size[0] * size[1] * 16


# N = 1, 3: the final pass at k = 1, 3; N = 9: its halo does not fit the tracing launch's LDS — launched where it is recorded
@pytest.mark.parametrize("n", [1, 3, 9])
def test_other_iteration_counts(hip_lib, monkeypatch, n):
    d, = _both(hip_lib, monkeypatch, n=n)
    print(n, d)
    if n == 9:
        assert d["recorded"] == 0
    else:
        assert d["launched_in_trace"] >= 4


def test_eight_frames_at_rest_seen_after_every_frame(hip_lib, monkeypatch):
    d, = _both(hip_lib, monkeypatch, every_frame=True)
    assert d["launched_in_trace"] == 0 and d["launched_alone"] == d["recorded"] == RECORDED8


def test_seen_and_unseen_sequences_are_the_same_frames(hip_lib, monkeypatch):
    seen, _ = _run(hip_lib, monkeypatch, True, every_frame=True)
    unseen, _ = _run(hip_lib, monkeypatch, True)
    _same(seen[-1], unseen[-1])


# ---- one case per entry point that sends the pending pass out, called between rtpt_end_frame and the next frame's passes
def _try(fn):
    try:
        return fn()
    except Exception as e:  # the same refusal in both contexts is the same outcome
        return f"{type(e).__name__}: {e}"


def _device_buffer(app, nbytes, dtype="uint8"):
    import torch
    t = torch.zeros(nbytes, dtype=getattr(torch, dtype), device="cuda")
    torch.cuda.synchronize()
    app._kept = getattr(app, "_kept", []) + [t]   # outlives the context's use of it
    return t


def _e_sync(P, app, ctx):
    ctx.sync()


def _e_readback(P, app, ctx):
    return [ctx.readback(p) for p in (P.PLANE_IMAGE, P.PLANE_PREVIOUS, P.PLANE_FILTERED)]


def _e_plane_ptr(P, app, ctx):
    assert ctx.plane_ptr(P.PLANE_PREVIOUS) != 0   # (the caller checks that nothing is pending behind it)


def _e_bind_plane(P, app, ctx):
    t = _device_buffer(app, ctx.plane_bytes(P.PLANE_FILTERED))
    ctx.bind_plane(P.PLANE_FILTERED, t.data_ptr(), t.numel())


def _e_set_plane(P, app, ctx):
    n = ctx.plane_bytes(P.PLANE_PREVIOUS) // 4
    ctx.set_plane(P.PLANE_PREVIOUS, np.random.default_rng(5).random(n, dtype=np.float32))


def _e_set_stream(P, app, ctx):
    import torch
    s = torch.cuda.Stream()
    app._kept = getattr(app, "_kept", []) + [s]
    ctx.set_stream(s.cuda_stream)


def _e_stream_wait(P, app, ctx):
    other = P.Context(P.config_default(64, 8))
    app._kept = getattr(app, "_kept", []) + [other]
    ctx.stream_wait(other)


def _e_stream_wait_other(P, app, ctx):
    other = P.Context(P.config_default(64, 8))
    app._kept = getattr(app, "_kept", []) + [other]
    other.stream_wait(ctx)


def _e_resize(P, app, ctx):
    ctx.resize(app.backend.width, app.backend.height)


def _e_present(P, app, ctx):
    t = _device_buffer(app, app.backend.width * app.backend.height * 4)
    ctx.present(t.data_ptr())
    ctx.sync()
    return t.cpu().numpy()


def _e_present_target(P, app, ctx):
    t = _device_buffer(app, app.backend.width * app.backend.height * 4)
    ctx.present_target(t.data_ptr())


def _e_modulate(P, app, ctx):
    return _try(lambda: ctx.modulate())


def _e_external_history(P, app, ctx):
    ctx.set_external_history(None)


def _e_external_guides(P, app, ctx):
    ctx.set_external_guides(None, None)


def _e_scene_upload(P, app, ctx):
    app.buildAccelerationStructure()


def _e_scene_rebuild(P, app, ctx):
    return _try(lambda: ctx.scene_rebuild())


def _e_scene_instances(P, app, ctx):
    return _try(lambda: ctx.scene_set_instances(np.eye(4, dtype=np.float32)[None, :3, :]))


def _e_materials(P, app, ctx):
    return _try(lambda: ctx.set_materials(None, None))


def _e_textures(P, app, ctx):
    return _try(lambda: ctx.set_textures())


def _e_enable_debug(P, app, ctx):
    ctx.enable_debug(P.DEBUG_HIT_ID)


def _e_timing_collect(P, app, ctx):
    ctx.timing_collect()


def _e_gbuffer_alone(P, app, ctx):
    # rtpt_gbuffer followed by something else than rtpt_temporal_gradient: K0 is launched, behind the pending pass
    app.updateUBO()
    ctx.gbuffer(app.ubo)
    return [ctx.readback(p) for p in (P.PLANE_VIS_ID, P.PLANE_PREVIOUS)]


ENTRY_POINTS = [_e_sync, _e_readback, _e_plane_ptr, _e_bind_plane, _e_set_plane, _e_set_stream, _e_stream_wait, _e_stream_wait_other,
                _e_resize, _e_present, _e_present_target, _e_modulate, _e_external_history, _e_external_guides, _e_scene_upload,
                _e_scene_rebuild, _e_scene_instances, _e_materials, _e_textures, _e_enable_debug, _e_timing_collect, _e_gbuffer_alone]


@pytest.mark.parametrize("entry", ENTRY_POINTS, ids=lambda e: e.__name__[3:])
def test_entry_point_sends_the_pending_pass_out_first(hip_lib, monkeypatch, entry):
    d, = _both(hip_lib, monkeypatch, between=(6, lambda app, ctx: entry(hip_lib, app, ctx)))
    assert d["launched_alone"] >= 1 and d["launched_in_trace"] >= 2


def test_destroy_with_a_pass_pending(hip_lib, monkeypatch):
    before = hip_lib.live_device_bytes()
    _, info = _run(hip_lib, monkeypatch, True, close_early=True)
    d = info[0][0]
    assert d["recorded"] == RECORDED8 and d["launched_in_trace"] == IN_TRACE8 and d["launched_alone"] == 0 and d["spare_bytes"] == 200 * 83 * 16
    assert hip_lib.live_device_bytes() == before


def test_context_that_never_defers_has_three_colour_buffers(hip_lib, monkeypatch):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    sizes = []
    for defer, frames in ((False, 6), (True, 6), (True, 3)):
        monkeypatch.setenv("RTPT_NO_FINAL_DEFER", "0" if defer else "1")
        before = hip_lib.live_device_bytes()
        app = make_app(200, 83, max_segments=SEG, iterations=5)
        app.run(frames)
        app.backend.ctx.sync()
        sizes.append(hip_lib.live_device_bytes() - before)
        app.backend.close()
    assert sizes[1] - sizes[0] == 200 * 83 * 16 and sizes[2] == sizes[0]


# a camera key and a light key in the middle: K0 / K1 join the trace, the pending pass goes out alone; then rest again
def test_camera_and_light_keys(hip_lib, monkeypatch):
    script = [(), (), (), (), ("D",), (), (), (), (), ("J",), (), (), (), ()]
    d, = _both(hip_lib, monkeypatch, script=script)
    print(d)
    assert d["launched_alone"] >= 3 and d["launched_in_trace"] >= 3


@pytest.mark.parametrize("case", ["spp4", "one_segment", "queue_window"])
def test_other_tracing_kernels(hip_lib, monkeypatch, case):
    kw = dict(spp4=dict(samples_per_pixel=4), one_segment=dict(max_segments=1), queue_window=dict(env=(("RTPT_PT_WINDOW", "2"),)))[case]
    d, = _both(hip_lib, monkeypatch, **kw)
    print(case, d)
    assert d["recorded"] == RECORDED8
    if case == "spp4":   # the tile kernel keeps its accumulators in LDS: it carries no pass
        assert d["launched_in_trace"] == 0
    else:
        assert d["launched_in_trace"] == IN_TRACE8


def test_strip_context(hip_lib, monkeypatch):
    d, = _both(hip_lib, monkeypatch, size=(200, 120), rank=1, world=3, mode="redundant", torch_planes=False)
    print(d)
    assert d["recorded"] == d["launched_in_trace"] + d["launched_alone"]


def test_two_contexts_alternating(hip_lib, monkeypatch):
    _both(hip_lib, monkeypatch, frames_in_flight=2)


def test_front_share_changes_no_bit(hip_lib, monkeypatch):
    ref, _ = _run(hip_lib, monkeypatch, False, size=(257, 83))
    for front in ("0", "1", "2", "1,25", "2,75", "7,100"):
        got, info = _run(hip_lib, monkeypatch, True, size=(257, 83), env=(("RTPT_FINAL_FRONT", front),))
        _same(got, ref)
        assert info[0][0]["launched_in_trace"] == IN_TRACE8, front
