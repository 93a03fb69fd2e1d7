"""Sequences of ABI calls that exercise the per-frame state of the context (csrc/api_internal.hpp: FrameState) and the plan of
a filter launch (csrc/api_passes.hip: plan_filter / commit_filter): which buffer plays which role after a pass, which rows of
it hold the finished frame, what a resize forgets, and how the recorded iterations are grouped into launches.  Every pixel
comparison is bit for bit; the launch tables are what the timing hooks count per frame."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

KERNELS = ("k_atrous", "k_atrous_final", "k_atrous_chain", "k_atrous_chain_final", "k_gbuffer_pathtrace")
KEYS = [(), ("J",), ("D",)]      # the light moves before the second frame, the camera before the third
SMALL = (65, 7)                  # the smallest size test_chain_gpu.py chains at: one full wave plus a pixel, both row clamps


def _app(hip_lib, size, n, flags=0, seg=3, **kw):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    app = make_app(size[0], size[1], max_segments=seg, iterations=n, flags=flags, **kw)
    app.backend.ctx.timing_enable(1)
    return app


def _trace(app, keys):
    app.updateScene(keys)
    app.drawVisbilityBuffer()
    app.computeTemporalGradient()
    app.drawSceneToImage()


def _filter(app, k, n, y0=0, y1=0):
    pc = app.pushConstants
    pc.maxWaveletIteration, pc.waveletIteration = n, k
    app.backend.temporal_filter(pc, app.ubo, y0, y1)


def _finish(app):
    app.copyImageToSwapChainsCurrentImage()   # rtpt_end_frame
    app.frameCount += 1


def _colour(hip_lib, ctx):
    return [ctx.readback(p) for p in (hip_lib.PLANE_IMAGE, hip_lib.PLANE_FILTERED, hip_lib.PLANE_PREVIOUS)]


def _launches(ctx, names=KERNELS):
    tm = ctx.timing_collect()
    return tuple(tm[n][1] for n in names)


def _same(a, b, tag):
    assert len(a) == len(b)
    for p, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (tag, p)


# ------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("chain", [0, 1])
@pytest.mark.parametrize("exact", [0, 1])
def test_final_pass_in_two_row_ranges(hip_lib, monkeypatch, exact, chain):
    """the final pass over rows [0, 15) and again over [15, 33) — row 15 splits a 4-row tile, 130 columns leave a ragged 64-column
    tile — leaves every colour role and the finished frame as one call over the whole frame does; between the two calls only
    the first range is a finished frame"""
    import torch
    if chain:
        monkeypatch.setenv("RTPT_CHAIN_MIN_PIXELS", "0")
    w, h, n, cut = 130, 33, 5, 15
    flags = hip_lib.FLAG_EXACT_FILTER if exact else 0
    a, b = _app(hip_lib, (w, h), n, flags, seg=4), _app(hip_lib, (w, h), n, flags, seg=4)
    img = torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for f, keys in enumerate(KEYS):
        for app in (a, b):
            _trace(app, keys)
            for k in range(1, n):
                _filter(app, k, n)
        _filter(a, n, n)
        _filter(b, n, n, 0, cut)
        with pytest.raises(hip_lib.RtptError) as e:
            b.backend.ctx.present(img[1].data_ptr(), 0, h)
        assert e.value.code == hip_lib.RTPT_E_INVALID
        b.backend.ctx.present(img[1].data_ptr(), 0, cut)
        _filter(b, n, n, cut, h)
        _same(_colour(hip_lib, a.backend.ctx), _colour(hip_lib, b.backend.ctx), (exact, chain, f))
        a.backend.ctx.present(img[0].data_ptr(), 0, h)
        b.backend.ctx.present(img[1].data_ptr(), 0, h)
        a.backend.ctx.sync()
        b.backend.ctx.sync()
        got = img.cpu().numpy()
        assert got[0].any() and got[0].tobytes() == got[1].tobytes(), (exact, chain, f)
        _finish(a)
        _finish(b)
    _same(_colour(hip_lib, a.backend.ctx), _colour(hip_lib, b.backend.ctx), (exact, chain, "end"))
    # whole-frame calls: chained pairs + the final pass when chaining is forced at this size, one kernel per iteration otherwise
    la, lb = _launches(a.backend.ctx), _launches(b.backend.ctx)
    print("two ranges", exact, chain, la, lb)
    assert la == ((0, 3, 6, 0, 3) if chain else (12, 3, 0, 0, 3))
    # the second range is one more k_atrous_final per frame and nothing else
    assert lb == la[:1] + (6,) + la[2:]
    a.backend.close()
    b.backend.close()


# ------------------------------------------------------------------------------------------ b
# per frame (k_atrous, k_atrous_final, k_atrous_chain, k_atrous_chain_final), by (N, RTPT_CHAIN_MAX, RTPT_CHAIN_FINAL);
# k_gbuffer_pathtrace is 1 in every frame.  Taken from a run against the library of the commit before plan_filter existed.
CHAIN_PLANS = {
    # N = 1: the only iteration is odd and last, the FINAL pass
    (1, 1, 0): (0, 1, 0, 0), (1, 1, 1): (0, 1, 0, 0), (1, 2, 0): (0, 1, 0, 0), (1, 2, 1): (0, 1, 0, 0), (1, 3, 0): (0, 1, 0, 0), (1, 3, 1): (0, 1, 0, 0),
    # RTPT_CHAIN_MAX = 1 records nothing: one kernel per iteration, the last one FINAL when N is odd
    (2, 1, 0): (2, 0, 0, 0), (2, 1, 1): (2, 0, 0, 0), (3, 1, 0): (2, 1, 0, 0), (3, 1, 1): (2, 1, 0, 0),
    (4, 1, 0): (4, 0, 0, 0), (4, 1, 1): (4, 0, 0, 0), (5, 1, 0): (4, 1, 0, 0), (5, 1, 1): (4, 1, 0, 0),
    # pairs, greedy from the front: (1,2) (3,4); a pair starts at an odd iteration, so it never ends in the FINAL pass
    (2, 2, 0): (0, 0, 1, 0), (2, 2, 1): (0, 0, 1, 0), (3, 2, 0): (0, 1, 1, 0), (3, 2, 1): (0, 1, 1, 0),
    (4, 2, 0): (0, 0, 2, 0), (4, 2, 1): (0, 0, 2, 0), (5, 2, 0): (0, 1, 2, 0), (5, 2, 1): (0, 1, 2, 0),
    # RTPT_CHAIN_MAX = 3, N = 2: the run ends after the pair
    (2, 3, 0): (0, 0, 1, 0), (2, 3, 1): (0, 0, 1, 0),
    # N = 3: a chain stops in front of the FINAL pass unless RTPT_CHAIN_FINAL admits it: (1,2) 3 / (1,2,3)
    (3, 3, 0): (0, 1, 1, 0), (3, 3, 1): (0, 0, 0, 1),
    # N = 4: (1,2,3) 4 — the last iteration is even, not FINAL, and alone
    (4, 3, 0): (1, 0, 1, 0), (4, 3, 1): (1, 0, 1, 0),
    # N = 5: (1,2,3) 4 5 / (1,2,3) (4,5)
    (5, 3, 0): (1, 1, 1, 0), (5, 3, 1): (0, 0, 1, 1),
}


@pytest.mark.parametrize("chain_final", [0, 1])
@pytest.mark.parametrize("chain_max", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_chain_plans(hip_lib, monkeypatch, n, chain_max, chain_final):
    """every grouping of N iterations into launches that RTPT_CHAIN_MAX and RTPT_CHAIN_FINAL admit leaves IMAGE and PREVIOUS as
    one kernel per iteration does, an even N leaves IMAGE with alpha 0, and the launches are the planned ones"""
    monkeypatch.setenv("RTPT_CHAIN_MIN_PIXELS", "0")
    monkeypatch.setenv("RTPT_CHAIN_MAX", str(chain_max))
    monkeypatch.setenv("RTPT_CHAIN_FINAL", str(chain_final))
    a, b = _app(hip_lib, SMALL, n), _app(hip_lib, SMALL, n, hip_lib.FLAG_NO_FILTER_FUSION)
    tables = []
    for f, keys in enumerate(KEYS):
        out = []
        for app in (a, b):
            _trace(app, keys)
            app.applyTemporalFiltering()
            image = app.backend.ctx.readback(hip_lib.PLANE_IMAGE)
            assert image[..., :3].any() and (n & 1 or not image[..., 3].any()), (n, f)
            _finish(app)
            out.append([image, app.backend.ctx.readback(hip_lib.PLANE_PREVIOUS)])
        _same(out[0], out[1], (n, chain_max, chain_final, f))
        tables.append(_launches(a.backend.ctx))
        # one kernel per iteration, K0 / K1 / K2 each a launch of its own
        assert _launches(b.backend.ctx) == (n - (n & 1), n & 1, 0, 0, 0)
    print("chain plan", (n, chain_max, chain_final), tables)
    assert tables == [CHAIN_PLANS[(n, chain_max, chain_final)] + (1,)] * 3
    a.backend.close()
    b.backend.close()


# ------------------------------------------------------------------------------------------ c
# per frame, as above
INTERRUPTED = {
    "stream_wait": (1, 1, 3, 0),   # (1,2) 3 go out chained at the wait, then (1,2) (3,4) 5
    "restart": (3, 1, 2, 0),       # 1 2 3 go out one by one when the restart arrives, then (1,2) (3,4) 5
}


@pytest.mark.parametrize("how", ["stream_wait", "restart"])
def test_an_interrupted_run_of_records(hip_lib, monkeypatch, how):
    """iterations 1-3 are recorded, then rtpt_stream_wait(c, c) launches them (chained: it looks at no plane), or a restart at
    iteration 1 ends the run (one kernel per iteration: the record is not continued); iterations 1-5 follow.  Same planes
    as a context that launches every call when it is made"""
    monkeypatch.setenv("RTPT_CHAIN_MIN_PIXELS", "0")
    n = 5
    a, b = _app(hip_lib, SMALL, n), _app(hip_lib, SMALL, n, hip_lib.FLAG_NO_FILTER_FUSION)
    tables = []
    for f, keys in enumerate(KEYS):
        out = []
        for app in (a, b):
            ctx = app.backend.ctx
            _trace(app, keys)
            for k in (1, 2, 3):
                _filter(app, k, n)
            if how == "stream_wait":
                ctx.stream_wait(ctx)
            for k in range(1, n + 1):
                _filter(app, k, n)
            out.append(_colour(hip_lib, ctx))
            _finish(app)
            out[-1].append(ctx.readback(hip_lib.PLANE_PREVIOUS))
        _same(out[0], out[1], (how, f))
        tables.append(_launches(a.backend.ctx))
        assert _launches(b.backend.ctx) == (7, 1, 0, 0, 0)   # 1 2 3 | 1 2 3 4 5: only the last call is a final pass
    print("interrupted", how, tables)
    assert tables == [INTERRUPTED[how] + (1,)] * 3
    a.backend.close()
    b.backend.close()


# ------------------------------------------------------------------------------------------ d
def _every_plane(hip_lib, ctx):
    out = []
    for p in range(hip_lib.PLANE_COUNT):
        try:
            out.append(ctx.readback(p))
        except hip_lib.RtptError:   # not allocated in this configuration
            out.append(np.zeros(0, np.float32))
    return out


@pytest.mark.parametrize("before", [2, 3])   # (after two frames every rotating pair is back where it started; after three none is)
@pytest.mark.parametrize("variant", ["plain", "variance_svgf", "demodulate", "normals_plane"])
def test_resize_equals_a_fresh_context(hip_lib, cornell, variant, before):
    """a context that rendered at 64 x 48 and was resized renders what a context created at the new size renders: every
    plane of every frame, and every launch but k_lut (the tables belong to the scene, which a resize keeps)"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.scenes import tessellate_quads
    flags = {"variance_svgf": 0x900, "demodulate": 0x8000}.get(variant, 0)
    kw = dict(mesh=tessellate_quads(cornell[0], cornell[1], 2)) if variant == "normals_plane" else {}
    old = _app(hip_lib, (64, 48), 5, flags, **kw)
    for _ in range(before):
        old.drawScene()
    resized = old.backend.ctx
    resized.resize(*SMALL)
    resized.timing_collect()
    a, b = _app(hip_lib, SMALL, 5, flags, **kw), _app(hip_lib, SMALL, 5, flags, **kw)
    spare, a.backend.ctx = a.backend.ctx, resized    # the host state of a new application drives the resized context
    names = [k for k in hip_lib.KERNEL_NAMES if k != "k_lut"]
    for f, keys in enumerate(KEYS):
        a.drawScene(keys)
        b.drawScene(keys)
        _same(_every_plane(hip_lib, resized), _every_plane(hip_lib, b.backend.ctx), (variant, f))
        la, lb = _launches(resized, names), _launches(b.backend.ctx, names)
        print("resize", variant, before, f, dict(zip(names, la)))
        assert la == lb and sum(la) > 0, (variant, f)
    spare.close()
    resized.close()
    b.backend.close()


# ------------------------------------------------------------------------------------------ e
@pytest.mark.parametrize("how", ["set_plane", "bind_plane"])
def test_an_injected_colour_plane(hip_lib, monkeypatch, how):
    """IMAGE written by the caller (rtpt_set_plane) or replaced by a caller's buffer (rtpt_bind_plane) behind the trace: it
    reads back with the alpha the caller wrote, the first filter iteration gives it its depth channel, and the recorded
    iterations give the frames of one kernel per iteration"""
    import torch
    monkeypatch.setenv("RTPT_CHAIN_MIN_PIXELS", "0")
    n = 5
    a, b = _app(hip_lib, SMALL, n), _app(hip_lib, SMALL, n, hip_lib.FLAG_NO_FILTER_FUSION)
    keep = []
    for f, keys in enumerate(KEYS):
        out = []
        for app in (a, b):
            ctx = app.backend.ctx
            _trace(app, keys)
            plane = ctx.readback(hip_lib.PLANE_IMAGE)
            plane[..., :3] = plane[..., :3] * 0.5 + 0.125
            plane[..., 3] = 0.25 + np.arange(plane.shape[1], dtype=np.float32)[None, :]
            if how == "set_plane":
                ctx.set_plane(hip_lib.PLANE_IMAGE, plane)
            else:   # a buffer of its own per frame: the roles rotate, the one bound last frame is PREVIOUS now
                keep.append(torch.from_numpy(plane).cuda())
                torch.cuda.synchronize()
                ctx.bind_plane(hip_lib.PLANE_IMAGE, keep[-1].data_ptr(), plane.nbytes)
            assert np.array_equal(bits(ctx.readback(hip_lib.PLANE_IMAGE)), bits(plane)), (how, f)
            app.applyTemporalFiltering()
            out.append(_colour(hip_lib, ctx))
            _finish(app)
            out[-1].append(ctx.readback(hip_lib.PLANE_PREVIOUS))
        _same(out[0], out[1], (how, f))
        # two chained pairs and the final pass, as without the injection: the depth stamp is no timed launch
        assert _launches(a.backend.ctx) == (0, 1, 2, 0, 1) and _launches(b.backend.ctx) == (4, 1, 0, 0, 0)
    a.backend.close()
    b.backend.close()
