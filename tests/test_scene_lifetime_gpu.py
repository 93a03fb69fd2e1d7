"""Who owns device memory (csrc/api_internal.hpp: Buf, Scene): every buffer of a context is released by rtpt_destroy, a
scene that is replaced gives its memory back, a refused call changes nothing, a plane bound by the caller is neither
freed nor counted.

Measured with the library's own count of the bytes its contexts hold (rtpt_debug_live_device_bytes): hipMemGetInfo reports
the whole device, which other processes share.  The count is process-wide, so every test compares readings and starts by
collecting contexts that earlier tests left to the garbage collector.  Flags are fixed at rtpt_create, so "every route"
runs one context per flag set, each through every kind of replacement.  No test here provokes an allocation failure."""
import gc

import numpy as np
import pytest

import test_traversal_gpu as T
from conftest import bits

pytestmark = pytest.mark.gpu

W, H, SEG, N = 64, 48, 3, 3
D_LBVH, D_SAH, D_FLAT = 0x1000, 0x2000, 0x4000
ROUTES = (0, D_LBVH, D_LBVH | D_SAH, D_LBVH | D_SAH | D_FLAT)   # host tree, device LBVH, device SAH, device flatten


@pytest.fixture(scope="module")
def soup():
    return T._soup(np.random.default_rng(500), 500)


@pytest.fixture
def live(hip_lib):
    gc.collect()
    return hip_lib.live_device_bytes


def _make(hip_lib, mesh, flags=0, xf=None, **kw):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    return make_app(W, H, max_segments=SEG, iterations=N, flags=flags, mesh=mesh, instance_xforms=xf, **kw)


def _upload(app, mesh, xf=None):
    app.objVertices, app.objIndices = mesh
    app.buildAccelerationStructure(xf)


def _two_instances(shift=0.0):
    xf = np.tile(np.eye(4, dtype=np.float32)[:3].ravel(), (2, 1))
    xf[1, [3, 7, 11]] = (0.9 + shift, 0.1, -0.5)
    return xf


def _frame(hip_lib, app):
    """one frame, pass by pass, with every plane the other GPU tests read back"""
    ctx, out = app.backend.ctx, {}
    app.updateScene(())
    app.drawVisbilityBuffer()
    app.computeTemporalGradient()
    app.drawSceneToImage()
    for name in ("IMAGE", "HIT_ID", "VIS_ID", "WORLDPOS", "DEPTH", "GRADIENT", "LUT", "LUT_PREV"):
        out["traced " + name] = ctx.readback(getattr(hip_lib, "PLANE_" + name))
    app.applyTemporalFiltering()
    out["final IMAGE"] = ctx.readback(hip_lib.PLANE_IMAGE)
    out["PREV_PIXEL"] = ctx.readback(hip_lib.PLANE_PREV_PIXEL)
    app.copyImageToSwapChainsCurrentImage()
    app.frameCount += 1
    out["PREVIOUS"] = ctx.readback(hip_lib.PLANE_PREVIOUS)
    out["rays"] = np.array([ctx.raycount()], np.uint64)
    return out


def test_destroy_returns_everything(hip_lib, live, soup, monkeypatch):
    """one LDS stack entry per lane: the traversal's spill area exists after a frame, and rtpt_destroy frees it too (it
    was missing from the list of buffers rtpt_destroy used to free by name)"""
    monkeypatch.setenv("RTPT_BVH_STACK_LDS", "1")
    start = live()
    app = _make(hip_lib, soup)
    created = live()
    app.drawScene()
    app.backend.ctx.sync()
    assert created > start and live() > created, (start, created, live())
    app.backend.close()
    assert live() == start, f"rtpt_destroy left {live() - start} bytes behind"


def test_every_route_and_every_replacement_returns_everything(hip_lib, live, soup, cornell, monkeypatch):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import PathTracingApplication
    monkeypatch.setenv("RTPT_BVH_STACK_LDS", "1")
    start = live()
    for flags in ROUTES:
        app = _make(hip_lib, soup, flags)
        ctx = app.backend.ctx
        info = ctx.scene_build_info()
        assert ctx.debug_upload_info()["device_flatten"] == int(bool(flags & D_FLAT)), hex(flags)
        assert info["builder"] == (hip_lib.BUILDER_DEVICE_SAH if flags & D_SAH else hip_lib.BVH_BUILDER_DEVICE_LBVH if flags
                                   else hip_lib.BVH_BUILDER_HOST_SAH), (hex(flags), info)
        app.drawScene()
        _upload(app, cornell[:2])                      # 32 triangles: brute force
        app.drawScene()
        _upload(app, soup, _two_instances())
        app.drawScene()
        app.setInstanceTransforms(_two_instances(0.3))
        app.drawScene()
        ctx.scene_rebuild()
        app.drawScene()
        ctx.resize(32, 24)
        PathTracingApplication(app.backend, 32, 24, N).drawScene()
        ctx.resize(W, H)
        app.drawScene()
        ctx.sync()
        assert live() > start
        app.backend.close()
        assert live() == start, f"flags {flags:#x}: rtpt_destroy left {live() - start} bytes behind"


@pytest.mark.parametrize("flags", [0, D_LBVH | D_SAH])
def test_no_growth_on_re_upload(hip_lib, live, soup, flags):
    """the first upload is excluded: the device builder's scratch grows to its size there and is kept"""
    start = live()
    app = _make(hip_lib, soup, flags)
    after = []
    for i in range(4):
        if i:
            _upload(app, soup)
        app.drawScene()
        app.backend.ctx.sync()
        after.append(live())
    assert after[1] == after[2] == after[3], after
    app.backend.close()
    assert live() == start


def test_borrowed_planes_are_not_freed_or_counted(hip_lib, live, soup):
    import torch
    start = live()
    app = _make(hip_lib, soup)
    ctx = app.backend.ctx
    px = W * H
    # a plane the context holds no buffer for (the debug plane, not enabled): binding moves nothing
    ids = torch.full((H, W), 0x5EED, dtype=torch.int32, device="cuda")
    # a plane the context owns: binding releases the context's buffer, and the tensor that takes its place is not counted
    image = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    before = live()
    ctx.bind_plane(hip_lib.PLANE_HIT_ID, ids.data_ptr(), ids.numel() * 4)
    assert live() == before
    ctx.bind_plane(hip_lib.PLANE_IMAGE, image.data_ptr(), image.numel() * 4)
    assert live() == before - px * 16
    app.drawScene()   # the history hand-over leaves the finished frame in the bound tensor or in a plane of the context
    ctx.sync()
    app.backend.close()
    assert live() == start
    torch.cuda.synchronize()
    assert (ids.cpu().numpy() == 0x5EED).all()
    ids.fill_(7)
    image.fill_(1.5)
    torch.cuda.synchronize()
    assert (ids.cpu().numpy() == 7).all() and (image.cpu().numpy() == 1.5).all()


def test_refused_calls_keep_the_scene(hip_lib, live, soup, monkeypatch):
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import PathTracingApplication
    monkeypatch.setenv("RTPT_NO_FRAME_REUSE", "1")
    app = _make(hip_lib, soup, debug_mask=hip_lib.DEBUG_HIT_ID | hip_lib.DEBUG_PREV_PIXEL)
    ctx = app.backend.ctx
    first = _frame(hip_lib, app)
    assert first["traced VIS_ID"].any() and first["rays"][0] > 0, "the frame sees the scene"
    before = live()
    bad = soup[1].copy()
    bad[-1, 2] = len(soup[0])
    with pytest.raises(hip_lib.RtptError) as e:
        ctx.scene_upload(soup[0], bad)
    assert e.value.code == hip_lib.RTPT_E_INVALID and "index out of range" in str(e.value)
    with pytest.raises(hip_lib.RtptError) as e:
        ctx.scene_set_instances(_two_instances())   # the upload had no transforms: its count is 1
    assert e.value.code == hip_lib.RTPT_E_INVALID
    assert live() == before
    # the inputs of the first frame again: frame number 0, no history (rtpt_resize to the same size clears the frame
    # state and leaves the scene alone)
    ctx.resize(W, H)
    again = _frame(hip_lib, PathTracingApplication(app.backend, W, H, N))
    for name, a in first.items():
        assert np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(again[name]) if a.dtype == np.float32 else again[name]), name
    assert live() == before
    app.backend.close()
