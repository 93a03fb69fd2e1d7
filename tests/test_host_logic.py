"""The headless host mirror (app.PathTracingApplication) against the reference's per-frame rules
(main.cpp:1090-1185, :1255-1306, :1463-1475), with a recording backend — no GPU involved."""
import ctypes as C

import numpy as np

from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi
from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import PathTracingApplication
from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan


class Recorder:
    def __init__(self):
        self.calls = []

    def scene_upload(self, *a):
        self.calls.append(("scene_upload",))

    def gbuffer(self, ubo, y0, y1):
        self.calls.append(("gbuffer", bytes(ubo), y0, y1))

    def temporal_gradient(self, pc, y0, y1):
        self.calls.append(("gradient", bytes(pc), y0, y1))

    def raytrace(self, pc, y0, y1):
        self.calls.append(("raytrace", bytes(pc), y0, y1))

    def temporal_filter(self, pc, ubo, y0, y1):
        self.calls.append(("filter", pc.waveletIteration, pc.maxWaveletIteration, y0, y1))

    def end_frame(self):
        self.calls.append(("end_frame",))

    def use_external_history(self, on, rows=None):
        self.calls.append(("ext_history", bool(on)))


def pc_of(raw):
    return abi.PushConstants.from_buffer_copy(raw)


def test_draw_scene_call_order_and_filter_loop():
    be = Recorder()
    app = PathTracingApplication(be, 100, 80, maxWaveletIteration=9)
    app.drawScene()
    names = [c[0] for c in be.calls]
    assert names == ["gbuffer", "gradient", "raytrace"] + ["filter"] * 9 + ["end_frame"]  # main.cpp:1105-1110
    assert [(c[1], c[2]) for c in be.calls if c[0] == "filter"] == [(k, 9) for k in range(1, 10)]  # :1258-1260
    assert all(c[-2:] == (0, 80) for c in be.calls if c[0] in ("gbuffer", "gradient", "raytrace", "filter"))
    assert app.frameCount == 1


def test_push_constant_update_rules():
    be = Recorder()
    app = PathTracingApplication(be, 64, 48, maxWaveletIteration=1)
    app.drawScene()                 # frame 0
    app.drawScene(("L",))           # light.x += 0.1
    app.drawScene(("W", "O"))       # camera.z -= 0.1, light.y += 0.1
    app.drawScene()
    pcs = [pc_of(c[1]) for c in be.calls if c[0] == "raytrace"]
    assert [p.frameNumber for p in pcs] == [0, 1, 2, 3]                      # :1171
    assert [p.sample_batch for p in pcs] == [0, 0, 0, 0]                     # :1237
    # frame 0: lightPosPrev is what initializeSceneConstants left in lightPos (main.cpp:661-666, :1177)
    assert list(pcs[0].lightPosPrev) == [1.0, 1.0, np.float32(-0.4)]
    assert list(pcs[0].lightPos) == [1.0, 1.0, np.float32(-0.4)]
    assert list(pcs[1].lightPos)[0] == np.float32(np.float32(1.0) + np.float32(0.1))
    assert list(pcs[1].lightPosPrev) == list(pcs[0].lightPos)               # :1177
    assert list(pcs[2].lightPosPrev) == list(pcs[1].lightPos)
    assert list(pcs[3].lightPosPrev) == list(pcs[3].lightPos)                # static again
    assert list(pcs[0].previousCameraColor) == [0.5, 0.5, 0.5]               # :1173 after :662
    # cameraPos is pushed on frame 0 and when the camera moved (:1181-1184)
    assert list(pcs[0].cameraPos) == [np.float32(-0.001), 1.0, 6.0]
    assert list(pcs[1].cameraPos) == list(pcs[0].cameraPos)
    assert list(pcs[2].cameraPos)[2] == np.float32(np.float32(6.0) - np.float32(0.1))


def test_light_wraparound_keys():
    be = Recorder()
    app = PathTracingApplication(be, 32, 32, maxWaveletIteration=1, lightPos=(1.95, 1.0, 0.0))
    app.updateScene(("L",))   # 2.05 > 2 -> -20 (main.cpp:1151-1153)
    assert app.lightPos[0] == -20
    app.updateScene(("J",))   # -20.1 < -20 -> 2 (main.cpp:1157-1160)
    assert app.lightPos[0] == 2


def test_ubo_prev_matrices_and_initial_view():
    be = Recorder()
    app = PathTracingApplication(be, 100, 80, maxWaveletIteration=1)
    first = bytes(app.ubo)
    u0 = abi.Ubo.from_buffer_copy(first)
    # uploadBuffers (main.cpp:481-489): the initial view looks at (0,1,0), prev = current
    assert list(u0.view) == list(abi.look_at((-0.001, 1.0, 6.0), (0, 1, 0), (0, 1, 0)))
    assert list(u0.viewPrev) == list(u0.view) and list(u0.projPrev) == list(u0.proj)
    assert u0.proj[5] < 0                                           # proj[1][1] *= -1 (main.cpp:484)
    app.drawScene()
    u1 = abi.Ubo.from_buffer_copy(be.calls[0][1])
    assert list(u1.viewPrev) == list(u0.view)                       # main.cpp:1465-1467
    assert list(u1.view) == list(abi.look_at((-0.001, 1.0, 6.0), (-0.001, 1.0, 0.0), (0, 1, 0)))  # :1470
    app.drawScene(("D",))
    u2 = abi.Ubo.from_buffer_copy([c for c in be.calls if c[0] == "gbuffer"][1][1])
    assert list(u2.viewPrev) == list(u1.view)
    assert u2.view[12] != u1.view[12]                               # camera x moved
    assert list(u2.model) == list(np.eye(4, dtype=np.float32).ravel())


def test_strip_rank_row_ranges_reach_the_backend():
    be = Recorder()
    plan = StripPlan(2160, 8, 3, 5, "redundant")
    app = PathTracingApplication(be, 3840, 2160, maxWaveletIteration=5, plan=plan)
    app.drawScene()
    o0, o1 = plan.own
    assert (o0, o1) == (810, 1080)
    assert ("ext_history", False) in be.calls     # frame 0 / resting camera: strip-local history
    calls = {c[0]: c for c in be.calls if c[0] != "filter"}
    assert calls["gbuffer"][-2:] == (o0 - 15, o1 + 15)
    assert calls["gradient"][-2:] == (o0, o1)
    assert calls["raytrace"][-2:] == (o0 - 15, o1 + 15)
    filt = [c for c in be.calls if c[0] == "filter"]
    assert [c[-2:] for c in filt] == [(o0 - 14, o1 + 14), (o0 - 12, o1 + 12), (o0 - 9, o1 + 9), (o0 - 5, o1 + 5), (o0, o1)]


# ------------------------------------------------------------------------------ output path
def test_output_unorm8_png_pfm_roundtrip(tmp_path):
    import struct
    import zlib
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import output
    img = np.zeros((5, 7, 4), np.float32)
    img[..., 0] = np.linspace(-0.5, 1.5, 7)[None, :]       # clamps on both sides
    img[..., 1] = 0.5
    img[2, 3, 2] = np.nan                                   # D7: NaNs may reach the image; the blit shows 0
    u8 = output.to_unorm8(img)
    assert u8.shape == (5, 7, 3) and u8.dtype == np.uint8
    assert u8[0, 0, 0] == 0 and u8[0, -1, 0] == 255 and u8[0, 0, 1] == 128 and u8[2, 3, 2] == 0
    assert (output.tonemap(img, gamma=1.0) == u8).all()
    p = tmp_path / "a.png"
    output.write_png(str(p), u8)
    raw = p.read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    w, h, depth, ctype = struct.unpack(">IIBB", raw[16:26])
    assert (w, h, depth, ctype) == (7, 5, 8, 2)
    n = struct.unpack(">I", raw[33:37])[0]
    assert raw[37:41] == b"IDAT"
    rows = np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(5, 1 + 21)
    assert (rows[:, 0] == 0).all() and (rows[:, 1:].reshape(5, 7, 3) == u8).all()
    q = tmp_path / "a.pfm"
    clean = np.nan_to_num(img)
    output.write_pfm(str(q), clean)
    assert np.array_equal(output.read_pfm(str(q)), clean[..., :3])


def test_posed_scene_bounds_and_static_test_follow_the_model_matrix():
    """app._world_bounds: the reprojection bound's depth range uses the POSED scene; app._camera_static also requires
    model == modelPrev (a moving model reprojects pixels across strips like a moving camera does)"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import DEFAULT_SCENE, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import reprojection_rows
    abi.load()
    app = PathTracingApplication(Recorder(), 64, 48, 3)
    app.loadMesh(DEFAULT_SCENE)
    app.buildAccelerationStructure()
    app.updateScene()
    app.frameCount += 1
    lo, hi = app._world_bounds()
    assert np.allclose(lo, app.sceneBounds[0]) and np.allclose(hi, app.sceneBounds[1])
    m = np.eye(4, dtype=np.float32)
    m[1, 3] = 0.5      # lift the scene by half a unit (column-major storage below)
    app.modelMatrix = np.ascontiguousarray(m.T).ravel()
    app.updateScene()
    assert not app._camera_static(), "view and proj rest, the model moved"
    lo2, hi2 = app._world_bounds()
    assert np.allclose(lo2, lo + [0, 0.5, 0]) and np.allclose(hi2, hi + [0, 0.5, 0])
    assert reprojection_rows(app.ubo, 64, 48, (10, 20), (lo2, hi2)) == (0, 48), "a changed model: the whole previous frame"
    app.frameCount += 1
    app.updateScene()   # same model again: static
    assert app._camera_static()
    a, b = reprojection_rows(app.ubo, 64, 48, (10, 20), app._world_bounds())
    assert a <= 10 and b >= 20 and (b - a) < 48


def test_bench_watchdog():
    """bench.py's guard on the secondary legs of a multi-rank run (a message that never arrives on an interconnect this code
    has not met): after the timeout rank 0 writes the headline line it holds, with a note, to the real stdout and the process
    exits 0 without running on; the other ranks leave silently a moment later"""
    import json
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import bench, time\n"
            "bench._STDOUT_FD.append(1)\n"
            "bench._arm_watchdog({'metric': 'm', 'value': 1.0}, %d, 0.05)\n"
            "time.sleep(20)\n"
            "print('not reached')\n")
    out = subprocess.run([sys.executable, "-c", code % 0], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "not reached" not in out.stdout
    line = json.loads(out.stdout.strip())
    assert line["metric"] == "m" and "did not finish" in line["also"]["_watchdog"]
    out = subprocess.run([sys.executable, "-c", code % 1], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout == ""


def test_bench_rewind_replays_the_first_frames():
    """bench.py's wake-up renders for a time, not a number of frames, and then rewinds the application: the frames after the
    rewind hand the backend the same push constants and UBOs as the first frames of a new application (the camera and light
    moved during the wake-up included)"""
    import bench
    script = [(), ("E",), ("J", "D"), ()]
    be = Recorder()
    app = PathTracingApplication(be, 64, 48, maxWaveletIteration=3)
    camera0, light0 = app.cameraOrigin.copy(), app.lightPos.copy()
    app.run(len(script), script)
    first = list(be.calls)
    app.run(6, [("W", "I")] * 6)
    bench._rewind(app, camera0, light0)
    be.calls.clear()
    app.run(len(script), script)
    assert be.calls == first and app.frameCount == len(script)


class _Finished:
    """the backend protocol's readback of the finished frame: pixel (x, y) of the frame holds (x, y, x * y, -1)"""
    def __init__(self, W, H):
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        self.frame = np.stack([x, y, x * y, -np.ones_like(x)], axis=-1)

    def readback_rows(self, plane, y0, y1):
        assert plane == abi.PLANE_PREVIOUS
        return self.frame[y0:y1]


def test_bench_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: rgb float32 of the finished frame, whole, or at a seeded ascending sample of distinct pixel indices when
    the frame exceeds DUMP_PIXELS — the same sample every run"""
    import types

    import bench
    W, H = 40, 30
    be = _Finished(W, H)
    app = types.SimpleNamespace(render_width=W, render_height=H, plan=StripPlan(H, 1, 0, 3), backend=be)
    bench.dump_outputs(app, str(tmp_path / "whole"), 1, None, None)
    got = np.load(tmp_path / "whole" / "frame.npy")
    assert got.dtype == np.float32 and got.tobytes() == be.frame[..., :3].tobytes()
    assert not (tmp_path / "whole" / "frame_pixel_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_PIXELS", 100)
    for d in ("a", "b"):
        bench.dump_outputs(app, str(tmp_path / d), 1, None, None)
    vals, idx = np.load(tmp_path / "a" / "frame.npy"), np.load(tmp_path / "a" / "frame_pixel_index.npy")
    assert vals.dtype == np.float32 and vals.shape == (100, 3) and idx.dtype == np.float64 and idx.shape == (100,)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < W * H and np.array_equal(idx, np.round(idx))
    i = idx.astype(np.int64)
    assert vals.tobytes() == be.frame.reshape(-1, 4)[i, :3].tobytes()
    assert np.load(tmp_path / "b" / "frame.npy").tobytes() == vals.tobytes()
    assert np.load(tmp_path / "b" / "frame_pixel_index.npy").tobytes() == idx.tobytes()
