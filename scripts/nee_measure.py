#!/usr/bin/env python3
"""What next-event estimation costs and buys (RTPT_FLAG_EXT_NEE): the 4K Cornell box lit by a small emissive quad under its
ceiling — an OBJ with an .mtl this script writes: Kd the reference's normal-keyed colour of every triangle, Ke on the quad —
with the flag off against on, the same build, the same material table.

    python scripts/nee_measure.py [--width 3840 --height 2160 --segments 4 --frames 200 --warmup 30 --repeats 3]
                                  [--lamp 0.1] [--reference-frames 4096] [--noise-frames 8]

Time: the two variants run in turn, `repeats` times over (alternating, so that a drift of the machine shows as spread and not as
a difference); every window is `frames` whole frames (K0 + K1 + K2 + 5 filter iterations) between two device synchronisations on
the host clock, after `warmup` frames of the same variant.  The light moves every frame so that frame reuse serves nothing.  The
tracing launch's time comes from the library's own HIP-event timing in ONE separate window of 20 frames per variant, off then on
(not interleaved: a figure beside the frame time, not a second comparison), the closest-hit queries per pixel from the ray counter
of that window.
Noise: the RMSE of the unfiltered one-sample IMAGE (K0 + K1 + K2, no filter) of `noise-frames` frames of either variant against
the mean of `reference-frames` flag-off samples per pixel — 64 samples per pixel a frame, so a sixty-fourth as many read-backs.
Both variants estimate that mean.  Prints one JSON line."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_scene(directory, xyz, idx, lamp_share):
    """lamp.obj + lamp.mtl: the mesh with one material per normal-keyed colour, and a square lamp of `lamp_share` of the room's
    width, facing down, 0.5 % of the room's height under the ceiling's middle.  Returns the OBJ's path"""
    v = xyz[idx].astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cls = np.where(n[:, 0] > 0.99, 1, np.where(-n[:, 0] > 0.99, 2, 0))
    lo, hi = xyz.min(0).astype(np.float64), xyz.max(0).astype(np.float64)
    c, h = (lo + hi) / 2, lamp_share * (hi[0] - lo[0]) / 2
    y = hi[1] - 0.005 * (hi[1] - lo[1])
    quad = [(c[0] - h, y, c[2] - h), (c[0] + h, y, c[2] - h), (c[0] + h, y, c[2] + h), (c[0] - h, y, c[2] + h)]
    with open(os.path.join(directory, "lamp.mtl"), "w") as f:
        f.write("newmtl grey\nKd 0.7 0.7 0.7\nnewmtl red\nKd 1 0 0\nnewmtl green\nKd 0 1 0\nnewmtl lamp\nKd 0 0 0\nKe 40 40 40\n")
    with open(os.path.join(directory, "lamp.obj"), "w") as f:
        f.write("mtllib lamp.mtl\n")
        for p in xyz:
            f.write("v %.9g %.9g %.9g\n" % tuple(p))
        for p in quad:
            f.write("v %.9g %.9g %.9g\n" % p)
        for k, name in enumerate(("grey", "red", "green")):
            f.write("usemtl %s\n" % name)
            for t in idx[cls == k]:
                f.write("f %d %d %d\n" % tuple(t + 1))
        b = len(xyz) + 1
        f.write("usemtl lamp\nf %d %d %d %d\n" % (b, b + 1, b + 2, b + 3))
    return os.path.join(directory, "lamp.obj")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lamp", type=float, default=0.1, help="the lamp's side as a share of the room's width")
    ap.add_argument("--reference-frames", type=int, default=4096, help="flag-off samples per pixel behind the reference mean (a multiple of 64)")
    ap.add_argument("--noise-frames", type=int, default=8)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: one ROCm runtime for both)
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import DEFAULT_SCENE, make_app
    xyz, idx = abi.load_obj(DEFAULT_SCENE)
    tmp = tempfile.mkdtemp(prefix="nee_measure_")
    scene = write_scene(tmp, xyz, idx, a.lamp)
    tri, mats = abi.load_obj_materials(scene)
    xyz, idx = abi.load_obj(scene)
    shutil.rmtree(tmp)       # read: mesh and table go to the contexts as arrays

    def app_of(nee, spp=1):
        app = make_app(a.width, a.height, max_segments=a.segments, iterations=5, mesh=(xyz, idx), nee=nee, samples_per_pixel=spp)
        app.backend.ctx.set_materials(tri, mats)
        assert len(app.backend.ctx.debug_light_list()) == (2 if nee else 0)
        return app
    apps = {"off": app_of(False), "on": app_of(True)}

    def run(app, frames):
        for f in range(frames):
            app.drawScene(("J",) if f & 1 else ("L",))     # the light moves: nothing is reused
        app.backend.sync()
    ms = {name: [] for name in apps}
    for r in range(a.repeats):
        for name in (("off", "on") if r % 2 == 0 else ("on", "off")):     # both orders
            run(apps[name], a.warmup)
            t0 = time.perf_counter()
            run(apps[name], a.frames)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    kernels, rays = {}, {}
    for name, app in apps.items():
        ctx = app.backend.ctx
        ctx.timing_enable(1)
        ctx.reset_counters()
        run(app, 20)
        tm = ctx.timing_collect()
        ctx.timing_enable(0)
        kernels[name] = {k: round(v[0] / v[1] * 1e3, 1) for k, v in tm.items() if v[1] and "pathtrace" in k}
        rays[name] = round(ctx.raycount() / (20 * a.width * a.height), 4)
        app.backend.close()

    def traced(app, frames):
        """the unfiltered IMAGE of `frames` frames of a resting scene, rgb float64 [H, W, 3] each"""
        for _ in range(frames):
            app.updateScene(())
            app.drawVisbilityBuffer()
            app.computeTemporalGradient()
            app.drawSceneToImage()
            yield app.backend.ctx.readback(abi.PLANE_IMAGE)[..., :3].astype(np.float64)
            app.frameCount += 1
    ref_app = app_of(False, spp=64)
    n_ref = max(1, a.reference_frames // 64)
    mean = np.zeros((a.height, a.width, 3))
    for img in traced(ref_app, n_ref):
        mean += img / n_ref
    ref_app.backend.close()
    rmse = {}
    for name, nee in (("off", False), ("on", True)):
        app = app_of(nee)
        for _ in range(n_ref):        # frame numbers behind the reference's: samples it has not seen
            app.frameCount += 1
        rmse[name] = round(float(np.sqrt(np.mean([np.mean((img - mean) ** 2) for img in traced(app, a.noise_frames)]))), 6)
        app.backend.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"size": [a.width, a.height], "segments": a.segments, "frames": a.frames, "repeats": a.repeats, "lamp_share": a.lamp,
           "frame_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "frame_ms_median": {k: round(v, 4) for k, v in med.items()},
           "frame_ms_ratio_on_off": round(med["on"] / med["off"], 4), "trace_kernel_us": kernels, "queries_per_pixel": rays,
           "ray_ratio_on_off": round(rays["on"] / rays["off"], 4), "reference_samples": n_ref * 64, "noise_frames": a.noise_frames,
           "rmse_1spp_unfiltered": rmse, "rmse_ratio_on_off": round(rmse["on"] / rmse["off"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
