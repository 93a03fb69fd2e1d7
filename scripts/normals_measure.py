#!/usr/bin/env python3
"""What smooth shading costs (rtpt_scene_set_normals): a 4K frame of a 10 x 10 x 10 lattice of scenes.uv_sphere(24, 36) — 1,000
instances of 1,656 triangles, every sphere with a diffuse, a mirror and a glass band (materials are the base triangle's) — at 8
segments, with the vertex normals off against on: the same build, the same context flags, the same materials.

    python scripts/normals_measure.py [--width 3840 --height 2160 --segments 8 --frames 60 --warmup 10 --repeats 3]
                                      [--lattice 10 10 10 --lat 24 --lon 36]

Time: the two variants run in turn, `repeats` times over (alternating windows); every window is `frames` whole frames between two
device synchronisations on the host clock, after `warmup` frames of the same variant.  The light moves every frame so that frame
reuse serves nothing.  The tracing launches' time comes from the library's own HIP-event timing in ONE separate window of 10 frames
per variant, the closest-hit queries per pixel from the ray counter of that window (absorbed paths change the count).  Both
variants trace through the BVH: 1,656,000 triangles.
Re-pose: frames in which rtpt_scene_set_instances moves every instance (the lattice shifted by a millimetre and back), normals off
against on: what a move adds to a resting frame with normals, minus what it adds without, is the cofactor table's kernel — one
thread per instance — behind the re-pose.  Prints one JSON line.

--guide adds RTPT_FLAG_EXT_SMOOTH_GUIDE (interpolated normals in the filter's edge stop) as a third variant beside "smooth", the same
way: frame time in alternating windows, the tracing launch (K0 writes the guide normals inside it) and the filter launches from the
library's event timing, moved frames.  And what it buys, at --benefit-size (default 1920 x 1080) on the same lattice at rest: the RMSE
of the FIRST filtered frame (no history yet) against the mean of --benefit-frames unfiltered frames, off against on, over the whole
frame and over the pixels within one pixel of a facet edge (a 3 x 3 neighbourhood of the id plane that holds another id)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--lattice", type=int, nargs=3, default=(10, 10, 10))
    ap.add_argument("--lat", type=int, default=24)
    ap.add_argument("--lon", type=int, default=36)
    ap.add_argument("--guide", action="store_true")
    ap.add_argument("--benefit-size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--benefit-frames", type=int, default=32)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: one ROCm runtime for both)
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi, scenes
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    xyz, idx, nrm = scenes.uv_sphere(a.lat, a.lon, 1.0, (0.0, 1.0, 0.0))
    nx, ny, nz = a.lattice
    pitch = 2.5
    xf = scenes.lattice_xforms(nx, ny, nz, pitch)
    height, width = (ny - 1) * pitch + 2.0, (nx - 1) * pitch + 2.0
    dist = max(height, width * 9.0 / 16.0) / 2.0 / 0.2027 * 1.15
    cam = (-0.001, height / 2.0, 1.0 + dist)
    # materials per BASE triangle: instances share them, so the kinds alternate by latitude band — every sphere shows glass, mirror
    # and diffuse bands
    band = (np.arange(len(idx)) * 3 // len(idx)).astype(np.uint32)
    mats = np.zeros((3, 6), np.float32)
    mats[:, :3] = [(0.7, 0.7, 0.7), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)]
    mext = abi.materials_ext(mats, {1: ((0.9, 0.9, 0.9), 0.0)}, {2: ((0.95, 0.97, 1.0), 1.5)})

    def app_of(smooth, guide=False, size=None):
        w, h = size or (a.width, a.height)
        app = make_app(w, h, max_segments=a.segments, iterations=5, mesh=(xyz, idx), instance_xforms=xf, smooth_guide=guide,
                       cameraOrigin=cam, z_far=float(dist + nz * pitch + 10.0), lightPos=(1.0, float(cam[1]), float(cam[2]) - 8.0))
        ctx = app.backend.ctx
        ctx.set_materials_ext(band, mext)
        if smooth:
            ctx.set_normals(nrm)
        return app
    apps = {"flat": app_of(False), "smooth": app_of(True)}
    if a.guide:
        apps["guide"] = app_of(True, True)

    def run(app, frames, move=False):
        for f in range(frames):
            if move:
                shifted = xf.reshape(-1, 3, 4).copy()
                shifted[:, 0, 3] += np.float32(1e-3 * (f & 1))
                app.backend.ctx.scene_set_instances(shifted)
            app.drawScene(("J",) if f & 1 else ("L",))     # the light moves: nothing is reused
        app.backend.sync()
    ms = {name: [] for name in apps}
    for r in range(a.repeats):
        for name in (tuple(apps) if r % 2 == 0 else tuple(apps)[::-1]):     # both orders
            run(apps[name], a.warmup)
            t0 = time.perf_counter()
            run(apps[name], a.frames)
            ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
    kernels, rays, moved_ms = {}, {}, {}
    for name, app in apps.items():
        ctx = app.backend.ctx
        ctx.timing_enable(1)
        ctx.reset_counters()
        run(app, 10)
        tm = ctx.timing_collect()
        ctx.timing_enable(0)
        kernels[name] = {k: round(v[0] / v[1] * 1e3, 1) for k, v in tm.items() if v[1] and ("pathtrace" in k or (a.guide and "atrous" in k))}
        rays[name] = round(ctx.raycount() / (10 * a.width * a.height), 4)
        t = []
        for _ in range(a.repeats):
            run(app, 4, move=True)
            t0 = time.perf_counter()
            run(app, 20, move=True)
            t.append((time.perf_counter() - t0) * 1e3 / 20)
        moved_ms[name] = [round(x, 4) for x in t]
    for app in apps.values():
        app.backend.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    mm = {k: float(np.median(v)) for k, v in moved_ms.items()}
    out = {"size": [a.width, a.height], "segments": a.segments, "frames": a.frames, "repeats": a.repeats, "triangles": int(len(idx) * len(xf)),
           "base_triangles": int(len(idx)), "instances": int(len(xf)),
           "frame_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "frame_ms_median": {k: round(v, 4) for k, v in med.items()},
           "frame_ms_ratio_smooth_flat": round(med["smooth"] / med["flat"], 4), "trace_kernel_us": kernels, "queries_per_pixel": rays,
           "moved_frame_ms": moved_ms, "moved_frame_ms_median": {k: round(v, 4) for k, v in mm.items()},
           # what a move costs with normals beyond what it costs without: (moved - resting) smooth minus (moved - resting) flat
           "cofactor_table_ms_per_move": round((mm["smooth"] - med["smooth"]) - (mm["flat"] - med["flat"]), 4)}
    if a.guide:
        out["frame_ms_ratio_guide_smooth"] = round(med["guide"] / med["smooth"], 4)
        out["benefit"] = benefit(abi, app_of, tuple(a.benefit_size), a.benefit_frames)
    print(json.dumps(out))


def benefit(abi, app_of, size, n):
    """RMSE of the first filtered frame against the mean of n unfiltered frames at rest, guide off / on, whole frame and facet edges"""
    res = {}
    for name, guide in (("off", False), ("on", True)):
        app = app_of(True, guide, size)
        ctx = app.backend.ctx
        mean, first, ids = None, None, None
        for f in range(n):
            app.updateScene(())
            app.drawVisbilityBuffer()
            app.computeTemporalGradient()
            app.drawSceneToImage()
            traced = ctx.readback(abi.PLANE_IMAGE)[..., :3].astype(np.float64)
            mean = traced if mean is None else mean + traced
            if f == 0:
                ids = ctx.readback(abi.PLANE_VIS_ID)
            app.applyTemporalFiltering()
            if f == 0:
                first = ctx.readback(abi.PLANE_IMAGE)[..., :3].astype(np.float64)
            app.copyImageToSwapChainsCurrentImage()
            app.frameCount += 1
        app.backend.close()
        mean /= n
        edge = np.zeros(ids.shape, bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                edge |= np.roll(np.roll(ids, dy, 0), dx, 1) != ids
        edge &= ids > 0
        err = ((first - mean) ** 2).sum(-1)
        res[name] = {"rmse": float(np.sqrt(err.mean())), "rmse_facet_edges": float(np.sqrt(err[edge].mean())), "edge_pixels": int(edge.sum())}
    res["frames_in_the_mean"] = n
    res["size"] = list(size)
    res["rmse_ratio_on_off"] = round(res["on"]["rmse"] / res["off"]["rmse"], 4)
    res["rmse_facet_edges_ratio_on_off"] = round(res["on"]["rmse_facet_edges"] / res["off"]["rmse_facet_edges"], 4)
    return res


if __name__ == "__main__":
    main()
