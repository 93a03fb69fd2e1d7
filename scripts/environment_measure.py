#!/usr/bin/env python3
"""What an environment map costs (rtpt_set_environment): four scattered 16-byte loads per path that ends in the sky, and where a
large map falls out of the caches.  Two frames, each with the environment off against on at map sizes 64, 1024 and 4096 (1 MB,
16 MB and 256 MB of texels), bilinear:

  cornell   bench.py's flagship workload, the 4K Cornell box at 4 segments
  lattice   normals_measure.py's 10 x 10 x 10 lattice of UV spheres with diffuse, mirror and glass bands, 4K, 8 segments

    python scripts/environment_measure.py [--width 3840 --height 2160 --frames 60 --warmup 10 --repeats 3] [--sizes 64 1024 4096]
                                          [--only cornell|lattice]

Time: the variants of a frame run in turn, `repeats` times over, in both orders (alternating windows); every window is `frames`
whole frames between two device synchronisations on the host clock, after `warmup` frames of the same variant.  The light moves every
frame so that frame reuse serves nothing.  The tracing launch's time comes from the library's own HIP-event timing in ONE separate
window of 10 frames per variant.  "off" is a context that never had an environment: its launches are the parent's kernels; note that
"on" also gives up the deferred final pass's ride in the tracing launch and the queue kernels (include/rtpt.h), so on the Cornell
box the difference is that too, not the lookup alone.  The map is a smooth synthetic sky with a small bright sun (values do not
change the cost; the addresses are the paths').  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sky_map(n):
    """[n, n, 4] float32: a gradient with a sun, written straight into the octahedral square"""
    c = ((np.arange(n, dtype=np.float32) + 0.5) / n) * 2 - 1
    u, v = np.meshgrid(c, c)
    up = 1 - np.abs(u) - np.abs(v)
    tx = np.ones((n, n, 4), np.float32)
    tx[..., 0] = 0.4 + 0.3 * up
    tx[..., 1] = 0.5 + 0.3 * up
    tx[..., 2] = 0.7 + 0.3 * up
    tx[(u - 0.3) ** 2 + (v + 0.2) ** 2 < 0.002] = (2e3, 1.8e3, 1.5e3, 1.0)
    return np.clip(tx, 0.0, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=(64, 1024, 4096))
    ap.add_argument("--only", choices=("cornell", "lattice"))
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: one ROCm runtime for both)
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi, scenes
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app

    def cornell():
        return make_app(a.width, a.height, max_segments=4, iterations=5), 4

    def lattice():
        xyz, idx, _ = scenes.uv_sphere(24, 36, 1.0, (0.0, 1.0, 0.0))
        nx, ny, nz, pitch = 10, 10, 10, 2.5
        xf = scenes.lattice_xforms(nx, ny, nz, pitch)
        height, width = (ny - 1) * pitch + 2.0, (nx - 1) * pitch + 2.0
        dist = max(height, width * 9.0 / 16.0) / 2.0 / 0.2027 * 1.15
        cam = (-0.001, height / 2.0, 1.0 + dist)
        app = make_app(a.width, a.height, max_segments=8, iterations=5, mesh=(xyz, idx), instance_xforms=xf, cameraOrigin=cam,
                       z_far=float(dist + nz * pitch + 10.0), lightPos=(1.0, float(cam[1]), float(cam[2]) - 8.0))
        band = (np.arange(len(idx)) * 3 // len(idx)).astype(np.uint32)
        mats = np.zeros((3, 6), np.float32)
        mats[:, :3] = [(0.7, 0.7, 0.7), (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)]
        app.backend.ctx.set_materials_ext(band, abi.materials_ext(mats, {1: ((0.9, 0.9, 0.9), 0.0)}, {2: ((0.95, 0.97, 1.0), 1.5)}))
        return app, 8

    def run(app, frames):
        for f in range(frames):
            app.drawScene(("J",) if f & 1 else ("L",))     # the light moves: nothing is reused
        app.backend.sync()

    out = {"size": [a.width, a.height], "frames": a.frames, "repeats": a.repeats, "map_sizes": list(a.sizes)}
    for scene, make in (("cornell", cornell), ("lattice", lattice)):
        if a.only and a.only != scene:
            continue
        apps = {"off": make()[0]}
        for n in a.sizes:
            apps[f"on_{n}"] = make()[0]
            apps[f"on_{n}"].backend.set_environment(sky_map(n))
        ms = {name: [] for name in apps}
        for r in range(a.repeats):
            for name in (tuple(apps) if r % 2 == 0 else tuple(apps)[::-1]):     # both orders
                run(apps[name], a.warmup)
                t0 = time.perf_counter()
                run(apps[name], a.frames)
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.frames)
        kernels, rays = {}, {}
        for name, app in apps.items():
            ctx = app.backend.ctx
            ctx.timing_enable(1)
            ctx.reset_counters()
            run(app, 10)
            tm = ctx.timing_collect()
            ctx.timing_enable(0)
            kernels[name] = {k: round(v[0] / v[1] * 1e3, 1) for k, v in tm.items() if v[1] and ("pathtrace" in k or "atrous" in k)}
            rays[name] = round(ctx.raycount() / (10 * a.width * a.height), 4)
        for app in apps.values():
            app.backend.close()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out[scene] = {"frame_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "frame_ms_median": {k: round(v, 4) for k, v in med.items()},
                      "frame_ms_ratio_on_off": {k: round(v / med["off"], 4) for k, v in med.items() if k != "off"},
                      "launch_us": kernels, "queries_per_pixel": rays}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
