#!/usr/bin/env python3
"""What sampling the analytic sphere light costs and buys (RTPT_FLAG_EXT_NEE_SPHERE): the 4K Cornell box of bench.py — no material
table, the reference's one light — four segments, with the flag off against on, the same build.  Written after
scripts/nee_measure.py.

    python scripts/nee_sphere_measure.py [--width 3840 --height 2160 --segments 4 --frames 200 --warmup 30 --repeats 3]
                                         [--reference-frames 4096] [--noise-frames 8]

Time: the two variants run in turn, `repeats` times over (alternating, both orders, so that a drift of the machine shows as spread
and not as a difference); every window is `frames` whole frames (K0 + K1 + K2 + 5 filter iterations) between two device
synchronisations on the host clock, after `warmup` frames of the same variant.  The light moves every frame so that frame reuse
serves nothing.  The flag gives up the queue kernels and the deferred final pass, so the frame time holds that too.  The tracing
launch's time comes from the library's own HIP-event timing in ONE separate window of 20 frames per variant, off then on (a figure
beside the frame time, not a second comparison), the closest-hit queries per pixel from the ray counter of that window: the
sample sends none, so they must not rise beyond what the changed paths explain.
Noise: the RMSE of the unfiltered one-sample IMAGE (K0 + K1 + K2, no filter) of `noise-frames` resting frames of either variant
against the mean of `reference-frames` flag-off samples per pixel (64 samples per pixel a frame), and the RMSE of the host's
finished frame (five a-trous passes, temporal accumulation) against the same mean: of the first frame of a fresh host, which has
no history, and of frame `noise-frames`.  Both variants estimate that mean.  Prints one JSON line."""
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
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reference-frames", type=int, default=4096, help="flag-off samples per pixel behind the reference mean (a multiple of 64)")
    ap.add_argument("--noise-frames", type=int, default=8)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: one ROCm runtime for both)
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app

    def app_of(on, spp=1):
        return make_app(a.width, a.height, max_segments=a.segments, iterations=5, nee_sphere=on, samples_per_pixel=spp)
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
    rmse, filtered_first, filtered_last = {}, {}, {}
    for name, on in (("off", False), ("on", True)):
        app = app_of(on)
        for _ in range(n_ref):        # frame numbers behind the reference's: samples it has not seen
            app.frameCount += 1
        rmse[name] = round(float(np.sqrt(np.mean([np.mean((img - mean) ** 2) for img in traced(app, a.noise_frames)]))), 6)
        app.backend.close()
        app = app_of(on)              # a fresh host: its first finished frame has no history
        for _ in range(n_ref):
            app.frameCount += 1
        for f in range(a.noise_frames):
            app.drawScene(())
            if f in (0, a.noise_frames - 1):
                final = app.backend.final_image_rows(0, a.height)[..., :3].astype(np.float64)
                (filtered_first if f == 0 else filtered_last)[name] = round(float(np.sqrt(np.mean((final - mean) ** 2))), 6)
        app.backend.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"size": [a.width, a.height], "segments": a.segments, "frames": a.frames, "repeats": a.repeats,
           "frame_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "frame_ms_median": {k: round(v, 4) for k, v in med.items()},
           "frame_ms_ratio_on_off": round(med["on"] / med["off"], 4), "trace_kernel_us": kernels, "queries_per_pixel": rays,
           "ray_ratio_on_off": round(rays["on"] / rays["off"], 4), "reference_samples": n_ref * 64, "noise_frames": a.noise_frames,
           "rmse_1spp_unfiltered": rmse, "rmse_ratio_on_off": round(rmse["on"] / rmse["off"], 4),
           "rmse_filtered_first_frame": filtered_first, "rmse_filtered_first_ratio_on_off": round(filtered_first["on"] / filtered_first["off"], 4),
           "rmse_filtered_last_frame": filtered_last, "rmse_filtered_last_ratio_on_off": round(filtered_last["on"] / filtered_last["off"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
