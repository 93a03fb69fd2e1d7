#!/usr/bin/env python3
"""What a glass box costs (rtpt_scene_set_materials_ext, RTPT_MAT_DIELECTRIC): the 4K Cornell box with the short box's ten
triangles made glass (ior 1.5, colour 0.9), against the same table all diffuse (through rtpt_scene_set_materials: the kernels that
know neither the specular bounce nor the dielectric interface) and against the same box as a mirror (the kernels that know the
specular bounce only).  Kd is the reference's normal-keyed colour of every triangle.

    python scripts/dielectric_measure.py [--width 3840 --height 2160 --segments 4 --frames 200 --warmup 30 --repeats 3]

The three variants run in turn, `repeats` times over (alternating, so that a drift of the machine shows as spread and not
as a difference); every window is `frames` whole frames (K0 + K1 + K2 + 5 filter iterations) between two device
synchronisations on the host clock, after `warmup` frames of the same variant.  The light moves every frame so that frame
reuse serves nothing.  The tracing launch's time comes from the library's own HIP-event timing in a separate short window,
the closest-hit queries per pixel from the ray counter of that window.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def short_box(xyz, idx):
    """triangles of the connected component that is a ten-triangle box and the shorter of the two"""
    key = {}
    vid = np.array([key.setdefault(tuple(np.round(p, 5)), len(key)) for p in xyz])[idx]
    parent = list(range(len(key)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for t in vid:
        parent[find(t[0])] = find(t[1])
        parent[find(t[1])] = find(t[2])
    comp = np.array([find(t[0]) for t in vid])
    room = xyz[:, 1].max()
    boxes = [c for c in np.unique(comp) if (comp == c).sum() == 10 and xyz[idx[comp == c]][..., 1].max() < 0.9 * room]
    return comp == min(boxes, key=lambda c: xyz[idx[comp == c]][..., 1].max())


def normal_key_albedo(xyz, idx):
    v = xyz[idx].astype(np.float64)
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    alb = np.full((len(idx), 3), 0.7, np.float32)
    alb[n[:, 0] > 0.99] = (1.0, 0.0, 0.0)
    alb[-n[:, 0] > 0.99] = (0.0, 1.0, 0.0)
    return alb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401  (before the library: one ROCm runtime for both)
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import DEFAULT_SCENE, make_app
    xyz, idx = abi.load_obj(DEFAULT_SCENE)
    n = len(idx)
    box = short_box(xyz, idx)
    assert box.sum() == 10
    tri = np.arange(n, dtype=np.uint32)      # one material per triangle
    mats = np.zeros((n, 6), np.float32)
    mats[:, :3] = normal_key_albedo(xyz, idx)
    colour, ior = (0.9, 0.9, 0.9), 1.5
    variants = {"diffuse": None, "mirror": "specular", "glass_1.5": "dielectric"}

    def app_of(g):
        app = make_app(a.width, a.height, max_segments=a.segments, iterations=5)
        if g is None:
            app.backend.ctx.set_materials(tri, mats)
        elif g == "specular":
            app.backend.ctx.set_materials_ext(tri, abi.materials_ext(mats, {int(t): (colour, 0.0) for t in np.flatnonzero(box)}))
        else:
            app.backend.ctx.set_materials_ext(tri, abi.materials_ext(mats, None, {int(t): (colour, ior) for t in np.flatnonzero(box)}))
        return app
    apps = {name: app_of(g) for name, g in variants.items()}

    def run(app, frames):
        for f in range(frames):
            app.drawScene(("J",) if f & 1 else ("L",))     # the light moves: nothing is reused
        app.backend.sync()
    ms = {name: [] for name in apps}
    for _ in range(a.repeats):
        for name, app in apps.items():
            run(app, a.warmup)
            t0 = time.perf_counter()
            run(app, a.frames)
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
    out = {"size": [a.width, a.height], "segments": a.segments, "frames": a.frames, "repeats": a.repeats, "box_triangles": int(box.sum()),
           "frame_ms": {k: [round(x, 4) for x in v] for k, v in ms.items()},
           "frame_ms_median": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
           "trace_kernel_us": kernels, "queries_per_pixel": rays}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
