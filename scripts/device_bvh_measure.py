"""Device-side BVH builds (csrc/bvh_build.hip: LBVH; csrc/bvh_build_sah.hip: the host's SAH tree built on the device) against
the host SAH builder, on the GPU in front of you:

* build_ms / upload_ms of rtpt_scene_upload for the Cornell box, a 3,000-triangle soup and the 1,152,000-triangle lattice
  (BASELINE configs[4]), each builder, after one warm-up upload (code objects load lazily);
* on the lattice under a sheared model: the frame time with the refit tree, the cost of rtpt_scene_rebuild, the frame time
  with the rebuilt tree — the figure that says when a rebuild pays; once per builder that can rebuild;
* the same uploads with RTPT_FLAG_DEVICE_FLATTEN (builders device_flat, device_sah_flat: csrc/scene_flatten.hip), with
  what rtpt_debug_upload_info says went over the bus;
* --instances: a lattice frame at rest, with ubo.model changing every frame, and with rtpt_scene_set_instances every frame.
  A library without these (an older commit) runs the legs it has.

    python scripts/device_bvh_measure.py [--frames 30] [--small]      # one JSON line per measurement
    python scripts/device_bvh_measure.py --instances-only --flags 0x7000   # moving instances alone, one set of flags
    rocprofv3 --kernel-trace --stats -d out -- python scripts/device_bvh_measure.py --builds-only   # the per-kernel split
    ... --builds-only --builders device_sah --scenes lattice --reps 1      # of one builder on one scene
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--small", action="store_true", help="1080p frames instead of 4K")
    ap.add_argument("--builds-only", action="store_true")
    ap.add_argument("--builders", default="device,device_sah,host",
                    help="comma list of device, device_sah, host (uploads and rebuild legs), device_flat, device_sah_flat (uploads)")
    ap.add_argument("--instances", action="store_true", help="also the moving-instances frames")
    ap.add_argument("--instances-only", action="store_true")
    ap.add_argument("--flags", type=lambda v: int(v, 0), default=None, help="flags of the moving-instances leg (default: 0 and 0x7000)")
    ap.add_argument("--scenes", default="cornell,soup3000,lattice", help="comma list of the upload scenes")
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    try:
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi, scenes
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import DEFAULT_SCENE, HipBackend, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan
    D = abi.FLAG_DEVICE_BVH_BUILD
    S = D | abi.FLAG_DEVICE_BVH_SAH
    F = getattr(abi, "FLAG_DEVICE_FLATTEN", None)  # None: a library from before the device flatten
    xyz, idx = abi.load_obj(DEFAULT_SCENE)
    rng = np.random.default_rng(707)
    c = rng.uniform(-0.8, 0.8, (3000, 1, 3))
    soup = ((c + rng.normal(0, 0.08, (3000, 3, 3))).astype(np.float32).reshape(-1, 3), np.arange(9000, dtype=np.uint32).reshape(-1, 3))
    vx, ti, xf, cam, zfar = scenes.instanced_cornell(xyz, idx)
    cases = {"cornell": (xyz, idx, None), "soup3000": soup + (None,), "lattice": (vx, ti, xf)}

    def upload(flags, mesh):
        cfg = abi.config_default(64, 64)
        cfg.flags = flags
        with abi.Context(cfg) as ctx:
            t0 = time.perf_counter()
            ctx.scene_upload(*mesh)
            wall = (time.perf_counter() - t0) * 1e3
            moved = ctx.debug_upload_info() if F else {}
            return dict(ctx.scene_build_info(), wall_ms=round(wall, 3), **moved)

    upload(D, cases["soup3000"])  # warm-up
    upload(S, cases["soup3000"])
    upload(0, cases["soup3000"])
    asked = args.builders.split(",")
    builders = [(label, flags) for label, flags in (("device", D), ("device_sah", S), ("host", 0)) if label in asked]
    flat = [(label, flags | F) for label, flags in (("device_flat", D), ("device_sah_flat", S)) if F and label in asked]
    if flat:
        upload(D | F, cases["soup3000"])  # warm-up of the flatten kernels
    for name, mesh in cases.items():
        if name not in args.scenes.split(",") or args.instances_only:
            continue
        for rep in range(args.reps):
            for label, flags in builders + flat:
                print(json.dumps({"what": "upload", "scene": name, "asked": label, "rep": rep, **upload(flags, mesh)}), flush=True)
    if args.builds_only:
        return
    if args.instances or args.instances_only:
        moving_instances(args, abi, (vx, ti, xf, cam, zfar), [args.flags] if args.flags is not None else [0, S | F] if F else [0])
    if args.instances_only:
        return

    w, h = (1920, 1080) if args.small else (3840, 2160)
    n = 5
    shear = np.eye(4)
    shear[:3, :3] = [[1.0, 0.8, 0.0], [0.0, 1.0, 0.0], [0.6, 0.0, 1.0]]
    shear = np.ascontiguousarray(shear.astype(np.float32).T).ravel()
    for upload_flags in [flags for _, flags in builders[::-1]]:
        be = HipBackend(w, h, StripPlan(h, 1, 0, n), max_segments=8, flags=upload_flags)
        app = PathTracingApplication(be, w, h, n, cameraOrigin=cam, z_far=zfar, lightPos=(1.0, float(cam[1]), float(cam[2]) - 8.0))
        app.objVertices, app.objIndices = vx, ti
        app.buildAccelerationStructure(xf)
        ctx = be.ctx

        def frames(k):
            for _ in range(5):
                app.drawScene(())
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(k):
                app.drawScene(())
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / k

        base = frames(args.frames)
        app.modelMatrix = shear
        refit = frames(args.frames)
        t0 = time.perf_counter()
        ctx.scene_rebuild()
        ctx.sync()
        rebuild_wall = (time.perf_counter() - t0) * 1e3
        info = ctx.scene_build_info()
        rebuilt = frames(args.frames)
        print(json.dumps({"what": "rebuild_vs_refit", "scene": "lattice sheared", "size": [w, h], "uploaded_by": {0: "host", D: "device", S: "device_sah"}[upload_flags],
                          "rebuilt_by": "device_sah" if upload_flags == S else "device",
                          "ms_per_frame_identity": round(base, 4), "ms_per_frame_refit_tree": round(refit, 4),
                          "ms_per_frame_rebuilt_tree": round(rebuilt, 4), "rebuild_wall_ms": round(rebuild_wall, 3),
                          "rebuild_build_ms": round(info["build_ms"], 3), "depth": info["depth"]}), flush=True)
        be.close()


def moving_instances(args, abi, scene, flag_sets):
    """ms per lattice frame (8 segments): at rest, with ubo.model changing every frame (re-pose + refit), and with
    rtpt_scene_set_instances every frame (flatten + re-pose + refit); the three legs twice, interleaved"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import HipBackend, PathTracingApplication
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan
    vx, ti, xf, cam, zfar = scene
    w, h = (1920, 1080) if args.small else (3840, 2160)
    n = 5
    poses = []
    for f in range(7):  # the poses of test_device_refit_equals_host_refit_and_does_not_stall_the_frame, as transforms too
        a, dx = 0.01 * f, 0.02 * (f % 5)
        c, s = np.cos(a), np.sin(a)
        m = np.array([[c, 0, s, dx], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float32)
        x = xf.reshape(-1, 3, 4).astype(np.float64)
        moved = np.concatenate([m[:3, :3].astype(np.float64) @ x[:, :, :3], (x[:, :, 3] @ m[:3, :3].T.astype(np.float64) + m[:3, 3])[:, :, None]], 2)
        poses.append((np.ascontiguousarray(m.T).ravel(), np.ascontiguousarray(moved.astype(np.float32).reshape(-1, 12))))
    for flags in flag_sets:
        be = HipBackend(w, h, StripPlan(h, 1, 0, n), max_segments=8, flags=flags)
        app = PathTracingApplication(be, w, h, n, cameraOrigin=cam, z_far=zfar, lightPos=(1.0, float(cam[1]), float(cam[2]) - 8.0))
        app.objVertices, app.objIndices = vx, ti
        app.buildAccelerationStructure(xf)
        ctx = be.ctx
        can_move = hasattr(app, "setInstanceTransforms")

        def frames(k, leg):
            t0 = None
            for f in range(-5, k):
                if f == 0:
                    ctx.sync()
                    t0 = time.perf_counter()
                if leg == "model":
                    app.modelMatrix = poses[f % 7][0]
                elif leg == "instances":
                    app.setInstanceTransforms(poses[f % 7][1])
                app.drawScene(())
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3 / k

        out = {"what": "moving_instances", "size": [w, h], "flags": hex(flags), "frames": args.frames}
        for rep in range(2):
            for leg in ("rest", "model") + (("instances",) if can_move else ()):
                app.modelMatrix = np.eye(4, dtype=np.float32).ravel()
                if can_move:
                    app.setInstanceTransforms(xf)
                out[f"ms_per_frame_{leg}_{rep}"] = round(frames(args.frames, leg), 4)
        if can_move:
            out.update(ctx.debug_upload_info())
        print(json.dumps(out), flush=True)
        be.close()


if __name__ == "__main__":
    main()
