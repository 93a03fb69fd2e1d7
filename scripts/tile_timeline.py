#!/usr/bin/env python3
"""Timeline of the workgroups of the last K0 / K2 launch of a frame (the TIMELINE build of the library:
scripts/build_variant.sh timeline -DRTPT_TILE_TIMELINE=1): how many workgroups are resident over time, how long a
workgroup lives by the time it starts, where the launch's tail is.

    RTPT_LIB_PATH=.../variants/librtpt_timeline.so python scripts/tile_timeline.py [--strip 3/8] [--workload 4k] [--out f.json]

--fused-final: the tracing launch of a frame at rest, which carries the final filter pass of the frame before it
(k_pathtrace_final) — tiles, run workgroups and filter workgroups on one clock, by kind; RTPT_FINAL_FRONT sizes the filter groups,
RTPT_EMPTY_RUN the runs of tiles in the columns no triangle reaches.  --camera 30,1,6: a frame of nothing but such columns.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fused_final_report(fn, W, rows, bucket_us, res, runs=None):
    """The tracing launch that carries the previous frame's final pass (k_pathtrace_final), tiles and filter workgroups on one
    clock: resident workgroups per bucket by kind, when each filter group's last workgroup ends, where the sky phase starts (the
    first dispatch-order eighth of the tiles whose mean lifetime is below a quarter of the first eighth's), the launch span.
    runs: rtpt_debug_empty_run_info of that launch, or None (a library without it).  The tiles its run workgroups serve have no
    record of their own (theirs is an earlier launch's): only the columns served as tiles are read, and the run workgroups are a
    kind of their own, recorded with the filter workgroups (role 3)."""
    gx, gy = (W + 63) // 64, (rows + 3) // 4
    nb = gx * gy
    buf = (C.c_ulonglong * (3 * nb))()
    assert fn(1, buf, nb) == 0
    t_all = np.frombuffer(buf, dtype=np.uint64).reshape(nb, 3).astype(np.int64)
    # the tiles in dispatch order: column by column from the middle outwards (csrc/final_split.hpp: tile_order_column); the
    # records are indexed by tile (by * gx + bx)
    order = []
    for col in range(gx):
        bx = (gx - 1) // 2 + (col + 1) // 2 if col & 1 else (gx - 1) // 2 - col // 2
        order.extend(by * gx + bx for by in range(gy))
    order = np.array(order)
    if runs and runs["run_workgroups"]:
        print(f"runs: {runs['full_columns']} of {gx} columns as tiles, {runs['run_workgroups']} run workgroups of at most {runs['run_len']} tiles "
              f"serve {runs['run_tiles']} tiles")
        order = order[:runs["full_columns"] * gy]
        res["runs"] = runs
    nb = len(order)
    if nb == 0:   # no column is reached: the clock starts with the filter workgroups
        t = np.zeros((0, 3), np.int64)
    else:
        t = t_all[order]
    nf = 1 << 16
    fbuf = (C.c_ulonglong * (3 * nf))()
    assert fn(2, fbuf, nf) == 0
    f = np.frombuffer(fbuf, dtype=np.uint64).reshape(nf, 3)
    role = (f[:, 2] >> np.uint64(48)).astype(np.int64)
    f = f.astype(np.int64)
    # records of the launch the tiles belong to (a record keeps what an earlier launch with more filter workgroups left there)
    if nb:
        lo, hi = t[:, 0].min() - 100000, t[:, 1].max() + 100000
    else:
        lo, hi = f[:, 0].max() - 100000, f[:, 0].max() + 100000
    live = (f[:, 0] != 0) & (f[:, 0] >= lo) & (f[:, 0] <= hi)
    if not live.any():
        print("fused launch: the last tracing launch carried no final pass")
        return
    base = min(t[:, 0].min() if nb else f[live, 0].min(), f[live, 0].min())
    end = max(t[:, 1].max() if nb else 0, f[live, 1].max())
    span = (end - base) / 100.0
    kinds = [("tiles", t[:, 0], t[:, 1])]
    for r, name in ((1, "front"), (3, "runs"), (2, "tail")):
        m = live & (role == r)
        if m.any():
            kinds.append((name, f[m, 0], f[m, 1]))
    print(f"fused launch (tracing tiles of frame n + 1, final pass of frame n): span {span:.1f} us; " +
          ", ".join(f"{len(s)} {name}" for name, s, _ in kinds))
    nbk = int(span / bucket_us) + 1
    print(f"   resident per {bucket_us:.0f} us (" + " + ".join(name for name, _, _ in kinds) + "):")
    rows_out = []
    for b in range(nbk):
        m = base + (b + 0.5) * bucket_us * 100.0
        rows_out.append([int(np.count_nonzero((s <= m) & (e > m))) for _, s, e in kinds])
    print("   " + " ".join("+".join(str(v) for v in r) for r in rows_out))
    out = {"span_us": float(span), "kinds": [k[0] for k in kinds], "resident": rows_out, "bucket_us": bucket_us}
    for name, s, e in kinds[1:]:
        lt = (e - s) / 100.0
        print(f"   {name} group: first start {(s.min() - base) / 100.0:.1f} us, last start {(s.max() - base) / 100.0:.1f} us, first end "
              f"{(e.min() - base) / 100.0:.1f} us, last end {(e.max() - base) / 100.0:.1f} us; lifetime min {lt.min():.1f} median {np.median(lt):.1f} max {lt.max():.1f} us")
        out[name] = {"workgroups": int(len(s)), "first_start_us": float((s.min() - base) / 100.0), "last_end_us": float((e.max() - base) / 100.0)}
    res["fused_final"] = out
    if nb == 0:
        return
    print(f"   tiles: first start {(t[:, 0].min() - base) / 100.0:.1f} us, last start {(t[:, 0].max() - base) / 100.0:.1f} us, last end {(t[:, 1].max() - base) / 100.0:.1f} us")
    s_us, dur = (t[:, 0] - base) / 100.0, (t[:, 1] - t[:, 0]) / 100.0
    eighths = np.array_split(np.arange(nb), 8)
    means = [dur[q].mean() for q in eighths]
    print("   tiles by dispatch order (eighths): first start us / mean lifetime us: " + " ".join(f"{s_us[q].min():.0f}/{m:.1f}" for q, m in zip(eighths, means)))
    sky = next((i for i, m in enumerate(means) if m < means[0] / 4), None)
    if sky is None:
        print("   sky phase: no eighth's mean lifetime is below a quarter of the first eighth's")
    else:
        q = eighths[sky]
        print(f"   sky phase: from eighth {sky} (tile {q[0]} of {nb} in dispatch order, {100.0 * q[0] / nb:.1f} % of the list), first start {s_us[q].min():.1f} us; "
              f"from there {nb - q[0]} tiles, mean lifetime {dur[q[0]:].mean():.1f} us, the launch has {span - s_us[q].min():.1f} us left")
        out["sky"] = {"eighth": sky, "tile": int(q[0]), "start_us": float(s_us[q].min())}
    res["fused_final"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fused-final", action="store_true",
                    help="report the last tracing launch as the one that carries the previous frame's final pass (frames at rest; "
                         "RTPT_FINAL_FRONT places the filter workgroups) instead of the frame's separate launches")
    ap.add_argument("--camera", default=None, metavar="X,Y,Z",
                    help="cameraOrigin (default -0.001,1,6; 30,1,6 looks past the box: every tile column sees only sky)")
    ap.add_argument("--strip", default=None, metavar="R/N")
    ap.add_argument("--workload", default="4k")
    ap.add_argument("--splits", default=None, metavar="0,A,...,H", help="with --strip R/N: unequal strips (strips.StripPlan.splits)")
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--bucket-us", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lpt", action="store_true",
                    help="experiment: after the first measurement, hand K2 its tiles longest-first (by the lifetimes just measured) "
                         "and measure again — what a longest-processing-time-first dispatch order is worth")
    args = ap.parse_args()
    import bench
    from real_time_path_tracing_with_spatiotemporal_filtering_amd import abi, scenes
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import DEFAULT_SCENE, make_app
    lib = abi.load()
    try:
        fn = lib.rtpt_debug_timeline
    except AttributeError:
        sys.exit("this library was not built with -DRTPT_TILE_TIMELINE=1")
    fn.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.c_uint32]
    wl = bench.WORKLOADS[args.workload]
    r, n = map(int, args.strip.split("/")) if args.strip else (0, 1)
    extra = {}
    if wl.get("instanced"):
        xyz, idx = abi.load_obj(DEFAULT_SCENE)
        vx, ti, xf, cam, zfar = scenes.instanced_cornell(xyz, idx)
        extra = dict(mesh=(vx, ti), instance_xforms=xf, cameraOrigin=cam, z_far=zfar, lightPos=(1.0, float(cam[1]), float(cam[2]) - 8.0))
    if args.camera:
        extra["cameraOrigin"] = tuple(float(v) for v in args.camera.split(","))
    app = make_app(wl["width"], wl["height"], max_segments=wl["max_segments"], iterations=wl["iterations"], rank=r, world=n,
                   mode="redundant", torch_planes=False, splits=tuple(int(v) for v in args.splits.split(",")) if args.splits else (), **extra)
    for _ in range(args.frames):
        app.drawScene(())
    app.backend.ctx.sync()
    if args.fused_final:   # the last frame's tracing launch carried the final pass of the frame before it; nothing has run since
        res = {"workload": args.workload, "final_front": os.environ.get("RTPT_FINAL_FRONT")}
        rows_of = app.plan.raytrace_rows()
        print(f"RTPT_FINAL_FRONT={res['final_front']} RTPT_EMPTY_RUN={os.environ.get('RTPT_EMPTY_RUN')} camera={args.camera}")
        info = getattr(app.backend.ctx, "empty_run_info", None)   # (absent in a library older than the runs)
        fused_final_report(fn, wl["width"], rows_of[1] - rows_of[0], args.bucket_us, res, info() if info else None)
        if args.out:
            json.dump(res, open(args.out, "w"))
        return
    # the filter's launches (atrous_chain.hip / atrous.hip, experiments/span_instrumentation.inc) fold every workgroup of every
    # launch since the last clear: re-arm them, draw ONE frame, and every launch of that frame sits on one clock
    spans, reader_names = [], {}
    for reader, slots, names in (("rtpt_debug_chain_span", 4, ["chain (1,2)", "chain (3,4)", "chain (1,2) final", "chain (3,4)+ final"]),
                                 ("rtpt_debug_comb_span", 2, ["single pass k < N", "final pass"])):
        f = getattr(lib, reader, None)
        if f is not None:
            f.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
            assert f(None, 1) == 0
            spans.append((f, slots, names))
            reader_names[id(f)] = reader
    if spans:
        app.drawScene(())
        app.backend.ctx.sync()
    W = wl["width"]
    res = {"strip": args.strip, "workload": args.workload}
    for round_ in range(2 if args.lpt else 1):
      if round_ == 1:
        fo = lib.rtpt_debug_tile_order
        fo.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
        order = np.argsort(-k2_dur, kind="stable").astype(np.uint32)   # timeline entries are indexed by tile (by * gx + bx)
        assert fo(order.ctypes.data_as(C.POINTER(C.c_uint32)), len(order)) == 0
        import time
        for _ in range(args.frames):
            app.drawScene(())
        app.backend.ctx.sync()
        t0 = time.perf_counter()
        for _ in range(200):
            app.drawScene(())
        app.backend.ctx.sync()
        print(f"--- tiles longest-first: {(time.perf_counter() - t0) / 200 * 1e3:.4f} ms per frame")
      elif args.lpt:
        import time
        t0 = time.perf_counter()
        for _ in range(200):
            app.drawScene(())
        app.backend.ctx.sync()
        print(f"--- built-in order: {(time.perf_counter() - t0) / 200 * 1e3:.4f} ms per frame")
      for kernel, name, rows_of in ((0, "K0+K1", app.plan.gbuffer_rows()), (1, "K2", app.plan.raytrace_rows())):
          rows = rows_of[1] - rows_of[0]
          gx, gy = (W + 63) // 64, (rows + 3) // 4
          nb = gx * gy
          buf = (C.c_ulonglong * (3 * nb))()
          assert fn(kernel, buf, nb) == 0
          t = np.frombuffer(buf, dtype=np.uint64).reshape(nb, 3)
          t0 = t[:, 0].astype(np.int64)
          t1 = t[:, 1].astype(np.int64)
          base = t0.min()
          s_us = (t0 - base) / 100.0   # 100 MHz wall clock
          e_us = (t1 - base) / 100.0
          dur = e_us - s_us
          if kernel == 1:
              k2_dur = dur
          span = e_us.max()
          nbk = int(span / args.bucket_us) + 1
          resident = np.zeros(nbk)
          for b in range(nbk):   # workgroups resident at the bucket's middle
              m = (b + 0.5) * args.bucket_us
              resident[b] = np.count_nonzero((s_us <= m) & (e_us > m))
          order = np.argsort(s_us)
          q = np.array_split(order, 8)
          print(f"{name}: {nb} workgroups ({gx} x {gy}), launch span {span:.1f} us, sum of lifetimes {dur.sum():.0f} us "
                f"(= {dur.sum() / span:.0f} resident on average), longest {dur.max():.1f} us, median {np.median(dur):.1f} us")
          print("   resident per %.0f us:" % args.bucket_us, " ".join(f"{int(v)}" for v in resident))
          print("   by start order (eighths): start us / mean lifetime us:",
                " ".join(f"{s_us[i].mean():.0f}/{dur[i].mean():.1f}" for i in q))
          # the last workgroups to end: where they sit in the grid and when they started
          last = np.argsort(e_us)[-8:]
          print("   last to end (block x, y, start, end):", [(int(b % gx), int(b // gx), round(float(s_us[b]), 1), round(float(e_us[b]), 1)) for b in last])
          xcc = (t[:, 2] >> np.uint64(32)).astype(np.int64) & 0xF
          print("   workgroups per XCC:", np.bincount(xcc, minlength=8).tolist())
          res[name] = {"workgroups": nb, "grid": [gx, gy], "span_us": float(span), "resident": resident.tolist(),
                       "bucket_us": args.bucket_us, "start_us": s_us.round(2).tolist(), "end_us": e_us.round(2).tolist(),
                       "abs_start": t0.tolist(), "abs_end": t1.tolist()}
    # K0 + K1 + K2 as ONE launch (the default): both kinds of workgroups on one clock — the G-buffer tiles are dispatched behind the
    # tracing tiles and run while those drain
    if "K0+K1" in res and "K2" in res and "abs_start" in res["K0+K1"]:
        a0, a1 = np.array(res["K0+K1"]["abs_start"]), np.array(res["K0+K1"]["abs_end"])
        b0, b1 = np.array(res["K2"]["abs_start"]), np.array(res["K2"]["abs_end"])
        base = min(a0.min(), b0.min())
        if abs(a0.min() - b0.min()) < 100000:   # within 1 ms of each other: the same launch
            span = (max(a1.max(), b1.max()) - base) / 100.0
            nbk = int(span / args.bucket_us) + 1
            rows = []
            for b in range(nbk):
                m = base + (b + 0.5) * args.bucket_us * 100.0
                rows.append((int(np.count_nonzero((b0 <= m) & (b1 > m))), int(np.count_nonzero((a0 <= m) & (a1 > m)))))
            print(f"one launch: span {span:.1f} us; resident per {args.bucket_us:.0f} us (tracing tiles + G-buffer tiles):",
                  " ".join(f"{t}+{g}" for t, g in rows))
            print(f"   first G-buffer tile starts at {(a0.min() - base) / 100.0:.1f} us, last tracing tile ends at {(b1.max() - base) / 100.0:.1f} us, "
                  f"last G-buffer tile at {(a1.max() - base) / 100.0:.1f} us")
            res["one_launch"] = {"span_us": float(span), "resident_trace_gbuffer": rows}
        # the whole frame on that clock: the launches of the filter behind the trace
        raws, raw_idx = {}, {}
        frame = [("K0+K1+K2", base, max(a1.max(), b1.max()), float((a1 - a0).sum() + (b1 - b0).sum()) / 100.0, len(a0) + len(b0), None)]
        for f, slots, names in spans:
            buf = (C.c_ulonglong * (slots * 4 + slots * 132))()
            assert f(buf, 0) == 0
            v = np.frombuffer(buf, dtype=np.uint64).astype(np.int64)
            for sl in range(slots):
                first, last_, life, n = v[4 * sl: 4 * sl + 4]
                if n:
                    st = v[4 * slots + 132 * sl: 4 * slots + 132 * (sl + 1)]
                    frame.append((names[sl], first, last_, life / 100.0, int(n), st if st[2] > 0 else None))
                    fr = getattr(lib, reader_names[id(f)] + "_raw", None)
                    if fr is not None:
                        fr.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.c_uint32]
                        rb = (C.c_ulonglong * (3 * 4096))()
                        if fr(sl, rb, 4096) == 0:
                            rr = np.frombuffer(rb, dtype=np.uint64).astype(np.int64).reshape(4096, 3)
                            raws[names[sl]] = rr[rr[:, 0] != 0]
                            raw_idx[names[sl]] = np.nonzero(rr[:, 0] != 0)[0]
        frame.sort(key=lambda e: e[1])
        if len(frame) > 1 and frame[-1][2] - base < 10000000:   # the same frame
            print("the frame on one clock (us from the first tracing tile; gap = idle time since the previous launch's last workgroup ended):")
            prev_end = None
            res["frame"] = []
            for name, first, last_, life, n, st in frame:
                gap = (first - prev_end) / 100.0 if prev_end is not None else 0.0
                print(f"   {name:20s} start {(first - base) / 100.0:7.1f}  end {(last_ - base) / 100.0:7.1f}  span {(last_ - first) / 100.0:6.1f}  gap {gap:5.1f}  "
                      f"{n:5d} workgroups, mean lifetime {life / n:6.1f}")
                e = {"launch": name, "start_us": (first - base) / 100.0, "end_us": (last_ - base) / 100.0, "gap_us": gap, "workgroups": n,
                     "mean_lifetime_us": life / n}
                raw = raws.get(name)
                if raw is not None and len(raw):
                    lt = (raw[:, 1] - raw[:, 0]) / 100.0
                    st0 = (raw[:, 0] - first) / 100.0
                    hw = raw[:, 2]
                    cu = ((hw >> 32) & 0xF) * 4096 + ((hw >> 13) & 0x7) * 512 + ((hw >> 12) & 0x1) * 256 + ((hw >> 8) & 0xF)
                    per_cu = {c: int(np.count_nonzero(cu == c)) for c in np.unique(cu)}
                    share = np.array([per_cu[c] for c in cu])
                    print(f"      lifetimes us: min {lt.min():.1f}  median {np.median(lt):.1f}  p90 {np.percentile(lt, 90):.1f}  max {lt.max():.1f};  "
                          f"starts: median {np.median(st0):.1f}  p90 {np.percentile(st0, 90):.1f}  last {st0.max():.1f};  {len(per_cu)} CUs used, "
                          "workgroups per CU -> CUs / mean lifetime: " +
                          "  ".join(f"{k}: {sum(1 for v in per_cu.values() if v == k)} / {lt[share == k].mean():.1f}" for k in sorted(set(per_cu.values()))))
                    idx = raw_idx[name]
                    print("      mean lifetime by XCD (workgroup index & 7): " + " ".join(f"{lt[(idx & 7) == x].mean():.1f}" for x in range(8) if np.any((idx & 7) == x)) +
                          ";  by position in the launch (eighths of the workgroup index): " +
                          " ".join(f"{lt[q].mean():.1f}" for q in np.array_split(np.argsort(idx), 8) if len(q)) +
                          ";  end of the first / median / last workgroup: " + f"{(raw[:, 1].min() - first) / 100.0:.1f} / {(np.median(raw[:, 1]) - first) / 100.0:.1f} / {(raw[:, 1].max() - first) / 100.0:.1f}")
                    e["lifetime_us"] = {"min": float(lt.min()), "median": float(np.median(lt)), "p90": float(np.percentile(lt, 90)), "max": float(lt.max())}
                    e["start_us"] = {"median": float(np.median(st0)), "p90": float(np.percentile(st0, 90)), "last": float(st0.max())}
                if st is not None:
                    T = int(min(st[2], 128))
                    steps = np.diff(np.concatenate([[st[1]], st[3:3 + T]])) / 100.0
                    print(f"      probe workgroup: starts {(st[0] - first) / 100.0:.1f} us into the launch, prologue {(st[1] - st[0]) / 100.0:.1f} us, {int(st[2])} steps, "
                          f"mean {steps.mean():.2f} us: " + " ".join(f"{x:.1f}" for x in steps))
                    e["probe"] = {"prologue_us": (st[1] - st[0]) / 100.0, "steps_us": steps.round(2).tolist()}
                res["frame"].append(e)
                prev_end = last_
            print(f"   frame: {(frame[-1][2] - base) / 100.0:.1f} us from the first workgroup's start to the last one's end")
        for k in ("K0+K1", "K2"):
            res[k].pop("abs_start", None)
            res[k].pop("abs_end", None)
    if args.out:
        json.dump(res, open(args.out, "w"))


if __name__ == "__main__":
    main()
