"""ORACLE — TEST INFRASTRUCTURE ONLY.

Shared by tests/test_reference_shaders.py and tests/golden/make_refshader.py: the frame script, the oracle-side record of
a frame, the runs of the reference's shader text on the same inputs, and the error measures the bars are stated in.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle as O
from oracle.refshader import refshader as R

# frames 0-3: nothing, light moves, camera moves, light moves and changes colour (the ",E,J,Q"-style key script).
# The camera move first tried, (0.1, 0.05, 0), put 0.85 % of the 65x33 frame's foreground within 1e-3 px of an integer
# reprojected position (R32 against R64, the reference text alone), above the 0.5 % condition; with (0.07, 0.03, 0) no
# pixel of any size lies there.  The pose was changed, not the cap.
SCRIPT = (
    dict(),
    dict(move_light=(-0.1, 0.0, 0.0)),
    dict(move_camera=(0.07, 0.03, 0.0)),
    dict(move_light=(0.05, 0.1, 0.1), light_color=(0.9, 0.6, 0.3)),
)
SIZES = ((64, 48), (65, 33), (100, 5))  # the fixture's size and two ragged sizes of test_fuzz_gpu.py's lists
SEGMENTS = (1, 2, 8, 32)
ITERATIONS = (1, 2, 5, 9)
COLOUR_FLOOR = 1e-2  # colours: |a - b| / max(|b|, floor); below the floor the measure is absolute / floor
MAX_DIVERGED = 0.01  # share of pixels per frame whose id sequences may differ
MAX_ON_INTEGER = 0.005  # share of foreground pixels whose R64 screen position lies within 1e-3 px of an integer


def colour_err(a, b):
    """largest |a - b| / max(|b|, COLOUR_FLOOR) over the finite entries of b; non-finite entries must match in kind"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    fin = np.isfinite(b)
    kind = (np.isnan(a) == np.isnan(b)) & (np.isposinf(a) == np.isposinf(b)) & (np.isneginf(a) == np.isneginf(b))
    if not kind.all():
        return np.inf
    if not fin.any():
        return 0.0
    return float((np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), COLOUR_FLOOR)).max())


def abs_err(a, b):
    """largest |a - b| with NaN == NaN (D7: 0/0 where both Phong colours are 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if not (np.isnan(a) == np.isnan(b)).all():
        return np.inf
    fin = ~np.isnan(b)
    return float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0


def same_paths(id_a, n_a, id_b, n_b):
    """pixels whose recorded closest-hit sequences (ids and count) agree to the end"""
    return (n_a == n_b) & (id_a == id_b).all(-1)


def copy_struct(s):
    return type(s).from_buffer_copy(bytes(s))


class Frame:
    """what the oracle computed for one frame, and the inputs it computed it from"""


def oracle_frames(W, H, tris, max_segments, iterations, script=SCRIPT):
    app = O.OracleApp(W, H, tris, max_segments=max_segments, iterations=iterations)
    for step in script:
        f = Frame()
        f.W, f.H, f.max_segments, f.iterations = W, H, max_segments, iterations
        f.history = app.history
        lut_prev = app.lut_prev
        if "light_color" in step:
            app.light_color = np.array(step["light_color"], np.float32)
        f.fo = app.draw_scene(move_camera=step.get("move_camera"), move_light=step.get("move_light"))
        f.lut_prev = f.fo.lut if lut_prev is None else lut_prev
        f.pc, f.ubo, f.cfg, f.tris = copy_struct(app.pc), copy_struct(app.ubo), app.cfg, app.tris
        f.traced, f.rays, f.hit_id, f.seq_id, f.seq_n, f.seq_end, f.dir0 = O.raytrace_seq(app.cfg, f.pc, app.tris)
        assert np.array_equal(f.traced.view(np.uint32), f.fo.traced.view(np.uint32)) and f.rays == f.fo.rays
        yield f


def oracle_filter_chain(f, traced, iterations, history="frame"):
    """the oracle's K3 chain on `traced`: per-iteration outputs and the final pass's reprojected pixels"""
    pc, cur, outs, pp = copy_struct(f.pc), np.ascontiguousarray(traced, np.float32), [], None
    pc.maxWaveletIteration = iterations
    hist = f.history if history == "frame" else history
    for k in range(1, iterations + 1):
        pc.waveletIteration = k
        res = O.atrous(f.cfg, pc, f.ubo, cur, f.fo.depth, f.fo.vis, f.fo.lut, f.lut_prev, f.fo.worldpos, hist,
                       want_prev_pixel=(k == iterations))
        cur, pp = res if k == iterations else (res, None)
        outs.append(cur)
    return outs, pp


def ref_filter_chain(arith, f, traced, iterations, history="frame", path=None):
    """the reference text's K3 chain on `traced`, ping-pong and final-pass rule as the oracle's host mirror has them"""
    pc, cur, outs, pp = copy_struct(f.pc), traced, [], None
    pc.maxWaveletIteration = iterations
    hist = f.history if history == "frame" else history
    for k in range(1, iterations + 1):
        pc.waveletIteration = k
        filtered, blend, ppk = R.temporal_filter(arith, f.W, f.H, pc, f.ubo, cur, f.fo.depth, f.fo.vis, f.fo.lut, f.lut_prev,
                                                 f.fo.worldpos, hist, path=path)
        cur = blend if (k == iterations and k & 1) else filtered
        pp = ppk if k == iterations else None
        outs.append(cur)
    return outs, pp


def ref_raytrace(arith, f, path=None, num_samples=1):
    return R.raytrace(arith, f.W, f.H, f.pc, f.tris, f.max_segments, num_samples, path=path)


def ref_gradient(arith, f, path=None):
    return R.temporal_gradient(arith, f.W, f.H, f.pc, f.fo.vis, f.fo.worldpos, f.fo.lut, f.lut_prev, path=path)


def screen_pos_on_integer(f, eps=1e-3):
    """foreground pixels whose reprojected screen position, evaluated in float64 from the same planes, lies within eps
    of an integer: there ivec2() of a binary32 and of a binary64 evaluation may legitimately differ"""
    H, W = f.fo.vis.shape
    vis = f.fo.vis.astype(np.int64)
    lut = np.asarray(f.lut_prev, np.float64).reshape(-1, 3, 4)[:, :, :3]
    a, b, c = lut[vis, 0], lut[vis, 1], lut[vis, 2]
    p = f.fo.worldpos[..., :3].astype(np.float64)

    def area(u, v, w):
        return 0.5 * np.linalg.norm(np.cross(v - u, w - u), axis=-1)
    with np.errstate(all="ignore"):
        t = area(a, b, c)
        bc = np.stack([area(p, b, c) / t, area(a, p, c) / t, area(a, b, p) / t], -1)
        wp = bc[..., 0:1] * a + bc[..., 1:2] * b + bc[..., 2:3] * c
        P = np.array(f.ubo.projPrev[:], np.float64).reshape(4, 4).T
        V = np.array(f.ubo.viewPrev[:], np.float64).reshape(4, 4).T
        clip = np.concatenate([wp, np.ones((H, W, 1))], -1) @ (P @ V).T
        sx = (clip[..., 0] / clip[..., 3] * 0.5 + 0.5) * W
        sy = (clip[..., 1] / clip[..., 3] * 0.5 + 0.5) * H
        near = (np.abs(sx - np.rint(sx)) < eps) | (np.abs(sy - np.rint(sy)) < eps)
    return near & (vis > 0)


def sphere_scene():
    """a non-Cornell scene: test_traversal_gpu.py's UV sphere, lifted into the camera's view (normals of every direction:
    all three albedo branches of raytrace.comp.glsl:155-163 are taken) over a floor quad"""
    import os
    import sys
    here = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.join(here, "tests"))
    try:
        from test_traversal_gpu import _sphere
    finally:
        sys.path.pop(0)
    xyz, idx = _sphere()
    xyz = (xyz + np.array([0.0, 1.0, 0.0], np.float32)).astype(np.float32)
    floor = np.array([[-2, 0.2, -2], [2, 0.2, -2], [2, 0.2, 2], [-2, 0.2, 2]], np.float32)
    n = len(xyz)
    xyz = np.concatenate([xyz, floor]).astype(np.float32)
    idx = np.concatenate([idx, [[n, n + 2, n + 1], [n, n + 3, n + 2]]]).astype(np.uint32)
    return O.flatten(xyz, idx)


PAIRS = (("r32", "r64"), ("oracle", "r32"), ("oracle", "r64"))


def observe(f, iterations=(), path=None):
    """every figure the tests bar, for one frame: {observable: {pair: value}} with pair = "a/b" (a measured against b)"""
    out = {k: {} for k in ("diverged", "traced", "dir0", "lambda", "filtered", "pp_mismatch", "pp_excluded")}
    tr = {"r32": ref_raytrace("f32", f, path), "r64": ref_raytrace("f64", f, path),
          "oracle": dict(image=f.traced, seq_id=f.seq_id, seq_n=f.seq_n, dir0=f.dir0, rays=f.rays)}
    gr = {"r32": ref_gradient("f32", f, path), "r64": ref_gradient("f64", f, path), "oracle": f.fo.gradient}
    for a, b in PAIRS:
        same = same_paths(tr[a]["seq_id"], tr[a]["seq_n"], tr[b]["seq_id"], tr[b]["seq_n"])
        out["diverged"][f"{a}/{b}"] = float(1.0 - same.mean())
        out["traced"][f"{a}/{b}"] = colour_err(tr[a]["image"][same], tr[b]["image"][same])
        out["dir0"][f"{a}/{b}"] = abs_err(tr[a]["dir0"], tr[b]["dir0"])
        out["lambda"][f"{a}/{b}"] = abs_err(gr[a], gr[b])
    near = screen_pos_on_integer(f)
    fg = f.fo.vis > 0
    for n_it in iterations:
        ch = {"oracle": oracle_filter_chain(f, f.traced, n_it), "r32": ref_filter_chain("f32", f, f.traced, n_it, path=path),
              "r64": ref_filter_chain("f64", f, f.traced.astype(np.float64), n_it, path=path)}
        for a, b in PAIRS:
            key = f"{a}/{b}"
            e = max(colour_err(x, y) for x, y in zip(ch[a][0], ch[b][0]))
            out["filtered"][key] = max(out["filtered"].get(key, 0.0), e)
            if f.pc.frameNumber > 0 and n_it & 1:  # the history load happens on frames > 0, in the (odd) final pass
                ppa, ppb = ch[a][1], ch[b][1]
                loaded = (ppa[..., 0] != R.NO_LOAD) & (ppb[..., 0] != R.NO_LOAD) if a != "oracle" else (ppb[..., 0] != R.NO_LOAD)
                excl = near if "r64" in (a, b) else np.zeros_like(near)
                bad = (ppa != ppb).any(-1) & loaded & ~excl
                out["pp_mismatch"][key] = max(out["pp_mismatch"].get(key, 0), int(bad.sum()))
                out["pp_excluded"][key] = float(excl.sum() / max(1, fg.sum()))
    out["_runs"] = (tr, gr)
    return out


# ---- the recorded fixture (tests/golden/refshader_cornell_64x48.npz) --------------------------------------------------
# To stay small the file keeps R64 planes rounded to binary32 (the rounding, 6e-8 relative, is two orders below every
# bar) and R32 planes as the integer difference of their bit patterns from those (a few ulp: it compresses to almost
# nothing and reconstructs R32 exactly).  Every frame keeps the final image; the per-iteration filtered colours are
# kept for frame 2 (camera moved: the blend goes through the reprojection) on the central quarter of the image
# (FIX_WINDOW: back wall, both boxes, floor and ceiling edges).  R64's id sequences are kept as XOR with R32's.
FIX_STACK_FRAMES = (2,)


def fix_window(H, W):
    return slice(H // 4, H - H // 4), slice(W // 4, W - W // 4)


def _pack32(r32, r64_as_f32):
    d = r32.view(np.int32).astype(np.int64) - r64_as_f32.view(np.int32).astype(np.int64)
    assert np.abs(d).max() < 2 ** 31
    return d.astype(np.int32)


def _unpack32(delta, r64_as_f32):
    return (r64_as_f32.view(np.int32).astype(np.int64) + delta).astype(np.int32).view(np.float32)


def fixture_planes(f, n_it, path=None):
    """the planes of one frame that the fixture records, from a live run: {name: (r32, r64 rounded to binary32)}"""
    out = {}
    tr = {a: ref_raytrace(a, f, path) for a in ("f32", "f64")}
    out["traced"] = tuple(np.ascontiguousarray(tr[a]["image"][..., :3], np.float32) for a in ("f32", "f64"))
    out["lambda"] = tuple(np.ascontiguousarray(ref_gradient(a, f, path)[..., 0], np.float32) for a in ("f32", "f64"))
    ch = {a: ref_filter_chain(a, f, f.traced.astype(R._dt(a)), n_it, path=path) for a in ("f32", "f64")}
    out["image"] = tuple(np.ascontiguousarray(ch[a][0][-1][..., :3], np.float32) for a in ("f32", "f64"))
    if f.pc.frameNumber in FIX_STACK_FRAMES:
        wy, wx = fix_window(f.H, f.W)
        out["stack"] = tuple(np.stack([o[wy, wx, :3] for o in ch[a][0]]).astype(np.float32) for a in ("f32", "f64"))
    ints = {"seq_id": tuple(tr[a]["seq_id"] for a in ("f32", "f64")), "seq_n": tuple(tr[a]["seq_n"].astype(np.uint8) for a in ("f32", "f64")),
            "prev_pixel": tuple(ch[a][1] for a in ("f32", "f64"))}
    return out, ints


def record_fixture(tris, W, H, seg, n_it):
    fx = {"meta": np.array([W, H, seg, n_it], np.int32)}
    yy, xx = np.mgrid[0:H, 0:W]
    here = np.stack([xx, yy], -1).astype(np.int32)
    for f in oracle_frames(W, H, tris, seg, n_it):
        i = f.pc.frameNumber
        fx[f"pc{i}"] = np.frombuffer(bytes(f.pc), np.uint8)
        fx[f"ubo{i}"] = np.frombuffer(bytes(f.ubo), np.uint8)
        planes, ints = fixture_planes(f, n_it)
        for name, (r32, r64) in planes.items():
            fx[f"{name}_f64_{i}"] = r64
            fx[f"{name}_d32_{i}"] = _pack32(r32, r64)
        for name, (i32, i64) in ints.items():
            if name == "prev_pixel":  # kept as the offset from the pixel's own coordinate; NO_LOAD (frame 0) stays
                i32, i64 = (np.where(v == R.NO_LOAD, R.NO_LOAD, v - here).astype(np.int32) for v in (i32, i64))
            if name == "seq_id":
                assert i32.max() < 256 and i64.max() < 256  # the Cornell box has 36 triangles
                i32, i64 = i32.astype(np.uint8), (i32 ^ i64).astype(np.uint8)
            fx[f"{name}_f32_{i}"] = i32
            fx[f"{name}_f64_{i}"] = i64
    return fx


def load_fixture(path):
    """-> (meta, frames) with frames[i] = dict(pc=bytes, ubo=bytes, f32={...}, f64={...}) of float32 / integer planes"""
    z = np.load(path)
    W, H, seg, n_it = (int(v) for v in z["meta"])
    yy, xx = np.mgrid[0:H, 0:W]
    here = np.stack([xx, yy], -1).astype(np.int32)
    frames = []
    for i in range(len(SCRIPT)):
        fr = dict(pc=z[f"pc{i}"].tobytes(), ubo=z[f"ubo{i}"].tobytes(), f32={}, f64={})
        for name in ("traced", "lambda", "image", "stack"):
            if f"{name}_f64_{i}" in z:
                fr["f64"][name] = z[f"{name}_f64_{i}"]
                fr["f32"][name] = _unpack32(z[f"{name}_d32_{i}"], fr["f64"][name])
        for name in ("seq_id", "seq_n", "prev_pixel"):
            for a in ("f32", "f64"):
                v = z[f"{name}_{a}_{i}"]
                if name == "seq_id":
                    v = v.astype(np.uint16) if a == "f32" else (v ^ z[f"{name}_f32_{i}"]).astype(np.uint16)
                if name == "prev_pixel":
                    v = np.where(v == R.NO_LOAD, R.NO_LOAD, v + here).astype(np.int32)
                fr[a][name] = v
        frames.append(fr)
    return dict(W=W, H=H, seg=seg, n_it=n_it), frames


WHOLE = dict(W=64, H=48, seg=8, n_it=5)  # the whole-frame comparison's configuration


def whole_frames(tris, W, H, seg, n_it, path=None):
    """four frames driven by the shader host in both arithmetics (K1, K2, K3 x N from the reference text, each frame's
    history its own previous output; K0 and the role rotation from the oracle's host mirror) next to OracleApp's.
    -> list of dict(fo, r32, r64) with r* = RefApp.draw()'s result"""
    out = []
    apps = None
    for f in oracle_frames(W, H, tris, seg, n_it):
        if apps is None:
            apps = {a: R.RefApp(a, None, path) for a in ("f32", "f64")}
        row = dict(f=f)
        for a in ("f32", "f64"):
            apps[a].tris = f.tris
            row[a] = apps[a].draw(f.fo, f.pc, f.ubo, seg, n_it)
        out.append(row)
    return out


def whole_errors(rows):
    """{pair: largest colour_err of the final image over the frames}; needs (and checks) that no path diverged"""
    err = {}
    for row in rows:
        f = row["f"]
        img = {"oracle": f.fo.image, "r32": row["f32"]["image"], "r64": row["f64"]["image"]}
        for a in ("f32", "f64"):
            tr = row[a]["traced"]
            assert same_paths(tr["seq_id"], tr["seq_n"], f.seq_id, f.seq_n).all(), "a path diverged: choose another configuration"
        for a, b in PAIRS:
            err[f"{a}/{b}"] = max(err.get(f"{a}/{b}", 0.0), colour_err(img[a], img[b]))
    return err
