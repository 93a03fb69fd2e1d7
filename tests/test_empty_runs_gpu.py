"""The tile columns no triangle reaches (csrc/final_split.hpp, include/rtpt.h: rtpt_debug_empty_run_info): in the tracing
launch that carries the deferred final pass, the columns at the end of the tiles' dispatch order that no triangle's screen
bounds reach are served R vertically consecutive tiles per workgroup, by a body that traces the primary segment only
(csrc/pathtrace_tile.hpp: pathtrace_empty_run).  RTPT_EMPTY_RUN=<R> sets R, 0 turns the runs off.

Every case renders frames at rest (N = 5, 4 segments; eight of them unless it says otherwise) and asks for the bits of two
references in every readable plane, the ray count and the reuse / reprojection counters: a context without runs
(RTPT_EMPTY_RUN=0) and a context that never defers (RTPT_NO_FINAL_DEFER=1, whose tracing launches are the plain tile kernel's).
A run changes which workgroup and which lane trace a pixel, never what is computed for it, so no bit may move.  The counter says
after every frame what the last tracing launch was made of: the cases built to have runs must have them, the others must not.
The references of a configuration are rendered once and shared by its values of R."""
import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

SEG, N = 4, 5
REST8 = [()] * 8
IN_TRACE8 = 4   # of the five final passes that eight frames at rest record, four run inside the next frame's trace

INSIDE_BOX = (-0.001, 1.0, 0.5)   # the camera between the walls: they pass behind it, every triangle's bounds are the whole frame
SIDEWAYS = (-2.2, 1.0, 6.0)       # the box right of the middle, into the last pixel column of 257: only column 0 is left over
FAR_AWAY = (30.0, 1.0, 6.0)       # the box far outside the frame: every column is empty
R_VALUES = [1, 2, 3, 16, 100]     # 100: above tiles_y of every size here


def _cols(w):
    return (w + 63) // 64


def _rows(h):
    return (h + 3) // 4


def _order(tx):
    return [(tx - 1) // 2 + (c + 1) // 2 if c & 1 else (tx - 1) // 2 - c // 2 for c in range(tx)]


# size; kw: make_app keywords; script: the keys held frame by frame (eight frames at rest without one); full: the columns a launch
# with runs serves as tiles ("some": not pinned; None: no launch has runs); count: a count-rows window; debug: a debug mask by name
CONFIGS = {
    # five columns, dispatch order 2 3 1 4 0: the box reaches 1 and 2, so column 3 is empty inside the prefix, the suffix is
    # {4, 0} and column 4 is one pixel wide
    "257x83": dict(size=(257, 83), full=3),
    "200x37": dict(size=(200, 37), full="some"),
    "64x4_one_tile": dict(size=(64, 4), full=None),
    "1000x40_many_empty_columns": dict(size=(1000, 40), full=2),
    "257x83_sideways_one_sided_suffix": dict(size=(257, 83), kw=dict(cameraOrigin=SIDEWAYS), full=4),
    "257x83_every_column_empty": dict(size=(257, 83), kw=dict(cameraOrigin=FAR_AWAY), full=0),
    "200x37_every_column_empty": dict(size=(200, 37), kw=dict(cameraOrigin=FAR_AWAY), full=0),
    "257x83_camera_inside_the_box": dict(size=(257, 83), kw=dict(cameraOrigin=INSIDE_BOX), full=None),
    # the light's disc (radius 0.2) projects to about x = 22 +- 8, y = 41 +- 8: inside column 0, a suffix column
    "257x83_light_in_a_suffix_column": dict(size=(257, 83), kw=dict(lightPos=(-2.6, 1.0, 1.0)), full=3, lit=(slice(25, 58), slice(6, 38))),
    "257x83_hit_id_plane": dict(size=(257, 83), debug="DEBUG_HIT_ID", full=3),
    "257x83_count_rows_cut_a_run": dict(size=(257, 83), count=(10, 50), full=3),
    "200x120_strip_1_of_3": dict(size=(200, 120), kw=dict(rank=1, world=3, mode="redundant", torch_planes=False), full="some"),
    # rest x 3, one key held, rest x 5: the box's padded right edge moves from pixel column 575 past 576, so column 9 of 16 becomes
    # a reached one (order 7 8 6 9 ...: 2 full columns before, 4 after), and the deferral starts over after the moving frame.  A
    # launch carries a final pass from the fifth frame at rest on, so here only the last two launches do, with the new bounds ...
    "1000x40_moving": dict(size=(1000, 40), kw=dict(cameraOrigin=(-2.45, 1.0, 6.0)), script=[()] * 3 + [("A",)] + [()] * 5, full="changes",
                           before=set(), after={4}),
    # ... and with six frames at rest on either side launches with runs see both sets of bounds
    "1000x40_moving_between_runs": dict(size=(1000, 40), kw=dict(cameraOrigin=(-2.45, 1.0, 6.0)), script=[()] * 6 + [("A",)] + [()] * 6,
                                        full="changes", before={2}, after={4}),
}
CASES = [(c, r) for c in CONFIGS for r in (R_VALUES if "_" not in c or c.startswith(("64x4", "1000x40_many")) else [3, 16])]


def _planes(P, debug):
    p = [P.PLANE_IMAGE, P.PLANE_FILTERED, P.PLANE_PREVIOUS, P.PLANE_WORLDPOS, P.PLANE_GRADIENT, P.PLANE_DEPTH, P.PLANE_VIS_ID,
         P.PLANE_PREV_VIS_ID, P.PLANE_LUT, P.PLANE_LUT_PREV]
    return p + ([P.PLANE_HIT_ID] if debug else [])


def _run(P, monkeypatch, name, defer, run_len):
    """-> (planes and ray count after the last frame, traced image of the last frame or None, (defer, reuse, reprojection
    counters), the run counter after every frame)"""
    from real_time_path_tracing_with_spatiotemporal_filtering_amd.app import make_app
    cfg = CONFIGS[name]
    monkeypatch.setenv("RTPT_NO_FINAL_DEFER", "0" if defer else "1")
    monkeypatch.delenv("RTPT_FINAL_FRONT", raising=False)
    monkeypatch.setenv("RTPT_EMPTY_RUN", str(run_len))
    debug = getattr(P, cfg["debug"]) if cfg.get("debug") else 0
    app = make_app(cfg["size"][0], cfg["size"][1], iterations=N, max_segments=SEG, debug_mask=debug, **cfg.get("kw", {}))
    ctx = app.backend.ctx
    if cfg.get("count"):
        ctx.set_count_rows(*cfg["count"])
    runs, traced = [], None
    script = cfg.get("script", REST8)
    for f, keys in enumerate(script):
        app.updateScene(keys)
        app.drawVisbilityBuffer()
        app.computeTemporalGradient()
        app.drawSceneToImage()
        runs.append(ctx.empty_run_info())
        if cfg.get("lit") and f == len(script) - 1:
            traced = ctx.readback(P.PLANE_IMAGE)   # the traced image, before the filter's last iteration replaces it
        app.applyTemporalFiltering()
        app.copyImageToSwapChainsCurrentImage()
        app.frameCount += 1
    seen = [ctx.readback(p) for p in _planes(P, debug)] + [np.array([ctx.raycount()], np.uint64)]
    info = (ctx.defer_info(), ctx.reuse_info(), ctx.reproj_info())
    app.backend.close()
    return seen, traced, info, runs


_reference = {}


def _refs(P, monkeypatch, name):
    if name not in _reference:
        out = []
        for defer, run_len in ((True, 0), (False, 3)):
            seen, traced, info, runs = _run(P, monkeypatch, name, defer, run_len)
            for a in seen:
                a.setflags(write=False)
            assert all(r["run_workgroups"] == 0 and r["run_tiles"] == 0 for r in runs), "a reference context launched runs"
            out.append((seen, info))
        assert out[1][1][0] == dict(recorded=0, launched_in_trace=0, launched_alone=0, spare_bytes=0)
        _reference[name] = out
    return _reference[name]


@pytest.mark.parametrize("name,run_len", CASES, ids=[f"{c}-R{r}" for c, r in CASES])
def test_runs_change_no_bit(hip_lib, monkeypatch, name, run_len):
    cfg = CONFIGS[name]
    refs = _refs(hip_lib, monkeypatch, name)
    got, traced, info, runs = _run(hip_lib, monkeypatch, name, True, run_len)
    print(name, run_len, info[0], [(r["full_columns"], r["run_workgroups"], r["run_tiles"]) for r in runs])
    for which, (ref, ref_info) in zip(("RTPT_EMPTY_RUN=0", "RTPT_NO_FINAL_DEFER=1"), refs):
        assert len(got) == len(ref)
        for i, (x, y) in enumerate(zip(got, ref)):
            assert x.shape == y.shape and x.dtype == y.dtype, f"observation {i}"
            assert np.array_equal(bits(x) if x.dtype.itemsize == 4 else x, bits(y) if y.dtype.itemsize == 4 else y), \
                f"observation {i} differs from the context with {which}"
        assert info[1:] == ref_info[1:], f"reuse / reprojection counters differ from the context with {which}"
    assert info[0] == refs[0][1][0], "the runs changed what is deferred"
    d = info[0]
    assert d["recorded"] == d["launched_in_trace"] + d["launched_alone"]
    if "script" not in cfg:   # (a script's count is the count of the context without runs, asserted above)
        assert d["launched_in_trace"] == IN_TRACE8

    # what the launches were made of
    W, rows = cfg["size"][0], cfg["size"][1]
    if "world" in cfg.get("kw", {}):
        rows = None   # a strip traces its own rows and a halo
    tx = _cols(W)
    assert all(r["run_len"] == run_len for r in runs)
    with_runs = [r for r in runs if r["run_workgroups"]]
    for r in runs:
        if not r["run_workgroups"]:
            assert r["full_columns"] == tx and r["run_tiles"] == 0
        else:
            assert r["full_columns"] < tx
            if rows is not None:
                ty = _rows(rows)
                assert r["run_tiles"] == (tx - r["full_columns"]) * ty
                assert r["run_workgroups"] == (tx - r["full_columns"]) * -(-ty // min(run_len, ty))
    full = cfg["full"]
    if full is None:
        assert not with_runs, "runs in a launch that has no empty suffix"
        return
    # a launch carries a final pass from the fifth frame at rest on (the reprojection is stored on the third, loaded and the
    # pass deferred on the fourth): every such launch of these cases has runs
    assert len(with_runs) == d["launched_in_trace"] >= 2, "the launches built to have runs have none"
    if full == "changes":
        key = cfg["script"].index(("A",))
        before = {r["full_columns"] for r in runs[:key] if r["run_workgroups"]}
        after = {r["full_columns"] for r in runs[key + 1:] if r["run_workgroups"]}
        assert before == cfg["before"] and after == cfg["after"], "the suffix did not change with the camera"
        assert runs[key]["run_workgroups"] == 0, "the moving frame's launch carries no final pass"
    elif full != "some":
        assert {r["full_columns"] for r in with_runs} == {full}
    if cfg.get("lit"):   # paths of a suffix column end on the light: 30 x 0.5 / 5 per channel at the first hit
        ys, xs = cfg["lit"]
        assert runs[-1]["run_workgroups"] and _order(tx)[runs[-1]["full_columns"]:].count(0) == 1, "column 0 is not served in runs"
        lit = np.ascontiguousarray(traced.reshape(cfg["size"][1], W, -1)[ys, xs, :3], np.float32)
        assert (lit.view(np.uint32) == np.float32(3.0).view(np.uint32)).all(axis=-1).any(), "no path of the suffix column ended on the light"
