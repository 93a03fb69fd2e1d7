"""The a-trous filter on STRIP contexts with injected adversarial planes: tests/test_filter_planes_gpu.py runs every route and
value class on whole frames (row_begin = 0, every launch over [0, H), the history the context's own full plane); the strip
tests of test_parity_gpu.py / test_strips.py run every row mode on rendered Cornell frames, one GPU run against another.
Here a context stores rows [stored) of a frame of tests/filter_planes.py's planes, filters plan.filter_rows(k) per
iteration (rows that shrink, row_base != 0, y0 != row_base) and its owned rows are compared with the rows [own) of the
WHOLE-FRAME oracle, whose previous-frame planes are restated to say what a band of valid rows says
(tests/strip_planes.py; its claims are checked in tests/test_strip_planes_cpu.py).  No tolerance anywhere:

  EXACT (0x1)    bit for bit the oracle's rows: image, PLANE_PREV_PIXEL after an odd final pass, moments and filtered variance
                 under 0x100; NaNs as positions.
  fast           bit for bit the fast direct kernel's whole-frame run on the same planes.

Harness (Strip, a sibling of test_filter_planes_gpu.gpu_run — the external bands, the second frame and the per-iteration
exchange do not fit one function with a plan argument): cfg.row_begin, row_end = plan.stored; upload; rtpt_gbuffer over the
stored rows (the tables); rtpt_set_plane every plane with rows [stored) of the whole-frame planes; rtpt_temporal_filter(k)
over plan.filter_rows(k).  External history / guide buffers are whole-frame torch allocations, NaN outside the band (the ids:
the frame's own previous ids, which match where the band says nothing may), passed as data_ptr() + row_begin * W * bytes: a
row misread by one, or a band read a row too wide, stays inside the allocation and shows.

A frame that follows rtpt_end_frame WITHOUT rtpt_raytrace (planes injected) is read through a second rtpt_end_frame and
PLANE_PREVIOUS: until the next rtpt_raytrace rtpt_readback(IMAGE) serves PREVIOUS (FrameState::image_alias).

Measured on an MI355X: the 36 tests of this file take 5.4 s together (about 1300 contexts of at most 130 x 97; the slowest
test 0.7 s, 2 s of set-up once for the oracle and the library)."""
import numpy as np
import pytest

import filter_planes as FP
import strip_planes as SP
import test_filter_planes_gpu as TF
from filter_planes import same_bits
from real_time_path_tracing_with_spatiotemporal_filtering_amd.strips import StripPlan

pytestmark = pytest.mark.gpu

X, DIRECT, NOFUSE = TF.X, TF.DIRECT, TF.NOFUSE
CHAIN_ENV = TF.CHAIN_ENV
CHAIN3 = dict(CHAIN_ENV, RTPT_CHAIN_MAX="3", RTPT_CHAIN_FINAL="1")


# ------------------------------------------------------------------------------------------ the harness
class Strip:
    """one context that stores plan.stored of p's frame"""

    def __init__(self, abi, p, plan, flags, *, inject_ids=True, timing=False):
        self.abi, self.plan, self.flags, self.inject_ids = abi, plan, flags, inject_ids
        self.W, self.H, self.nt = p["W"], p["H"], p["nt"]
        cfg = abi.config_default(self.W, self.H)
        cfg.flags = flags
        cfg.row_begin, cfg.row_end = plan.stored
        self.ctx = abi.Context(cfg)
        self.keep = []                      # external device buffers: alive as long as the context
        self.second_frame = False
        try:
            self.ctx.enable_debug(abi.DEBUG_PREV_PIXEL)
            self.ubo = TF._ubo(abi.Ubo, self.W, self.H, p)
            self.ctx.scene_upload(*FP.mesh_of(p["tris"]))
            self.ctx.gbuffer(self.ubo, *plan.stored)
            if timing:
                self.ctx.timing_enable(1)
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()
        self.keep.clear()

    def rows(self, arr):
        s0, s1 = self.plan.stored
        return np.ascontiguousarray(arr[s0:s1])

    def inject(self, p, previous=True):
        """previous=False: a frame after a real rtpt_end_frame — PREVIOUS, PREV_VIS_ID and MOMENTS_PREV are the context's own"""
        abi = self.abi
        todo = [(abi.PLANE_IMAGE, p["img"]), (abi.PLANE_DEPTH, p["depth"]), (abi.PLANE_WORLDPOS, p["worldpos"]),
                (abi.PLANE_GRADIENT, p["gradient"])]
        if self.inject_ids:
            todo.append((abi.PLANE_VIS_ID, FP.check_ids(p["ids"], self.nt)))
        if previous:
            todo += [(abi.PLANE_PREVIOUS, p["history"]), (abi.PLANE_PREV_VIS_ID, FP.check_ids(p["prev_vis"], self.nt))]
            if self.flags & 0x100:
                todo.append((abi.PLANE_MOMENTS_PREV, p["moments_prev"]))
        for which, arr in todo:
            self.ctx.set_plane(which, self.rows(arr))
        self.ctx.set_plane(abi.PLANE_LUT_PREV, p["lut_prev"])

    def _device(self, arr, rows, fill):
        """a whole-frame device buffer of arr with `fill` outside rows; returns the address of row rows[0]"""
        import torch
        a = np.array(arr)
        a[SP._outside(self.H, rows)] = fill
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        torch.cuda.synchronize()
        self.keep.append(t)
        return t.data_ptr() + rows[0] * (a.nbytes // self.H)

    def external_history(self, p, rows):
        self.ctx.set_external_history(self._device(p["history"], rows, np.nan), *rows)

    def external_guides(self, p, rows, moments=True):
        """the id buffer keeps the frame's previous ids OUTSIDE the band too (what a gather buffer holds from an earlier frame):
        a sentinel there would never match and hide a band read one row too wide; the moments outside are NaN"""
        ids = self._device(np.asarray(p["prev_vis"]).view(np.int32), (0, self.H), -1)
        ids += rows[0] * self.W * 4
        mom = self._device(p["moments_prev"], rows, np.nan) if moments else None
        self.ctx.set_external_guides(ids, mom, *rows)

    def filter(self, N, frame, first=1, last=None, rows_of=None):
        pc = self.abi.PushConstants()
        pc.frameNumber, pc.maxWaveletIteration = frame, N
        for k in range(first, (last or N) + 1):
            pc.waveletIteration = k
            self.ctx.temporal_filter(pc, self.ubo, *(rows_of or self.plan.filter_rows)(k))

    def end_frame(self):
        self.ctx.end_frame()
        self.second_frame = True

    def read(self, N):
        """the owned rows.  In a frame that followed rtpt_end_frame without rtpt_raytrace this ENDS the frame (module docstring)"""
        abi, (s0, _), (o0, o1) = self.abi, self.plan.stored, self.plan.own
        own = slice(o0 - s0, o1 - s0)
        out = {"prev_pixel": self.ctx.readback(abi.PLANE_PREV_PIXEL)[own] if N & 1 else None}
        if self.flags & 0x100:
            out["moments"] = self.ctx.readback(abi.PLANE_MOMENTS)[own]
            out["variance"] = self.ctx.readback(abi.PLANE_VARIANCE)[own]
        if self.second_frame:
            self.ctx.end_frame()
            out["image"] = self.ctx.readback(abi.PLANE_PREVIOUS)[own]
        else:
            out["image"] = self.ctx.readback(abi.PLANE_IMAGE)[own]
        return out

    def launches(self):
        tm = {k: v[1] for k, v in self.ctx.timing_collect().items()}
        return tm["k_atrous_chain"] + tm["k_atrous_chain_final"], tm["k_atrous"] + tm["k_atrous_final"], tm


def own_rows(ref, plan):
    o0, o1 = plan.own
    return {k: (v[o0:o1] if isinstance(v, np.ndarray) else v) for k, v in ref.items() if k != "iters"}


def strip_run(abi, p, plan, flags, N, frame, *, hist=None, guides=None, guide_moments=True, inject_ids=True, timing=False):
    """one strip, one filtered frame; hist / guides: the rows of an external history / guide buffer (None: the context's own
    injected planes, valid over the stored rows)"""
    with Strip(abi, p, plan, flags, inject_ids=inject_ids, timing=timing) as s:
        out = {}
        if not inject_ids:
            out["vis"] = s.ctx.readback(abi.PLANE_VIS_ID)
        s.inject(p)
        if hist is not None:
            s.external_history(p, hist)
        if guides is not None:
            s.external_guides(p, guides, guide_moments)
        s.filter(N, frame)
        out.update(s.read(N))
        if timing:
            out["chained"], out["single"], out["timing"] = s.launches()
        return out


def _env(m, env):
    for k, v in env.items():
        m.setenv(k, v)


# ------------------------------------------------------------------------------------------ routes and rotations
# name -> (T, flags, environment read by rtpt_create, a chained launch is expected); the first three also run the extension cases
ROUTES = {
    "comb_pair": (40, NOFUSE, {}, False),                  # k_atrous_comb_sh (id-pair table in LDS); its extension instances
    "direct": (40, DIRECT, {}, False),                     # k_atrous; k_atrous_ext
    "T100": (100, NOFUSE, {}, False),                      # no pair table, injected ids: k_atrous; k_atrous_ext
    "chain_max2": (40, 0, dict(CHAIN_ENV, RTPT_CHAIN_MAX="2", RTPT_CHAIN_FINAL="0"), True),   # k_atrous_chain + comb final
    "chain_max3": (40, 0, CHAIN3, True),                   # k_atrous_chain, the final pass chained too
    "grid": ("grid", 0, {}, False),                        # the G-buffer's own ids over the stored rows: per-pixel normals staged
}


def rotation(route, ci, rank, n):
    """n (class, id kind, roll, finite ids, frame) per route, case and rank: n = 6 is every class; with fewer, every class meets
    every case and rank over three consecutive routes.  The all-identical-vertex triangle's ids (0 / 0, spreading by the summed reach: one pixel in 41 leaves
    no finite pixel after two iterations) stay in every third run, never with N >= 5 or the planted class"""
    ri = list(ROUTES).index(route)
    T = ROUTES[route][0]
    case = SP.CASES[ci]
    out = []
    for j in range(n):
        v = ri + ci + rank + j * (3 if n <= 2 else 1)
        cls = FP.CLASSES[v % len(FP.CLASSES)]
        if T == "grid":
            kind, roll = "gbuffer", 0
        elif T == 40:
            kind, roll = SP.kind_of(case, rank, v)
        else:
            kind, roll = ("random", "blocks")[v % 2], 0
        finite = cls == "planted" or case[3] >= 5 or v % 3 != 0
        out.append((cls, kind, roll, finite and T != "grid", (v + 1) % 2))
    return out


def _cases_of(route):
    return [ci for ci, case in enumerate(SP.CASES) if not case[5] or list(ROUTES).index(route) < 3]


def compare(got, ref, tag, N, ext):
    TF.compare_exact(got, ref, tag, N, ext)


# ------------------------------------------------------------------------------------------ 1, 2: redundant strips
@pytest.mark.parametrize("route", list(ROUTES))
def test_exact_strip_equals_the_oracle_rows(hip_lib, oracle, monkeypatch, route):
    """every case, every rank, every class (id kinds, finite ids and frame 0 / 1 rotate), history from the `stored` band.
    comb_pair: k_atrous_comb_sh / its extension instances, k_stamp_depth, k_moments + k_var_prefilter under 0x100 / 0x900;
    direct, T100: k_atrous / k_atrous_ext; chain_max2 / 3: k_atrous_chain (+ chained final); grid: the per-pixel-normal comb"""
    T, flags, env, chained = ROUTES[route]
    _env(monkeypatch, env)
    ran_chain = 0
    for ci in _cases_of(route):
        W, H, world, N, _, ext, _ = SP.CASES[ci]
        for rank in range(world):
            plan = SP.plan_of(SP.CASES[ci], rank)
            for (cls, kind, roll, finite, frame) in rotation(route, ci, rank, 6):
                p = TF.planes(oracle, T, W, H, kind, cls, finite=finite, roll=roll)
                ref = TF.oracle_run(oracle, SP.restate_prev(p, plan.stored), ext, N, frame)
                got = strip_run(hip_lib, p, plan, flags | ext | X, N, frame, inject_ids=T != "grid", timing=True)
                tag = (route, ci, rank, cls, kind, frame)
                if T == "grid":
                    s0, s1 = plan.stored
                    assert np.array_equal(got["vis"], p["ids"][s0:s1]) and len(np.unique(got["vis"])) > 5, tag
                compare(got, own_rows(ref, plan), tag, N, ext)
                assert got["chained"] + got["single"] >= 1
                if not chained or ext:
                    assert got["chained"] == 0, (tag, got["timing"])
                else:
                    assert got["chained"] >= 1, (tag, got["timing"])
                ran_chain += got["chained"]
    assert bool(ran_chain) == chained


@pytest.mark.parametrize("route", list(ROUTES))
def test_fast_strip_equals_the_fast_direct_whole_frame(hip_lib, oracle, monkeypatch, route):
    """the same routes without RTPT_FLAG_EXACT_FILTER, two classes per route, case and rank: bit for bit the fast direct kernel's
    whole-frame run (RTPT_FLAG_DIRECT_FILTER: k_atrous / k_atrous_ext over [0, H)) on the same planes, history restricted to
    the stored rows by zeroing the rest of the whole-frame history (ids: an id no pixel carries is not expressible in the
    context's own plane, so the guide flags compare moments and disocclusion on whole-frame guides: band `whole`)"""
    T, flags, env, chained = ROUTES[route]
    for ci in _cases_of(route):
        W, H, world, N, _, ext, _ = SP.CASES[ci]
        for rank in range(world):
            plan = SP.plan_of(SP.CASES[ci], rank)
            for (cls, kind, roll, finite, frame) in rotation(route, ci, rank, 2):
                p = TF.planes(oracle, T, W, H, kind, cls, finite=finite, roll=roll)
                guided = bool(ext & 0x180)
                q = dict(SP.restate_prev(p, plan.stored), prev_vis=p["prev_vis"])      # history of the band, ids of the frame
                want = TF.gpu_run(hip_lib, q, ext | DIRECT, N, frame, inject_ids=T != "grid")
                with monkeypatch.context() as m:
                    _env(m, env)
                    got = strip_run(hip_lib, p, plan, flags | ext, N, frame, inject_ids=T != "grid", timing=True,
                                    guides=(0, H) if guided else None)
                TF.compare_runs(got, own_rows(want, plan), (route, ci, rank, cls, kind, frame), N, ext)
                assert (got["chained"] >= 1) == (chained and not ext), got["timing"]


# ------------------------------------------------------------------------------------------ 3: every history source
HIST_CASE = {0: 1, 0x80: 6, 0x100: 7, 0x9F0: 8}


@pytest.mark.parametrize("ext", list(HIST_CASE))
def test_every_history_source(hip_lib, oracle, monkeypatch, ext):
    """middle and last rank, frame 1, N = 3: PREVIOUS injected (`stored`) and external buffers over the frame (`whole`), a band
    whose ends cut through rows that pixels land in (`partial`) and one disjoint from the stored rows (`elsewhere`) — hist_row_base,
    hist_y0 / y1, pvis_row_base, pvis_y0 / y1 of k_atrous (plain direct), k_atrous_ext (extension direct), k_atrous_comb_sh,
    k_atrous_chain (plain, RTPT_CHAIN_FINAL=1) and k_moments (0x100, 0x9F0), against the oracle on restated planes.  Then
    different bands for history and guides, ids registered without moments, and rtpt_set_external_*(NULL)."""
    ci = HIST_CASE[ext]
    case = SP.CASES[ci]
    W, H, world, N = case[:4]
    routes = [("staged", X, {}), ("direct", X | DIRECT, {})] + ([("chain", X, CHAIN3)] if not ext else [])
    for rank in (1, 2):
        plan = SP.plan_of(case, rank)
        kind, roll = SP.landing_kind(ci, rank)
        p = TF.planes(oracle, SP.T_PAIR, W, H, kind, ("bounded", "wide")[rank % 2], finite=True, roll=roll)
        for how in ("stored", "whole", "partial", "elsewhere"):
            rows = SP.band(plan, how)
            counts = SP.landing_counts(p["landing"], plan, rows)
            assert all(counts[c] > 0 for c in SP.CLASSES if SP.possible(plan, rows, c)), (ci, rank, how, counts)
            ref = own_rows(TF.oracle_run(oracle, SP.restate_prev(p, rows), ext, N, 1), plan)
            ext_rows = None if how == "stored" else rows
            for name, flags, env in routes:
                with monkeypatch.context() as m:
                    _env(m, env)
                    got = strip_run(hip_lib, p, plan, flags | ext, N, 1, hist=ext_rows, guides=ext_rows if ext & 0x180 else None,
                                    timing=True)
                compare(got, ref, (hex(ext), rank, how, name), N, ext)
                assert (got["chained"] >= 1) == (name == "chain"), got["timing"]
        if ext == 0x9F0:      # history and guides on different bands
            hr, gr = SP.band(plan, "partial"), SP.band(plan, "whole")
            ref = own_rows(TF.oracle_run(oracle, SP.restate_prev(p, hr, gr), ext, N, 1), plan)
            compare(strip_run(hip_lib, p, plan, X | ext, N, 1, hist=hr, guides=gr), ref, (hex(ext), rank, "two bands"), N, ext)
            ref = own_rows(TF.oracle_run(oracle, SP.restate_prev(p, gr, hr), ext, N, 1), plan)
            compare(strip_run(hip_lib, p, plan, X | DIRECT | ext, N, 1, hist=gr, guides=hr), ref, (hex(ext), rank, "two bands'"), N, ext)
        if ext == 0x100:
            # 0x180, ids registered without moments: the disocclusion test of the final pass reads the registered ids, the
            # moment accumulation (prev_guides(with_moments = true)) falls back to the context's own planes (the stored rows);
            # then NULL, NULL and NULL: the next frame reads the context's own planes again
            f, st, gr = 0x180, plan.stored, SP.band(plan, "partial")
            ref = own_rows(TF.oracle_run(oracle, SP.restate_prev(p, st, gr, st), f, N, 1), plan)
            ref_stored = own_rows(TF.oracle_run(oracle, SP.restate_prev(p, st), f, N, 1), plan)
            assert not np.array_equal(ref["image"], ref_stored["image"])
            for flags in (X | f, X | DIRECT | f):
                with Strip(hip_lib, p, plan, flags) as s:
                    s.inject(p)
                    s.external_guides(p, gr, moments=False)
                    s.external_history(p, st)
                    s.filter(N, 1)
                    compare(s.read(N), ref, (hex(flags), rank, "ids without moments"), N, f)
                    s.ctx.set_external_guides(None, None)
                    s.ctx.set_external_history(None)
                    s.end_frame()
                    s.inject(p)
                    s.filter(N, 1)
                    compare(s.read(N), ref_stored, (hex(flags), rank, "after NULL"), N, f)


# ------------------------------------------------------------------------------------------ 4, 7: the `own` band
def _second_frame(oracle, s, p, p1, ref0, ext, N, tag):
    """after a real rtpt_end_frame: PREVIOUS holds the finished frame on the rows the final pass wrote (`own`; its halo rows are
    stale and asserted to be), the previous ids / moments the stored rows (fr.guides).  Frame 1 injects p1's planes but no
    previous-frame plane; the reference is the oracle's frame 1 on the oracle's frame 0, restated to those bands."""
    plan, abi = s.plan, s.abi
    (s0, s1), (o0, o1) = plan.stored, plan.own
    s.end_frame()
    prev = s.ctx.readback(abi.PLANE_PREVIOUS)
    same_bits(prev[o0 - s0:o1 - s0], ref0["image"][o0:o1], tag + ("frame 0",))
    # the halo rows of PREVIOUS hold an earlier iteration's output or nothing.  (Not every pixel differs from the finished
    # frame: between random ids most normal weights are 0 and a pixel keeps its colour through every iteration.)  What counts:
    # pixels of frame 1 land on stale ones
    a, b = prev[..., :3], ref0["image"][s0:s1][..., :3]
    stale = ((a != b) & ~(np.isnan(a) & np.isnan(b))).any(-1)
    assert not stale[o0 - s0:o1 - s0].any()
    hit = SP.landing_masks(p1["landing"], plan, plan.own)["stored_not_valid"]
    py, px = p1["landing"][o0:o1][hit][:, 1], p1["landing"][o0:o1][hit][:, 0]
    assert stale[py - s0, px].sum() >= 1, (tag, "no pixel lands on a stale halo pixel: the band would not matter", int(stale.sum()))
    base = dict(p1, key=p1["key"] + ("after", p["key"], ext, N, tag), history=ref0["image"], prev_vis=np.array(p["ids"]))
    if ext & 0x100:
        base["moments_prev"] = ref0["moments"]
    ref1 = TF.oracle_run(oracle, SP.restate_prev(base, plan.own, plan.stored), ext, N, 1)
    as_stored = TF.oracle_run(oracle, SP.restate_prev(base, plan.stored), ext, N, 1)
    assert not np.array_equal(ref1["image"][o0:o1], as_stored["image"][o0:o1]), (tag, "the band matters")
    s.inject(p1, previous=False)
    s.filter(N, 1)
    compare(s.read(N), own_rows(ref1, plan), tag + ("frame 1",), N, ext)


def _frame_before(p):
    """the planes of the frame BEFORE p's: its ids are p's previous ids (filter_planes.prev_ids: the id of every second pixel
    that lands inside the frame), so that after rtpt_end_frame the disocclusion test and the moment history find matches"""
    return dict(p, key=p["key"] + ("the frame before",), ids=np.array(p["prev_vis"]))


OWN_ROUTES = {"comb": (NOFUSE, {}, 0), "chain_final": (0, CHAIN3, 0), "default": (0, {}, 0), "ext_0x180": (0, {}, 0x180),
              "ext_0x180_direct": (DIRECT, {}, 0x180)}


@pytest.mark.parametrize("route", list(OWN_ROUTES))
def test_own_band_after_a_real_hand_over(hip_lib, oracle, monkeypatch, route):
    """two frames on one context, redundant mode, every rank: frame 0 from injected planes, rtpt_end_frame (fr.hist = fr.final =
    the owned rows, fr.guides = the stored rows), frame 1 through the unchained (comb: k_atrous_comb_sh) and the chained
    (k_atrous_chain, RTPT_CHAIN_FINAL=1) final pass, the extension kernels under 0x180 (k_moments reads the context's own
    previous moments)"""
    flags, env, ext = OWN_ROUTES[route]
    _env(monkeypatch, env)
    for ci in ((6,) if ext else (1, 3)):
        case = SP.CASES[ci]
        W, H, world, N = case[:4]
        for rank in range(world):
            plan = SP.plan_of(case, rank)
            kind, roll = SP.landing_kind(ci, rank)
            p1 = TF.planes(oracle, SP.T_PAIR, W, H, kind, ("subnormal", "planted", "wide")[rank], finite=True, roll=roll)
            p = _frame_before(TF.planes(oracle, SP.T_PAIR, W, H, kind, "bounded", finite=True, roll=roll))
            ref0 = TF.oracle_run(oracle, p, ext, N, 0)
            with Strip(hip_lib, p, plan, flags | ext | X, timing=True) as s:
                s.inject(p)
                s.filter(N, 0)
                _second_frame(oracle, s, p, p1, ref0, ext, N, (route, ci, rank))
                chained, single, tm = s.launches()
                assert (chained >= 2) == (route == "chain_final"), tm


@pytest.mark.parametrize("flags", [NOFUSE, 0, DIRECT])
def test_two_row_ranges_of_one_final_pass(hip_lib, oracle, flags):
    """the owned rows as [o0, m) then [m, o1) (FilterPlan::second_range, fr.final.extend), rtpt_end_frame: the next frame's
    `own` band covers both ranges.  k_atrous_comb_sh / k_atrous final pass over a part of the strip"""
    for ci in (1, 3):
        case = SP.CASES[ci]
        W, H, world, N = case[:4]
        for rank in range(world):
            plan = SP.plan_of(case, rank)
            o0, o1 = plan.own
            m = o0 + (o1 - o0) // 3 + 1
            kind, roll = SP.landing_kind(ci, rank)
            p = _frame_before(TF.planes(oracle, SP.T_PAIR, W, H, kind, "bounded", finite=True, roll=roll))
            p1 = TF.planes(oracle, SP.T_PAIR, W, H, kind, ("bounded", "wide")[ci % 2], finite=True, roll=roll)
            ref0 = TF.oracle_run(oracle, SP.restate_prev(p, plan.stored), 0, N, 1)
            with Strip(hip_lib, p, plan, flags | X) as s:
                s.inject(p)
                s.filter(N, 1, last=N - 1)
                s.filter(N, 1, first=N, rows_of=lambda k: (o0, m))
                s.filter(N, 1, first=N, rows_of=lambda k: (m, o1))
                compare(s.read(N), own_rows(ref0, plan), ("two ranges", hex(flags), ci, rank), N, 0)
                _second_frame(oracle, s, p, p1, ref0, 0, N, ("two ranges", hex(flags), ci, rank))


# ------------------------------------------------------------------------------------------ 5: exchange mode
def _whole_frame_iterations(abi, p, flags, N, frame):
    """[(image, variance)] after every iteration of a whole-frame run with separate launches (what the neighbours would send)"""
    plan = StripPlan(p["H"], 1, 0, N, "exchange", flags & 0x9F0)
    out = []
    with Strip(abi, p, plan, flags | NOFUSE) as s:
        s.inject(p)
        for k in range(1, N + 1):
            s.filter(N, frame, first=k, last=k)
            img = s.ctx.readback(abi.PLANE_FILTERED if (k & 1 and k < N) else abi.PLANE_IMAGE)
            out.append((img, s.ctx.readback(abi.PLANE_VARIANCE) if flags & 0x100 else None))
        final = s.read(N)
    return out, final


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("ci", [1, 3, 4, 5, 7])
def test_exchange_mode_one_rank_at_a_time(hip_lib, oracle, ci, exact):
    """exchange-mode plans (halo = the longest reach, every iteration over the owned rows): before iteration k the receive rows
    of plan.exchange_rows(k) are overwritten with the whole frame's output of iteration k - 1 — the oracle's under EXACT, a
    whole-frame separate-launch GPU run's without — and under 0x100 the filtered variance with them.  Staged
    (k_atrous_comb_sh and its extension instances, k_stamp_depth after every rtpt_set_plane) and direct (k_atrous /
    k_atrous_ext) on every rank; classes rotate, planted and overflow among them"""
    abi = hip_lib
    case = SP.CASES[ci]
    W, H, world, N, _, ext, _ = case
    for rank in range(world):
        plan = SP.plan_of(case, rank, "exchange")
        s0 = plan.stored[0]
        for j, flags in enumerate((NOFUSE, DIRECT)):
            cls = ("planted", "overflow", "bounded", "wide", "subnormal", "flat")[(ci + rank + 3 * j) % 6]
            frame = (rank + j) % 2
            kind, roll = SP.kind_of(case, rank, ci + rank + j)
            p = TF.planes(oracle, SP.T_PAIR, W, H, kind, cls, finite=True, roll=roll)
            q = SP.restate_prev(p, plan.stored)
            if exact:
                ref = TF.oracle_run(oracle, q, ext, N, frame)
                iters, final = ref["iters"], own_rows(ref, plan)
            else:
                qq = dict(q, prev_vis=p["prev_vis"])
                iters, final = _whole_frame_iterations(abi, qq, ext, N, frame)
                o0, o1 = plan.own
                final = {k: (v[o0:o1] if v is not None else None) for k, v in final.items()}
            with Strip(abi, p, plan, flags | ext | exact) as s:
                s.inject(p)
                if not exact and ext & 0x180:
                    s.external_guides(p, (0, H))
                for k in range(1, N + 1):
                    todo = plan.exchange_rows(k)
                    if k > 1 and todo:
                        which = abi.PLANE_FILTERED if (k - 1) & 1 else abi.PLANE_IMAGE
                        planes = [(which, iters[k - 2][0])] + ([(abi.PLANE_VARIANCE, iters[k - 2][1])] if ext & 0x100 else [])
                        for plane, src in planes:
                            buf = s.ctx.readback(plane)
                            for _, _, (a, b) in todo:
                                buf[a - s0:b - s0] = src[a:b]
                            s.ctx.set_plane(plane, buf)
                    s.filter(N, frame, first=k, last=k)
                got = s.read(N)
            (TF.compare_exact if exact else TF.compare_runs)(got, final, ("exchange", ci, rank, hex(flags), cls, exact), N, ext)


# ------------------------------------------------------------------------------------------ 6: present
@pytest.mark.parametrize("N", [1, 3])
def test_present_on_a_strip(hip_lib, oracle, N):
    """rtpt_present_target / rtpt_present of the owned rows into a buffer of exactly that many rows (its first byte is pixel
    (0, own[0])): the fused store of the id-pair final pass (k_atrous_comb_sh) and k_present give oracle.present_bgra8 of the
    oracle's rows [own), frame 0 and frame 1 with the `stored` band; once more over a sub-range of the owned rows"""
    import torch
    abi = hip_lib
    W, H, T = 130, 97, 40
    p = TF._present_planes(oracle, T, W, H, finite=True)
    if N > 1:
        # a colour of +-Inf turns its 3 x 3 neighbourhood NaN (weight 0 x Inf) and three iterations the whole frame: keep the
        # colours outside [0, 1], the huge one and the single NaN, make the infinite ones finite
        img = np.array(p["img"])
        img[np.isposinf(img)], img[np.isneginf(img)] = np.float32(7.5), np.float32(-7.5)
        p = dict(p, key=p["key"] + ("finite colours",), img=img)
    for rank in range(3):
        plan = StripPlan(H, 3, rank, N, "redundant")
        o0, o1 = plan.own
        a, b = o0 + 3, o1 - 5
        for frame in (0, 1):
            ref = own_rows(TF.oracle_run(oracle, SP.restate_prev(p, plan.stored), 0, N, frame), plan)
            want = oracle.present_bgra8(ref["image"])
            with Strip(abi, p, plan, X, timing=True) as s:
                s.inject(p)
                img8 = [torch.zeros((o1 - o0, W, 4), dtype=torch.uint8, device="cuda") for _ in range(2)]
                part = torch.zeros((b - a, W, 4), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                s.ctx.present_target(img8[0].data_ptr(), o0, o1)
                s.filter(N, frame)
                got = s.read(N)
                s.ctx.present(img8[0].data_ptr(), o0, o1)       # returns at once: the final pass wrote the rows
                s.ctx.present_target(None)
                s.ctx.present(img8[1].data_ptr(), o0, o1)       # k_present
                s.ctx.present(part.data_ptr(), a, b)
                s.ctx.sync()
                tm = s.launches()[2]
            same_bits(got["image"], ref["image"], ("present", N, rank, frame))
            for which, t in zip(("fused", "k_present"), img8):
                g = t.cpu().numpy()
                assert g.tobytes() == want.tobytes(), (N, rank, frame, which, np.argwhere(g != want)[:4].tolist())
            g = part.cpu().numpy()
            assert g.tobytes() == want[a - o0:b - o0].tobytes(), (N, rank, frame, "sub-range", np.argwhere(g != want[a - o0:b - o0])[:4].tolist())
            assert tm["k_present"] == 2, tm
            assert len(np.unique(want)) > 100 and np.isfinite(ref["image"]).mean() > 0.3
