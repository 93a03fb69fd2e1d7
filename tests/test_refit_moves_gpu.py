"""Closest hit after a REFIT: hostile instance moves (refit_moves.py) on every refit route, against the oracle's brute
force over the moved triangles — ids equal, t bit for bit, no tolerance anywhere.

test_traversal_gpu.py holds a tree that was just built for its geometry to D4; here the tree keeps the topology of the
upload's pose while rtpt_scene_set_instances and a changed ubo.model (repose_scene, api_scene.hip) stack the instances onto
one another, swap them, fling one 1e5 away, collapse them onto a plane and a point, mirror them and scale them by 1e-3 and
1e3: k_pose / k_refit_level / k_refit_grid / k_refit_quantise (refit.hip), the host's refit_bvh + pack_quantised_nodes
(RTPT_HOST_REFIT=1), the device flatten and the pair records of launch_scene_prepare, the brute-force kernel's `paired`
flag.  After every move the tree on the device must also pass rtpt_debug_bvh_check.

Each test is one upload and a sequence of moves on the same context; the references are traced once per session
(refit_moves.reference) and proven to hit enough by test_refit_moves_cpu.py."""
import numpy as np
import pytest

import refit_moves as R
import test_traversal_gpu as T
from conftest import bits
from test_instances_gpu import CLEAN, D_FLAT, D_LBVH, D_SAH, _ubo

pytestmark = pytest.mark.gpu

# name: (flags, RTPT_HOST_REFIT)
ROUTES = {"device_refit": (0, "0"), "host_refit": (0, "1"), "device_lbvh": (D_LBVH, "0"), "device_sah": (D_LBVH | D_SAH, "0"),
          "device_flatten": (D_LBVH | D_SAH | D_FLAT, "0")}


class _Scene:
    """one context with the mesh uploaded under x0(); every step checks the tree and compares a trace with its reference"""

    def __init__(self, hip_lib, oracle, monkeypatch, mesh, flags=0, host_refit="0", env=None):
        monkeypatch.setenv("RTPT_HOST_REFIT", host_refit)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        self.lib, self.oracle, self.mesh, self.flags = hip_lib, oracle, mesh, flags
        self.host_refit = host_refit == "1"
        self.tag = f"{mesh} flags={flags:#x} host_refit={host_refit} {env or ''}"
        self.moves, self.model = 0, "identity"
        cfg = hip_lib.config_default(64, 64)
        cfg.flags = flags
        cfg.ray_tmax = R.TMAX
        self.ctx = hip_lib.Context(cfg)
        xyz, idx = R.mesh(mesh)
        self.n_tris = len(idx) * R.N_INST
        self.ctx.scene_upload(xyz, idx, R.x0())
        self.ubo = _ubo(hip_lib, 64, 64)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()

    @property
    def device_moves(self):
        """where a move is applied: on the device for every BVH scene unless RTPT_HOST_REFIT=1 keeps a host tree on the host"""
        bvh = self.n_tris > 64 or bool(self.flags & self.lib.FLAG_FORCE_BVH)
        return bvh and (not self.host_refit or bool(self.flags & D_LBVH))

    def assert_route(self, no_pairs=False):
        info, up = self.ctx.scene_build_info(), self.ctx.debug_upload_info()
        want = {0: self.lib.BVH_BUILDER_HOST_SAH, D_LBVH: self.lib.BVH_BUILDER_DEVICE_LBVH}.get(self.flags & (D_LBVH | D_SAH), self.lib.BUILDER_DEVICE_SAH)
        assert info["builder"] == want and info["fallback"] == self.lib.BVH_FALLBACK_NONE, (self.tag, info)
        assert info["leaf_pairs"] == int(R.PAIRED[self.mesh] and not no_pairs), (self.tag, info)
        assert up["device_flatten"] == int(bool(self.flags & D_FLAT)) and up["moves_without_sync"] == 0, (self.tag, up)

    def move(self, name):
        self.ctx.scene_set_instances(R.move(name))
        self.moves += 1
        up = self.ctx.debug_upload_info()
        assert up["device_flatten"] == int(self.device_moves) and up["device_pairs"] == 0, (self.tag, name, up)
        assert up["moves_without_sync"] == (self.moves if self.device_moves else 0), (self.tag, name, up)

    def set_model(self, name):
        self.ubo.model[:] = R.model(name)
        self.ubo.modelPrev[:] = self.ubo.model[:]
        self.ctx.gbuffer(self.ubo)
        self.model = name

    def check(self, move):
        """the tree is clean and the trace is the oracle's for (mesh, move, the model in force); returns the GPU's (ids, t)"""
        case = R.reference(self.oracle, self.mesh, move, self.model)
        st = self.ctx.debug_bvh_check()
        assert all(st[k] == 0 for k in CLEAN), (self.tag, move, self.model, st)
        ids, ts = self.ctx.selftest_trace(case.rays)
        msg = T._first_mismatch(f"{self.tag} after {move} under {self.model}", case.rays, ids, ts, case.wid, case.wts)
        assert msg is None, msg
        return ids, ts


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


# ------------------------------------------------------------------------------ 1. every move on every refit route
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("mesh", R.LARGE)
def test_every_move_on_every_route(hip_lib, oracle, monkeypatch, mesh, route):
    flags, host_refit = ROUTES[route]
    with _Scene(hip_lib, oracle, monkeypatch, mesh, flags, host_refit) as s:
        s.assert_route()
        first = s.check("home")
        for name in R.MOVES:
            s.move(name)
            got = s.check(name)
        assert name == "home" and _same_bits(got, first), f"{s.tag}: a refit left a residue"


# ------------------------------------------------------------------------------ 2. traversal forms after a move
FORMS = {name: (flags, env) for name, flags, env in T._forms(1000, True) if env}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("mesh", ["heightfield", "soup"])
def test_traversal_forms_after_a_move(hip_lib, oracle, monkeypatch, mesh, form):
    """leaves over single triangles where the scene is all fan pairs, and a traversal stack that spills"""
    flags, env = FORMS[form]
    assert set(FORMS) == {"no_pairs", "stack_lds_1"}
    with _Scene(hip_lib, oracle, monkeypatch, mesh, flags, env=env) as s:
        s.assert_route(no_pairs=form == "no_pairs")
        s.check("home")
        for name in ("stack", "fling"):
            s.move(name)
            s.check(name)


# ------------------------------------------------------------------------------ 3. three moves back to back
@pytest.mark.parametrize("route", ["device_refit", "device_flatten"])
@pytest.mark.parametrize("mesh", ["heightfield", "soup"])
def test_three_moves_back_to_back(hip_lib, oracle, monkeypatch, mesh, route):
    """nothing between the calls: both pinned staging buffers of stage_transforms are in use and the third call waits for
    the first one's event; the scene that is traced is the last one's"""
    flags, host_refit = ROUTES[route]
    with _Scene(hip_lib, oracle, monkeypatch, mesh, flags, host_refit) as s:
        for name in ("stack", "fling", "mirror"):
            s.ctx.scene_set_instances(R.move(name))
        s.moves = 3
        assert s.ctx.debug_upload_info()["moves_without_sync"] == 3
        s.check("mirror")
        for name in ("collapse", "home"):   # and two more: the staging buffers come round again
            s.ctx.scene_set_instances(R.move(name))
        s.check("home")


# ------------------------------------------------------------------------------ 4. model and instances in both orders
@pytest.mark.parametrize("route", ["device_refit", "host_refit"])
@pytest.mark.parametrize("mesh", ["heightfield", "soup"])
def test_model_and_instances_in_both_orders(hip_lib, oracle, monkeypatch, mesh, route):
    """ubo.model (through rtpt_gbuffer) and the instances both end in repose_scene; the posed scene is the LUT's whichever
    came last"""
    flags, host_refit = ROUTES[route]
    with _Scene(hip_lib, oracle, monkeypatch, mesh, flags, host_refit) as s:
        first = s.check("home")
        s.set_model("general")
        s.check("home")
        s.move("fling")               # order A: the model is set, then the instances move
        s.check("fling")
        s.set_model("identity")
        s.check("fling")
        s.move("collapse")            # order B: the instances move, then the model is set
        s.set_model("general")
        s.check("collapse")
        s.set_model("identity")
        s.check("collapse")
        s.move("home")
        assert _same_bits(s.check("home"), first), f"{s.tag}: a refit left a residue"


# ------------------------------------------------------------------------------ 5. rebuild after a move
@pytest.mark.parametrize("route", ["device_lbvh", "device_sah"])
@pytest.mark.parametrize("mesh", ["heightfield", "soup"])
def test_rebuild_after_a_hostile_move(hip_lib, oracle, monkeypatch, mesh, route):
    """rtpt_scene_rebuild builds the tree for the pose it holds: the hits keep their bits; the new tree is then refit in turn"""
    flags, host_refit = ROUTES[route]
    with _Scene(hip_lib, oracle, monkeypatch, mesh, flags, host_refit) as s:
        s.assert_route()
        first = s.check("home")
        for name in ("swap", "fling"):
            s.move(name)
            before = s.check(name)
            s.ctx.scene_rebuild()
            info = s.ctx.scene_build_info()
            assert info["n_primitives"] == (s.n_tris // 2 if R.PAIRED[mesh] else s.n_tris), (s.tag, name, info)
            assert _same_bits(s.check(name), before), (s.tag, name)
        s.move("home")                # a tree built for the flung pose, refit to the upload's
        assert _same_bits(s.check("home"), first), f"{s.tag}: a refit left a residue"


# ------------------------------------------------------------------------------ 6. small scenes
@pytest.mark.parametrize("flags", [0, 2])   # brute force, re-flattened and re-posed on the host / the BVH, refit on the device
@pytest.mark.parametrize("mesh", R.SMALL)
def test_small_scenes(hip_lib, oracle, monkeypatch, mesh, flags):
    """at most 64 triangles: every move recomputes the brute-force kernel's `paired` flag (small_soup: false, true under
    all_points, false again)"""
    assert flags in (0, hip_lib.FLAG_FORCE_BVH)
    with _Scene(hip_lib, oracle, monkeypatch, mesh, flags) as s:
        assert s.n_tris <= 64 and s.ctx.scene_build_info()["builder"] == hip_lib.BVH_BUILDER_HOST_SAH
        first = s.check("home")
        for name in R.SMALL_MOVES:
            s.move(name)
            got = s.check(name)
            if name == "all_points":
                assert not got[0].any(), f"{s.tag}: a point was hit"
        assert _same_bits(got, first), f"{s.tag}: a refit left a residue"
