#!/usr/bin/env python3
"""Record what the seven numpy path walkers of the tests returned before tests/path_walker.py replaced them.

    git worktree add ../parent <the commit before the one walker>
    python scripts/record_walker_frames.py ../parent

The checkout's tests/ and root go on sys.path, the oracle is built from the checkout's own oracle/, and the `want` side of six
"walker B with its feature off is walker A" tests is called with those tests' own loops and written to
tests/golden/walker_frames.npz of THIS tree: per group of calls (a test and the walker it called) the calls' keys, IMAGE, HIT_ID,
ALBEDO and seq_n stacked as uint32 bit patterns, `picks` end to end, and the integer counts with their names; tests/path_walker.py's
recorded() reads it back.  The frames of test_lattice_cpu are held as the SHA-256 of IMAGE's bytes: 108 frames of 96 x 12 would be
more than a megabyte.

It runs once, at that commit: the walkers it calls do not exist after it, so it cannot be run on a later checkout (DESIGN.md,
"The test walker")."""
import hashlib
import os
import subprocess
import sys

import numpy as np

U32 = np.uint32
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHA_GROUPS = ("lattice/PW", "lattice/DS")


class Recording:
    def __init__(self):
        self.groups = {}

    def add(self, group, tag, r):
        self.groups.setdefault(group, []).append((",".join(str(t) for t in tag), r))

    def arrays(self):
        out = {}
        for group, calls in self.groups.items():
            first = calls[0][1]
            names = [k for k, v in first.items() if isinstance(v, (int, np.integer)) and not isinstance(v, bool)]
            planes = [p for p in ("IMAGE", "HIT_ID", "ALBEDO", "seq_n") if p in first]
            for key, r in calls:
                assert [p for p in ("IMAGE", "HIT_ID", "ALBEDO", "seq_n") if p in r] == planes, (group, key)
                assert [k for k, v in r.items() if isinstance(v, (int, np.integer)) and not isinstance(v, bool)] == names, (group, key)
            keys = [key for key, _ in calls]
            assert len(set(keys)) == len(keys), (group, keys)
            out[group + "/keys"] = np.array(keys)
            out[group + "/names"] = np.array(names)
            out[group + "/counts"] = np.array([[int(r[k]) for k in names] for _, r in calls], np.int64)
            for p in planes:
                stack = np.stack([np.ascontiguousarray(r[p]).view(U32) for _, r in calls])
                if p == "IMAGE" and group in SHA_GROUPS:
                    out[group + "/IMAGE_sha256"] = np.array([np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8) for a in stack])
                else:
                    out[group + "/" + p] = stack
            if "picks" in first:
                out[group + "/picks"] = np.concatenate([np.asarray(r["picks"], np.int64) for _, r in calls])
                out[group + "/picks_n"] = np.array([len(r["picks"]) for _, r in calls], np.int64)
        return out


def main(checkout):
    checkout = os.path.abspath(checkout)
    sys.path[:0] = [os.path.join(checkout, "tests"), checkout]
    from oracle import oracle as O
    assert os.path.abspath(O.__file__).startswith(checkout + os.sep), O.__file__
    O.build()
    O.set_threads(min(8, os.cpu_count() or 1))
    import dielectric_scenes as DS
    import lattice_paths as LP
    import lattice_scenes as LS
    import nee_paths as NP
    import nee_power as PW
    import nee_scenes as N
    import nee_sphere as NS
    import normal_paths as NRM
    import pathtrace_scenes as P

    W0, H0 = N.SIZES[0]
    W1, H1 = N.SIZES[1]
    NONE = np.zeros(0, U32)
    rec = Recording()

    # 1. test_nee_paths_cpu::test_walker_without_lights_is_the_dielectric_walker
    for form in ("small", "pairs"):
        for segments in (9, 33):
            scene, glass = DS.glass_room(form)
            r = DS.records(scene, None, glass)
            rec.add("nee_paths/DS", (form, segments, "lit"), DS.walk(O, scene, W1, H1, segments, r))
            if segments == 9:
                dark = scene._replace(materials=P._frozen(np.where(np.arange(6)[None, :] >= 3, 0, np.asarray(scene.materials))))
                rec.add("nee_paths/DS", (form, segments, "dark"), DS.walk(O, dark, W1, H1, segments, DS.records(dark, None, glass), spp=2))

    # 2. test_nee_sphere_cpu::test_walker_reduces_to_the_existing_walkers
    scene, glass = NS.glass_room_lit("small")
    r = DS.records(scene, None, glass)
    lights = NP.light_list(scene, 1, r)
    for segments, spp in ((9, 1), (5, 2)):
        rec.add("nee_sphere/DS", (segments, spp), DS.walk(O, scene, W1, H1, segments, r, spp=spp))
        rec.add("nee_sphere/NP", (segments, spp), NP.walk_nee(O, scene, W1, H1, segments, r, lights, spp=spp))
    rec.add("nee_sphere/DS", (1, 2), DS.walk(O, scene, W1, H1, 1, r, spp=2))

    # 3. test_nee_power_cpu::test_power_off_is_the_sphere_walker and test_equal_weights_pick_as_the_uniform_walker
    room, glass, room_rec = PW.glass_room_two_lamps()
    room_lights = NP.light_list(room, 1, room_rec)
    two = NP.two_lamps()
    for sphere in (False, True):
        for sc, r, li, seg, spp in ((room, room_rec, room_lights, 9, 2), (two, DS.records(two), NP.light_list(two), 5, 1)):
            rec.add("nee_power/NS", (sc.name, seg, spp, sphere), NS.walk_nee_sphere(O, sc, W1, H1, seg, r, li, sphere, spp=spp))
    rec.add("nee_power/NS", ("empty",), NS.walk_nee_sphere(O, room, W1, H1, 9, room_rec, NONE, True))
    equal = PW.equal_lamps()
    for segments in (2, 5):
        rec.add("nee_power_equal/NP", (segments,), NP.walk_nee(O, equal, W0, H0, segments, DS.records(equal), NP.light_list(equal)))

    # 4. test_nee_mis_cpu::test_mis_off_is_the_power_walker and test_one_segment_and_an_empty_list_ignore_the_flag
    for power, sphere in ((False, False), (True, False), (True, True)):
        for sc, r, li, seg, spp in ((two, DS.records(two), NP.light_list(two), 5, 1), (room, room_rec, room_lights, 9, 2)):
            rec.add("nee_mis/PW", (sc.name, seg, spp, power, sphere),
                    PW.walk_nee_power(O, sc, W1, H1, seg, r, li, sphere=sphere, power=power, spp=spp))
    rec.add("nee_mis/DS", ("one",), DS.walk(O, room, W1, H1, 1, room_rec))
    for sphere in (False, True):
        rec.add("nee_mis/NS", ("empty", sphere), NS.walk_nee_sphere(O, room, W1, H1, 9, room_rec, NONE, sphere))

    # 5. test_lattice_cpu::test_walker_equals_the_older_walkers_at_level_0
    LW, LH = LS.SHAPES[0]
    for name in LS.SCENES:
        for form in ("small", "odd"):
            c = LS.case(O, name, form)
            sc = c.sh.scene
            s = LS.setup(O, c, 6)
            level0 = LP.textures(c.sh, 1)
            for segments, spp in ((2, 1), (LS.SEGMENTS, 1), (2, 3)):
                for tx in (None, level0):
                    old_tex = None if tx is None else (tx.tri_uv, tx.tri_texture, tx.desc, tx.texels)
                    for sphere in (False, True):
                        for power in (False, True):
                            rec.add("lattice/PW", (name, form, segments, spp, tx is not None, sphere, power),
                                    PW.walk_nee_power(O, sc, LW, LH, segments, s["rec"], s["lights"], sphere=sphere, power=power, spp=spp,
                                                      texture=old_tex))
                rec.add("lattice/DS", (name, form, segments, spp, "no list"), DS.walk(O, sc, LW, LH, segments, s["rec"], spp=spp))

    # 6. test_normal_paths_cpu::test_without_a_smooth_triangle_it_is_the_lattice_walker
    NW, NH = NRM.SHAPE
    for name in NRM.CASES:
        for spec in (2, 4, 5):
            c, nrm = NRM.case(O, name)
            s = NRM.setup(O, c, spec)
            tex = LP.textures(c.sh, 2)
            for demod in (False, True):
                rec.add("normal_paths/LP" + ("/demod" if demod else ""), (name, spec, demod),
                        LP.walk(O, c.sh.scene, NW, NH, 4, rec=s["rec"], lights=s["lights"], sphere=s["sphere"], power=s["power"], tex=tex,
                                demod=demod))

    out = rec.arrays()
    out["parent"] = np.array(subprocess.check_output(["git", "-C", checkout, "rev-parse", "HEAD"], text=True).strip())
    path = os.path.join(HERE, "tests", "golden", "walker_frames.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {sum(len(c) for c in rec.groups.values())} calls in {len(rec.groups)} groups, {os.path.getsize(path)} bytes, "
          f"parent {out['parent']}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
