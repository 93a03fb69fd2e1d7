"""Regenerates tests/golden/refshader_bars.json and tests/golden/refshader_cornell_64x48.npz.  Needs the shader host
(oracle/_ref/librefshader.so, built by __graft_entry__.build() on a machine that has the reference tree):

    python tests/golden/make_refshader.py

refshader_bars.json — tolerances are measured, not chosen.  For each float observable the bar for "oracle vs R64" (and for
the HIP path vs R64) is the largest error of R32 vs R64 over the test inputs — the reference text's own binary32 rounding
noise — times 4; the file also records the measured maxima, the observed oracle errors and the shares of pixels left out.

refshader_cornell_64x48.npz — data recorded from runs of the reference's shader text, so that the pin survives on a
machine without the reference tree: Cornell box, frames 0-3 of compare.SCRIPT, 32 segments, N = 5 (layout:
compare.record_fixture)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from oracle.refshader import compare as X  # noqa: E402
from oracle.refshader import refshader as R  # noqa: E402

SCENE = os.path.join(ROOT, "real_time_path_tracing_with_spatiotemporal_filtering_amd", "scenes", "CornellBox-Original-Merged.obj")
FACTOR = 4.0
FIX_W, FIX_H, FIX_SEG, FIX_N = 64, 48, 32, 5


def cases(cornell):
    for (w, h) in X.SIZES:
        for seg in X.SEGMENTS:
            yield f"cornell {w}x{h} seg {seg}", w, h, cornell, seg, (X.ITERATIONS if seg == 8 else ())
    yield "sphere 64x48 seg 32", 64, 48, X.sphere_scene(), 32, (5,)


def main():
    assert R.available(), "build the shader host first (needs the reference tree)"
    O.set_threads(min(8, os.cpu_count() or 1))
    xyz, idx = O.load_obj(SCENE)
    cornell = O.flatten(xyz, idx)
    worst = {}
    for tag, w, h, tris, seg, its in cases(cornell):
        for f in X.oracle_frames(w, h, tris, seg, 5):
            obs = X.observe(f, its)
            obs.pop("_runs")
            for k, pairs in obs.items():
                for pair, v in pairs.items():
                    cur = worst.setdefault(k, {}).setdefault(pair, {"value": 0, "where": ""})
                    if v >= cur["value"]:
                        cur["value"], cur["where"] = v, f"{tag} frame {f.pc.frameNumber}"
    wh = X.whole_errors(X.whole_frames(cornell, **X.WHOLE))
    worst["whole"] = {pair: {"value": v, "where": "cornell %(W)dx%(H)d seg %(seg)d N %(n_it)d, frames 0-3" % X.WHOLE} for pair, v in wh.items()}
    bars = {k: FACTOR * worst[k]["r32/r64"]["value"] for k in ("traced", "dir0", "lambda", "filtered", "whole")}
    doc = {
        "_doc": "written by tests/golden/make_refshader.py; bar = factor x (largest R32-vs-R64 error of the reference text)",
        "factor": FACTOR, "colour_floor": X.COLOUR_FLOOR, "bars": bars, "measured": worst,
        "conditions": {"max_diverged_share": X.MAX_DIVERGED, "max_on_integer_share": X.MAX_ON_INTEGER},
    }
    with open(os.path.join(HERE, "refshader_bars.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    # ---- fixture
    path = os.path.join(HERE, "refshader_cornell_64x48.npz")
    np.savez_compressed(path, **X.record_fixture(cornell, FIX_W, FIX_H, FIX_SEG, FIX_N))
    print(json.dumps({"bars": bars, "diverged": worst["diverged"], "pp": worst.get("pp_mismatch"),
                      "pp_excluded": worst.get("pp_excluded"), "measured": {k: worst[k] for k in bars}}, indent=1))
    print("fixture bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
