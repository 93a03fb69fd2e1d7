#!/bin/bash
# Reprojection reuse (the final pass loads the reprojected pixels while its inputs rest) against its parent commit on the GPU
# box, one job on one box.  Every GPU step runs under its own time limit, the steps are chained and nothing is retried.
#   headline   bench.py's default 4K line: parent, change, parent, change, parent, change
#   outputs    bench.py --dump-outputs on both: frame.npy bit for bit, frame_pixel_index.npy equal
#   moving     --camera-keys EQ (no store, no load): parent, change, parent, change
#   others     --workload 1080p and --workload instanced (the per-pixel-normal final pass) on both
#   placement  (optional third argument: a library built with -DRTPT_REPROJ_LOAD_PLACE=4, scripts/build_variant.sh: the other
#              placement of the two loads in both variants — id-pair behind the taps, per-pixel normals ahead of them) the 4K
#              and the instanced line with it, next to the change's
# usage: scripts/ab_reproj_reuse.sh <outdir> <parent_tree> [other_placement_library]
#        (parent_tree: a checkout of the parent commit with its library built)
OUT=$(realpath -m "$1"); PARENT=$(realpath "$2"); LATE=${3:+$(realpath "$3")}; HERE=$PWD
mkdir -p "$OUT"
run() {  # tag tree [bench arguments]
  TAG=$1; TREE=$2; shift 2
  (cd "$TREE" && timeout -k 10 300 python bench.py --gpus 1 --steps 200 --warmup 20 "$@" > "$OUT/$TAG.json" 2> "$OUT/$TAG.err") || { echo "$TAG failed"; tail -3 "$OUT/$TAG.err"; return 1; }
  python - "$OUT/$TAG.json" "$TAG" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(sys.argv[2], "ms/frame", d["ms_per_step"], "Mray/s", d.get("value"), "rays/frame", d.get("rays_per_frame"),
      {n: v["avg_us"] for n, v in d["kernels"].items()})
PY
}
same_outputs() {
  python - "$OUT/dump_parent" "$OUT/dump_change" <<'PY'
import sys
import numpy as np
a, b = (np.load(f"{d}/frame.npy") for d in sys.argv[1:3])
ia, ib = (np.load(f"{d}/frame_pixel_index.npy") for d in sys.argv[1:3])
same = a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ia, ib)
print("outputs: frame.npy", a.shape, "bit-identical and frame_pixel_index.npy equal" if same else "DIFFER")
sys.exit(0 if same else 1)
PY
}
run parent_1 "$PARENT" && run change_1 "$HERE" && run parent_2 "$PARENT" && run change_2 "$HERE" && \
run parent_3 "$PARENT" && run change_3 "$HERE" && \
run dump_parent_line "$PARENT" --dump-outputs "$OUT/dump_parent" && run dump_change_line "$HERE" --dump-outputs "$OUT/dump_change" && same_outputs && \
rm -r "$OUT/dump_parent" "$OUT/dump_change" && \
run moving_parent_1 "$PARENT" --camera-keys EQ && run moving_change_1 "$HERE" --camera-keys EQ && \
run moving_parent_2 "$PARENT" --camera-keys EQ && run moving_change_2 "$HERE" --camera-keys EQ && \
run 1080p_parent "$PARENT" --workload 1080p && run 1080p_change "$HERE" --workload 1080p && \
run instanced_parent "$PARENT" --workload instanced && run instanced_change "$HERE" --workload instanced && \
if [ -n "$LATE" ]; then
  RTPT_LIB_PATH=$LATE run other_4k_1 "$HERE" && run shipped_4k_1 "$HERE" && RTPT_LIB_PATH=$LATE run other_4k_2 "$HERE" && run shipped_4k_2 "$HERE" && \
  RTPT_LIB_PATH=$LATE run other_instanced "$HERE" --workload instanced && run shipped_instanced "$HERE" --workload instanced
fi
