#!/bin/bash
# Albedo demodulation (RTPT_FLAG_EXT_DEMODULATE) against its parent commit on the GPU box, one job on one box:
# bench.py's default 4K line for parent, change, parent, change, then the change with --flags 0x8000 twice.
# usage: scripts/ab_demodulate.sh <outdir> <parent_tree>    (parent_tree: a checkout of the parent commit with its library built)
OUT=$(realpath -m "$1"); PARENT=$(realpath "$2"); HERE=$PWD
mkdir -p "$OUT"
run() {  # tag tree [bench arguments]
  TAG=$1; TREE=$2; shift 2
  (cd "$TREE" && timeout -k 10 300 python bench.py --gpus 1 --steps 200 --warmup 20 "$@" > "$OUT/$TAG.json" 2> "$OUT/$TAG.err") || { echo "$TAG failed"; tail -3 "$OUT/$TAG.err"; return 1; }
  python - "$OUT/$TAG.json" "$TAG" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(sys.argv[2], "ms/frame", d["ms_per_step"], {n: v["avg_us"] for n, v in d["kernels"].items()})
PY
}
run parent_1 "$PARENT" && run change_1 "$HERE" && run parent_2 "$PARENT" && run change_2 "$HERE" && \
run demodulate_1 "$HERE" --flags 0x8000 && run demodulate_2 "$HERE" --flags 0x8000
