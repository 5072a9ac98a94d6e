#!/bin/bash
# A/B of SVO_HIP_SIA_OPT_REDUCTION on the SAME box: tools/ab_reduction.sh [lib.so ...]  (default: the in-tree library)
# Every library runs bench.py's plain line (C1: 2000 patches, 4096 pairs per launch) with the default per-wave sums and with
# the tile-order sums (set through hip.SIA_DEFAULT_OPTIONS, which every solver object bench.py creates starts with;
# bench.py itself is untouched), interleaved AB_ROUNDS (3) times so that clock drift and the spread of a leg's own repeats
# show.  A library without the option (an older build) runs the default leg only.
cd "$(dirname "$0")/.."
tmp=$(mktemp -d) && trap 'rm -rf "$tmp"' EXIT
[ $# -eq 0 ] && set -- android_svo_amd/csrc/libsvo_hip.so
for round in $(seq 1 "${AB_ROUNDS:-3}"); do
  for lib in "$@"; do
    for mode in per_wave tile_order; do
      if [ "$mode" = tile_order ] && ! python -c "import ctypes, sys; ctypes.CDLL(sys.argv[1]).svo_hip_tracker_set_sia_option" "$PWD/$lib" 2> /dev/null; then continue; fi
      SVO_HIP_LIB="$PWD/$lib" AB_MODE=$mode timeout -k 10 300 python - --gpus 1 --steps "${AB_STEPS:-100}" --warmup "${AB_WARMUP:-5}" ${AB_ARGS} > "$tmp/ab.json" 2> "$tmp/ab.err" <<'PY' || { tail -5 "$tmp/ab.err"; exit 1; }
import os, runpy, sys
from android_svo_amd import hip
if os.environ["AB_MODE"] == "tile_order":
    hip.SIA_DEFAULT_OPTIONS[hip.SIA_OPT_REDUCTION] = hip.SIA_REDUCTION_TILE_ORDER
sys.argv[0] = "bench.py"
runpy.run_path("bench.py", run_name="__main__")
PY
      python - "$lib" "$mode" "$tmp/ab.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[3]).read().strip().splitlines()[-1])
print("%-40s %-10s %10.1f frames/s  %.4f ms/step" % (sys.argv[1], sys.argv[2], d["value"], d["ms_per_step"]))
PY
    done
  done
done
