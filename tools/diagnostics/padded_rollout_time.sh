#!/bin/sh
# profiles/padded_rollout.txt: ms per model call of the T = 3 training step and of the T = 8 forecast on auto-padded grids (and on
# the enclosing grids that fit) on this tree (native route and use_native_rollout = False), on a built checkout of the PARENT commit
# (the yardstick; on a padded grid it only has the generic route), and on this tree again; then the flagship benchmark on both.
# Every GPU step under its own time limit, the chain ending at the first failure.
#   tools/diagnostics/padded_rollout_time.sh OUT_DIR [PARENT_TREE]
# PARENT_TREE: a checkout of the parent commit with its library built; this script's Python file is run against it unchanged.
set -e
here=$(cd "$(dirname "$0")" && pwd)
root=$(cd "$here/../.." && pwd)
out=${1:?output directory}
parent=${2:-}
mkdir -p "$out"
out=$(cd "$out" && pwd)
timeout -k 10 420 python "$here/padded_rollout_time.py" --entry-points > "$out/padded_rollout_this.json"
if [ -n "$parent" ]; then
    cp "$here/padded_rollout_time.py" "$parent/tools/diagnostics/padded_rollout_time.py"
    timeout -k 10 420 python "$parent/tools/diagnostics/padded_rollout_time.py" > "$out/padded_rollout_parent.json" &&
    timeout -k 10 420 python "$here/padded_rollout_time.py" > "$out/padded_rollout_this_again.json" &&
    # (no pipe behind a GPU step: its own exit status ends the chain; the JSON line is taken afterwards, off the GPU)
    (cd "$root" && timeout -k 10 300 python bench.py --gpus 1 --steps 10 --warmup 3 > "$out/bench_this.log") &&
    (cd "$parent" && timeout -k 10 300 python bench.py --gpus 1 --steps 10 --warmup 3 > "$out/bench_parent.log") &&
    (cd "$root" && timeout -k 10 300 python bench.py --gpus 1 --steps 10 --warmup 3 > "$out/bench_this_again.log") &&
    for name in bench_this bench_parent bench_this_again; do tail -n 1 "$out/$name.log" > "$out/$name.json"; done
fi
