#!/bin/sh
# profiles/inter_steps_rollout.txt: ms per model call of the K = 2 training step and of the T = 8 forecast on this tree (native route
# and use_native_rollout = False), and on a built checkout of the PARENT commit (the yardstick; it only has the generic route),
# every GPU step under its own time limit, the chain ending at the first failure.
#   tools/diagnostics/inter_steps_time.sh OUT_DIR [PARENT_TREE]
# PARENT_TREE: a checkout of the parent commit with its library built; this script's Python file is run against it unchanged.
set -e
here=$(cd "$(dirname "$0")" && pwd)
out=${1:?output directory}
parent=${2:-}
mkdir -p "$out"
timeout -k 10 420 python "$here/inter_steps_time.py" > "$out/inter_steps_this.json"
if [ -n "$parent" ]; then
    cp "$here/inter_steps_time.py" "$parent/tools/diagnostics/inter_steps_time.py"
    timeout -k 10 420 python "$parent/tools/diagnostics/inter_steps_time.py" > "$out/inter_steps_parent.json" &&
    timeout -k 10 420 python "$here/inter_steps_time.py" > "$out/inter_steps_this_again.json"
fi
