#!/bin/bash
# the tracker's XCD-aware feature -> workgroup map (SVO_GROUP_LK_XCD, SVO_GROUP_LK_CHUNKS) against blockIdx = (feature, lane)
set -uo pipefail
cd "${GRAFT_REPO_ROOT:-.}"
one() { python bench.py --full --steps 10 --warmup 3 --no-single --no-cpu-baseline --no-other-workloads --no-streaming "$@" 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); t=d['roofline']['tracker_kernel']; print('%.0f frames/s, differ %d, lk %.0f us x %d' % (d['value'], d['parity_self']['lane_steps_that_differ_from_step_0'], t['avg_launch_us'], t['launches']))"; }
echo "warm-up run: $(one)"
for r in 1 2; do
  for c in ${SWEEP_CHUNKS:-8 16 32}; do echo "xcd map, $c chunks: $(SVO_GROUP_LK_CHUNKS=$c one)"; done
  echo "feature x lane grid: $(SVO_GROUP_LK_XCD=0 one)"
done
