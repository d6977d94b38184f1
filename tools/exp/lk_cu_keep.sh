#!/bin/bash
# Developer experiment: the pipeline groups' tracker launches restricted to K of every 32 CUs (SVO_GROUP_LK_CU_KEEP)
KEEP=$(mktemp)
for K in "$@"; do
  SVO_GROUP_LK_CU_KEEP=$K timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-other-workloads --no-single 2>/dev/null > "$KEEP"
  python - "$K" "$KEEP" <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
print("LK on", sys.argv[1], "of 32 CUs:", round(d["value"]), "frames/s, host cores", d["config"]["host_cores_busy"], ", LK launch", round(d["roofline"]["dominant_kernel"]["avg_launch_us"]), "us")
PY
done
