"""Worker for tests/test_lk_paths.py::test_hip_per_level_pyramid_equals_the_restatements: the pyramid through one pyr_down_kernel
launch per level.  The library reads SVO_PYR_PER_LEVEL once per process, hence a process of its own; it reads the images of
argv[1] (npz, "<w>x<h>") and writes every level to argv[2] ("<w>x<h>_<level>")."""
import os
import sys

import numpy as np

try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's is loaded first, as in conftest.py)
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    src, dst = sys.argv[1], sys.argv[2]
    assert os.environ.get("SVO_PYR_PER_LEVEL") == "1"
    import stereo_vo_amd as S
    ctx = S.Context(1280, 720, max_batch=1, max_corners=256, max_candidates=1 << 12)
    res = {}
    for key, img in np.load(src).items():
        for l, lv in enumerate(ctx.build_pyramid(img)):
            res["%s_%d" % (key, l)] = lv
    ctx.close()
    np.savez(dst, **res)


if __name__ == "__main__":
    main()
