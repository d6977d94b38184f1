"""Worker for tests/test_corner_paths.py::test_two_pass_form_reaches_every_decision: corner detection through the f32 response map
(corner_response_kernel + corner_nms_kernel).  The library reads SVO_CORNER_TWO_PASS once per process, hence a process of its own;
it writes every case's corner list and the test compares them with the restatement."""
import os
import sys

import numpy as np

try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's is loaded first, as in conftest.py)
except Exception:  # pragma: no cover
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import corner_ref as CR  # noqa: E402


def main():
    out = sys.argv[1]
    assert os.environ.get("SVO_CORNER_TWO_PASS") == "1"
    import stereo_vo_amd as S
    ctx = S.Context(1280, 720, max_batch=1, max_corners=4096, max_candidates=1 << 17)
    res = {cid: ctx.corner_detect(img, maxc, q, md) for cid, (img, maxc, q, md) in CR.cases().items()}
    ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main()
