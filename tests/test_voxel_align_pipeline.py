"""GPU: a pipeline's keyframe clouds aligned against a voxel map before they are inserted (include/svo.h, "Voxel map align";
INTEGRATION 4a).  Three process calls with keyframe clouds on: the first keyframe's cloud is inserted under its pose7; every later
keyframe's cloud is aligned from its own pose7 and from that pose displaced (half a voxel along (0.6, -0.5, 0.62), 0.01 rad about
(0.5, 0.7, -0.5)), from the table's device pointer, and then inserted under the result of the first.  Everything equals the
restatement (tests/voxel_align_ref.py) over the host copies of the same clouds and the downloaded table; frame results, tracked
set and clouds are byte-identical to a run that never aligns."""
import numpy as np
import pytest

import voxel_align_ref as A
import voxel_ref as V
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_map_pipeline import DEPTH, H, LOG2, MD, VS, W, _bytes

pytestmark = pytest.mark.gpu


def _pose(frame):
    """A pose7 per keyframe, a non-unit quaternion close to the identity: the clouds of successive keyframes overlap."""
    return np.array([1.0, 0.001 * frame, -0.002 * frame, 0.0003 * frame, 0.01 * frame, 0.0, 0.005 * frame])


def _f64bits(a):
    return np.asarray(a, np.float64).view(np.uint64).tolist()


def test_keyframe_clouds_aligned_before_they_are_inserted(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))
    ap = A.default_params(VS, max_iters=4)

    def run(vm):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs, log = [], [], []
        for b0 in range(0, n, call):
            res += pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
            tab = pl.keyframe_clouds()
            for t in tab if vm is not None else ():
                pose = _pose(b0 + t["frame"])
                if vm.stats()["n_inserted"] == 0:
                    vm.insert(t["dev"], t["n_stored"], pose7=pose)
                    continue
                d = {k: v.copy() for k, v in vm.download().items()}
                pts = t["points"].view(V.POINT)
                moved = np.array(A.displaced(pose, [0.5 * VS * c for c in (0.6, -0.5, 0.62)], [0.01 * c for c in (0.5, 0.7, -0.5)]))
                for start in (pose, moved):
                    got_out, got = vm.align(t["dev"], t["n_stored"], start, **ap._asdict())
                    out, want, _ = A.loop(start, ap, lambda m: A.sums_np(d, pts, m, VS, DEPTH, ap))
                    assert _f64bits(got_out) == _f64bits(out) and _f64bits(got["xi"]) == _f64bits(want["xi"])
                    assert {k: v for k, v in got.items() if k != "xi"} == {k: v for k, v in want.items() if k != "xi"}, (got, want)
                    log.append((want["status"], want["iterations"], want["first_matched"]))
                    if start is pose:
                        refined = got_out
                after = vm.download()
                assert all(np.array_equal(d[k], after[k]) for k in d)  # aligning changes nothing in the map
                vm.insert(t["dev"], t["n_stored"], pose7=refined)
            tabs += _bytes(tab)
        ids, xy = pl.tracked()
        pl.close()
        return [_bits(r) for r in res], tabs, (ids.tobytes(), xy.tobytes()), log

    res0, tabs0, tracked0, _ = run(None)
    vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
    res1, tabs1, tracked1, log = run(vm)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    assert len(log) >= 2 and any(first > 64 for _, _, first in log), log  # at least one keyframe was aligned, and it found the map
    vm.close()
