"""The voxel map's keyframe ledger (include/svo.h, "Voxel map ledger").

CPU: the GPU-free table stereo_vo_amd/host/voxel_ledger.h walked by tests/sanitize/voxel_ledger_test.cpp under ASan + UBSan, a
stand-alone program, and beside it the voxel map's other GPU-free host logic, stereo_vo_amd/host/voxel_args.h, walked by
tests/sanitize/voxel_args_test.cpp the same way.  GPU: clouds held, moved, retired and removed through the ledger leave the map
the restatement (tests/voxel_remove_ref.py) gives for the same sequence of inserts, moves and removals, with == on the whole
table; the ledger owns its copies (the caller's buffer is overwritten after every insert); every refusal launches nothing.
"""
import numpy as np
import pytest

import voxel_ref as V
import voxel_remove_ref as X
import test_voxel_map as T
from test_host_sanitizers import _run_sanitized

VS, LG = 0.25, 15


def test_ledger_table_fill_refusals_release_orders_and_random_walk(tmp_path):
    """host/voxel_ledger.h on the CPU under ASan + UBSan: fill, refuse when full, duplicate and unknown ids, oversize n; release in
    every order and slot reuse; the recorded matrix is the inserted one; 10,000 random operations against a std::map model."""
    _run_sanitized(tmp_path, "voxel_ledger_test", "voxel ledger ok")


def test_voxel_args_every_refusal_at_its_boundary_matrices_box_and_geometry(tmp_path):
    """host/voxel_args.h on the CPU under ASan + UBSan: the map's parameters and bytes, the cloud, counts, carve and render
    argument checks with code and exact message on either side of every boundary, the copy's box -> key range (NaN, a voxel
    face and one ulp below it, the clamp at +-2^21), the two matrices of a pose7 (identity and a half turn exactly, composition
    and the 2 / |q|^2 normalisation within 4 ulp for ten seeded poses), the launch geometry without 32-bit wrap."""
    _run_sanitized(tmp_path, "voxel_args_test", "voxel args ok")


def _pose(k, step=0):
    """Keyframe k's pose after `step` refinements: a few centimetres and a fraction of a degree per step."""
    return np.array([1.0, 0.01 * k + 0.002 * step, -0.3 + 0.05 * k - 0.003 * step, 0.004 * k, -2.0 + 0.4 * k + 0.03 * step, 0.02 * step, 0.5 + 0.1 * k])


def _clouds():
    return {10: T.main_scene(), 11: T.second_cloud(), 12: V.scene(seed=12), 13: V.scene(seed=13)[:5000]}


def _m(pose7):
    from stereo_vo_amd import api
    return api.pose7_to_cam_to_world(pose7).reshape(12)


def _put(led, k, pts, pose7):
    """Insert through the ledger, then overwrite the caller's buffer: the ledger must own a copy."""
    import torch
    t = T._dev(pts)
    led.insert(k, t.data_ptr(), len(pts), pose7)
    led.ctx.sync()
    t.fill_(0x7F7F7F7F)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_ledger_moves_retires_and_removes(ctx):
    import stereo_vo_amd as S
    cl = _clouds()
    # the restatement of the same sequence, zero-payload keys and all
    want = None
    for k in (10, 11, 12):
        want = X.insert(want, cl[k], _m(_pose(k)), VS)
    moves = ((10, 0, 1), (11, 0, 1), (11, 1, 2))
    for k, a, b in moves:
        want, c = X.both(want, cl[k], _m(_pose(k, a)), VS)
        assert c["n_short"] == 0 and c["n_missing"] == 0
        want = X.insert(want, cl[k], _m(_pose(k, b)), VS)
    want, c12 = X.both(want, cl[12], _m(_pose(12)), VS)
    final = X.insert(want, cl[13], _m(_pose(13)), VS)
    assert V.longest_run(V.occupied(final.keys, LG)) < V.MAX_PROBES
    last = None  # "each remaining cloud inserted once under its last pose"
    for k, step in ((10, 1), (11, 2)):
        last = X.insert(last, cl[k], _m(_pose(k, step)), VS)
    assert X.same(X.live(want), last) and len(want.keys) > len(last.keys)

    vm = T._map(ctx, VS, LG)
    led = S.VoxelLedger(vm, 3, 12800)
    for k in (10, 11, 12):
        _put(led, k, cl[k], _pose(k))
    assert led.ids() == [10, 11, 12]
    # a full ledger, a held id and an oversize cloud are refused with nothing launched
    big = T._dev(np.concatenate([cl[10], cl[10][:1]]))
    ctx.profile_select("voxel_insert")
    for k, n, word in ((13, 5000, "no free slot"), (11, 5000, "already held"), (13, 12801, "max_points"), (13, -1, "negative")):
        with pytest.raises(S.SvoError, match=word):
            led.insert(k, big.data_ptr(), n, _pose(13))
    assert ctx.profile_read()[1] == 0
    for sel in ("voxel_move", "voxel_remove"):
        ctx.profile_select(sel)
        for call in (lambda: led.update(99, _pose(0)), lambda: led.retire(99), lambda: led.remove(99), lambda: led.get(99)):
            with pytest.raises(S.SvoError, match="unknown id"):
                call()
        assert ctx.profile_read()[1] == 0
    ctx.profile_select("voxel_move")
    led.update(10, _pose(10, 1))
    led.update_all({11: _pose(11, 1)})
    led.update(11, _pose(11, 2))
    led.update(11, _pose(11, 2))  # the same bits again: nothing to do
    assert ctx.profile_read()[1] == 3
    ctx.profile_select(None)
    g = led.get(11)
    assert np.array_equal(g["pose7"], _pose(11, 2)) and g["n"] == 12800 and g["dev"]
    led.retire(10)
    assert led.ids() == [11, 12]
    import torch
    c = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    led.remove(12, counts_ptr=c.data_ptr())
    ctx.sync()
    assert dict(zip(X.COUNTS, c.cpu().tolist())) == c12 and c12["n_short"] == 0 and c12["n_missing"] == 0
    assert led.ids() == [11]
    got = X.Table(*T._stored(vm))
    assert X.same(got, want)
    assert X.same(X.live(got), last)
    # the slots freed by retire and by remove take new clouds; the retired cloud's content stays in the map
    _put(led, 13, cl[13], _pose(13))
    assert led.ids() == [11, 13] and led.get(13)["n"] == 5000
    assert X.same(X.Table(*T._stored(vm)), final)
    _put(led, 10, cl[10][:7], _pose(10))  # the retired id may come again: it is a new cloud to the ledger
    assert led.ids() == [10, 11, 13]
    led.close()
    vm.close()
