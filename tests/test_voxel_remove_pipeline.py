"""GPU: the keyframe ledger over a pipeline and over a pipeline group (include/svo.h, "Voxel map ledger").  Every
keyframe cloud goes into a ledger under results[frame].pose7 from the table's device pointer; after each process call every held
keyframe is updated to its own pose7 plus j * DELTA, j counting that keyframe's updates (the pipeline hands out no refined poses:
DELTA stands in for what bundle adjustment would change); a fifth keyframe retires the oldest.  The final map equals the
restatement (tests/voxel_remove_ref.py) of the same inserts and moves over the host copies of the clouds, with == on the whole
table; frame results, tracked set and clouds are byte-identical to a run with no map at all."""
import numpy as np
import pytest

import voxel_ref as V
import voxel_remove_ref as X
from test_pipeline import _seq
from test_rectify import _bits, _params
from test_voxel_map_pipeline import _bytes

pytestmark = pytest.mark.gpu

W, H, MD = 496, 160, 10.0
VS, LOG2, DEPTH, HELD = 0.25, 15, 15.0, 4
DELTA = np.array([0.0, 0.001, -0.002, 0.0005, 0.01, 0.0, -0.005])  # a centimetre and about a fifth of a degree per update


class _Lane:
    """One lane's ledger loop, and the same operations recorded for the restatement."""

    def __init__(self, ctx):
        import stereo_vo_amd as S
        self.vm = S.VoxelMap(ctx, voxel_size=VS, capacity_log2=LOG2, max_depth=DEPTH)
        self.led = S.VoxelLedger(self.vm, HELD, (W // 2) * (H // 2))
        self.ops, self.held = [], {}  # held: id -> [host points, pose7 at insertion, updates so far]

    def after_call(self, entries):
        """entries: (global frame, table entry, pose7) of this call's keyframe clouds, in frame order."""
        for frame, e, pose in entries:
            if len(self.held) == HELD:  # the oldest keyframe leaves the window: its pose is final
                old = min(self.held)
                self.led.retire(old)
                del self.held[old]
            self.led.insert(frame, e["dev"], e["n_stored"], pose)
            self.held[frame] = [e["points"], np.array(pose), 0]
            self.ops.append(("insert", e["points"], np.array(pose)))
        assert self.led.ids() == sorted(self.held)
        new = {}
        for k, h in self.held.items():
            self.ops.append(("move", h[0], h[1] + h[2] * DELTA, h[1] + (h[2] + 1) * DELTA))
            h[2] += 1
            new[k] = h[1] + h[2] * DELTA
        self.led.update_all(new)

    def check(self):
        from stereo_vo_amd import api
        m = lambda q: api.pose7_to_cam_to_world(q).reshape(12)
        want, n_ins, n_rej, n_given = None, 0, 0, 0
        for op in self.ops:
            pts = op[1].view(V.POINT).reshape(-1)
            if op[0] == "move":
                want, c = X.remove_np(want, pts, m(op[2]), VS, DEPTH)
                assert c["n_short"] == 0 and c["n_missing"] == 0
            t = V.insert_np(pts, m(op[-1]), VS, DEPTH)
            n_ins, n_rej, n_given = n_ins + t.n_inserted, n_rej + t.n_rejected, n_given + len(pts)
            want = X.insert(want, pts, m(op[-1]), VS, DEPTH)
        assert V.longest_run(V.occupied(want.keys, LOG2)) < V.MAX_PROBES
        # what is live is every cloud once, under its last pose
        last, final = None, {}
        for op in self.ops:
            final[id(op[1])] = (op[1], op[-1])
        for pts, pose in final.values():
            last = X.insert(last, pts.view(V.POINT).reshape(-1), m(pose), VS, DEPTH)
        assert X.same(X.live(want), X.live(last)) and len(want.keys) >= len(last.keys)
        d = self.vm.download()
        occ = d["keys"] != np.uint64(V.EMPTY)
        o = np.argsort(d["keys"][occ])
        for name in X.Table._fields:
            assert np.array_equal(d[name][occ][o], getattr(want, name)), name
        assert self.vm.stats() == {"n_voxels": len(want.keys), "n_inserted": n_ins, "n_rejected": n_rej, "n_dropped": 0}
        assert n_ins + n_rej == n_given
        return want, n_ins

    def close(self):
        self.led.close()
        self.vm.close()


def test_pipeline_keyframes_through_a_ledger(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    n, call = 12, 4
    p, L, R = _seq(n, w=W, h=H, seed=0x5EED0A00)
    pp = _params(S, p, MD)
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(lane):
        pl = S.Pipeline(ctx, pp)
        pl.set_keyframe_clouds(prm)
        res, tabs = [], []
        for b0 in range(0, n, call):
            r = pl.process_batch(L[b0:b0 + call], R[b0:b0 + call])
            res += r
            tab = pl.keyframe_clouds()
            if lane is not None:  # before the next call replaces the clouds
                lane.after_call([(b0 + t["frame"], t, np.array(r[t["frame"]].pose7)) for t in tab])
            tabs += _bytes(tab)
        ids, xy = pl.tracked()
        pl.close()
        return [_bits(x) for x in res], tabs, (ids.tobytes(), xy.tobytes())

    res0, tabs0, tracked0 = run(None)  # with no map anywhere
    lane = _Lane(ctx)
    res1, tabs1, tracked1 = run(lane)
    assert res1 == res0 and tabs1 == tabs0 and tracked1 == tracked0
    n_moves = sum(1 for op in lane.ops if op[0] == "move")
    assert len(lane.ops) - n_moves >= 3 and n_moves >= 4, [op[0] for op in lane.ops]
    want, n_ins = lane.check()
    assert n_ins >= 5000 and len(want.keys) >= 100
    lane.close()


def test_group_lanes_each_through_a_ledger_of_their_own(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    lanes, batch, calls = 2, 2, 3
    n = batch * calls
    seqs = [_seq(n, w=W, h=H, seed=0x5EED0A00 + 17 * i) for i in range(lanes)]
    pp = _params(S, seqs[0][0], MD)
    Ls, Rs = np.stack([s[1] for s in seqs]), np.stack([s[2] for s in seqs])
    prm = api.CloudParams(2, 0.0, (W // 2) * (H // 2))

    def run(ledgers):
        g = S.PipelineGroup(ctx, pp, lanes)
        g.set_keyframe_clouds(-1, prm)
        res, tabs = [[] for _ in range(lanes)], []
        for b0 in range(0, n, batch):
            r = g.process_batch(Ls[:, b0:b0 + batch], Rs[:, b0:b0 + batch])
            tab = g.keyframe_clouds()
            for l in range(lanes):
                res[l] += [_bits(x) for x in r[l]]
                if ledgers is not None:
                    ledgers[l].after_call([(b0 + t["frame"], t, np.array(r[l][t["frame"]].pose7)) for t in tab if t["lane"] == l])
            tabs += _bytes(tab)
        g.close()
        return res, tabs

    res0, tabs0 = run(None)
    ledgers = [_Lane(ctx) for _ in range(lanes)]
    res1, tabs1 = run(ledgers)
    assert res1 == res0 and tabs1 == tabs0
    wants = [lane.check()[0] for lane in ledgers]
    assert all(sum(1 for op in lane.ops if op[0] == "insert") >= 1 for lane in ledgers)
    assert not np.array_equal(wants[0].keys, wants[1].keys)
    for lane in ledgers:
        lane.close()
