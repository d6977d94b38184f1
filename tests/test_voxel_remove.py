"""The voxel map's removal and move (include/svo.h, "Voxel map removal") against the restatement
tests/voxel_remove_ref.py, with ==.

Every scene is a list of steps (insert, remove, move, carve).  CPU: the restatement's two routes agree after every step of every
scene; the main scene's figures; each deliberate misreading of the contract changes a stated scene; the pure entries and the
refusals that need no context.  GPU: after every step the downloaded table sorted by key (zero-payload keys included), the four
counts and svo_voxel_map_stats equal the restatement.  Each scene first asserts longest_run(occupied(...)) < 64 on the restatement.

Main scene (tests/test_voxel_map.py: 160 x 80, 12,800 records per cloud, cloud A under the rotated view, cloud B under a second
pose): removing A from A + B gives counts {12,669, 131, 0, 0} at 0.05, 0.1 and 0.25 m.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import voxel_carve_ref as R
import voxel_ref as V
import voxel_remove_ref as X
import test_voxel_map as T

SIZES = ((0.05, 15), (0.1, 15), (0.25, 12))  # voxel size, table log2 (two clouds)
POSE_A = np.array([1.0333, 0.0044, -0.3772, -0.0033, -2.43, 0.02, 0.56])  # close to the rotated view T.MAIN_M, a non-unit quaternion
POSE_A2 = np.array([1.0333, 0.0054, -0.3792, -0.0033, -2.42, 0.02, 0.57])  # a centimetre and a fraction of a degree away
FAR = V.rot_y(0.7, (1501.5, 0.0, -2.0))  # T.MAIN_M a kilometre and a half away: no voxel in common with anything


def _m(pose_or_m):
    """A step's transform as 12 doubles: a pose7 goes through the library's own pure conversion (its bits are the contract's)."""
    a = np.asarray(pose_or_m, np.float64).reshape(-1)
    if len(a) == 12:
        return a
    from stereo_vo_amd import api
    return api.pose7_to_cam_to_world(a).reshape(12)


def _carve_map():
    """A far surface everywhere: every voxel that projects into the image with its window lies in front of it."""
    return np.full((R.H, R.W), 16, np.int16)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (voxel size, max_depth, table log2, steps).  A step is ("insert", pts, T), ("remove", pts, T, how), ("move", pts,
    T_from, T_to) or ("carve",); T is 12 doubles or a pose7; how is "dev", "nocounts" or "reversed" (the records in reversed
    order); a pose7 as T selects the pose7 entry."""
    A, B = T.main_scene(), T.second_cloud()
    out = {}
    for vs, lg in SIZES:
        for entry, ma in (("dev", T.MAIN_M), ("pose7", POSE_A)):
            out[f"main_{vs}_{entry}"] = (vs, 0.0, lg, [("insert", A, ma), ("insert", B, T.ACC_M2), ("remove", A, ma, "dev"),
                                                       ("insert", A, ma), ("remove", A, ma, "reversed")])
        out[f"everything_{vs}"] = (vs, 0.0, lg, [("insert", A, T.MAIN_M), ("remove", A, T.MAIN_M, "nocounts"), ("insert", A, T.MAIN_M)])
        out[f"move_{vs}"] = (vs, 0.0, lg, [("insert", A, T.MAIN_M), ("move", A, T.MAIN_M, T.ACC_M2)])
    out["move_pose7"] = (0.1, 0.0, 15, [("insert", A, POSE_A), ("move", A, POSE_A, POSE_A2), ("move", A, POSE_A2, POSE_A)])
    out["max_depth"] = (0.1, 6.0, 15, [("insert", A, T.MAIN_M), ("insert", B, T.ACC_M2), ("remove", A, T.MAIN_M, "dev")])
    for name, (p, m, vs, md, lg) in T.wave_shapes().items():  # twice in, three times out: exact, emptied, and all short
        out["wave_" + name] = (vs, md, lg, [("insert", p, m), ("insert", p, m)] + [("remove", p, m, "dev")] * 3)
    p, _ = T.reject_scene()
    out["rejects"] = (0.25, 5.0, 8, [("remove", p, T.IDENT, "dev"), ("insert", p, T.IDENT), ("remove", p, T.IDENT, "dev")])
    out["never_inserted"] = (0.1, 0.0, 14, [("insert", B, T.ACC_M2), ("remove", A, FAR, "dev")])
    for name, (ins, rm, _, _) in X.saturation_scenes().items():
        out["sat_" + name] = (X.VS, 0.0, X.LOG2, [("insert", ins, X.IDENT), ("remove", rm, X.IDENT, "dev")])
    five = X.saturation_scenes()["count_5_minus_2_own"][0]
    both = np.concatenate([five, X.filler(70, row=1)])
    out["sat_remove_twice"] = (X.VS, 0.0, X.LOG2, [("insert", both, X.IDENT), ("remove", both, X.IDENT, "dev"), ("remove", both, X.IDENT, "dev")])
    out["sat_carve_then_remove"] = (X.VS, 0.0, X.LOG2, [("insert", both, X.IDENT), ("carve",), ("remove", both, X.IDENT, "dev")])
    return out


def _as_v(t):
    return V.Table(t.keys, t.ci, t.sx, t.sy, t.sz, 0, 0)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The scene by the restatement, both routes asserted equal: a list, per step, of (Table, counts or None, stats)."""
    vs, md, lg, steps = scenes()[name]
    table, out = None, []
    n_ins = n_rej = 0
    for s in steps:
        counts = None
        if s[0] in ("remove", "move"):
            pts = s[1][::-1] if s[0] == "remove" and s[3] == "reversed" else s[1]
            if table is None:
                table = X.Table(*(np.zeros(0, np.uint64) for _ in range(5)))
            table, counts = X.both(table, pts, _m(s[2]), vs, md)
        if s[0] in ("insert", "move"):
            m = _m(s[3] if s[0] == "move" else s[2])
            t = V.insert_np(s[1], m, vs, md)
            n_ins, n_rej = n_ins + t.n_inserted, n_rej + t.n_rejected
            table = X.insert(table, s[1], m, vs, md)
        if s[0] == "carve":
            a, ca = R.carve_np(_as_v(table), _carve_map(), R.CAM, T.IDENT, vs)
            b, cb = R.carve_py(_as_v(table), _carve_map(), R.CAM, T.IDENT, vs)
            assert V.same(a, b) and ca == cb
            table = X.table_of(a)
        run = V.longest_run(V.occupied(table.keys, lg))
        assert run < V.MAX_PROBES, (name, run, lg)
        out.append((table, counts, {"n_voxels": len(table.keys), "n_inserted": n_ins, "n_rejected": n_rej, "n_dropped": 0}))
    return out


def _zero(t):
    return not any(getattr(t, n).any() for n in ("ci", "sx", "sy", "sz"))


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_scene():
    for name in scenes():
        assert len(restated(name)) == len(scenes()[name][3]), name  # restated() asserts the agreement step by step


def test_the_main_scene_removed_leaves_the_other_cloud():
    A, B = T.main_scene(), T.second_cloud()
    for vs, lg in SIZES:
        for entry, ma in (("dev", T.MAIN_M), ("pose7", _m(POSE_A))):
            steps = restated(f"main_{vs}_{entry}")
            ta, tb = V.insert_np(A, ma, vs), V.insert_np(B, T.ACC_M2, vs)
            got, counts, stats = steps[2]
            assert counts == {"n_removed": 12669, "n_rejected": 131, "n_missing": 0, "n_short": 0}, (vs, entry, counts)
            assert set(got.keys.tolist()) == set(ta.keys.tolist()) | set(tb.keys.tolist())  # the key set is A u B
            on_b = np.isin(got.keys, tb.keys)
            assert X.same(X.Table(*(getattr(got, n)[on_b] for n in X.Table._fields)), X.table_of(tb))  # B's payload on every key of B
            assert 0 < (~on_b).sum() < len(ta.keys) and _zero(X.Table(*(getattr(got, n)[~on_b] for n in X.Table._fields)))  # zero on A-only keys
            assert X.same(X.live(got), X.table_of(tb))
            assert stats["n_inserted"] == ta.n_inserted + tb.n_inserted and stats["n_voxels"] == len(got.keys)
            # the reversed record order changes nothing
            assert X.same(steps[4][0], got) and steps[4][1] == counts
    for vs, _ in SIZES:
        first, gone, again = restated(f"everything_{vs}")
        assert _zero(gone[0]) and np.array_equal(gone[0].keys, first[0].keys) and len(V.extract(_as_v(gone[0]), vs, 1)) == 0
        assert X.same(again[0], first[0])
        before, after = restated(f"move_{vs}")
        fresh = X.table_of(V.insert_np(A, T.ACC_M2, vs))
        assert X.same(X.live(after[0]), fresh)  # clear; insert(A, P2) on the voxels with count > 0
        dead = ~np.isin(after[0].keys, fresh.keys)
        assert dead.sum() > 0 and set(after[0].keys[dead].tolist()) == set(before[0].keys.tolist()) - set(fresh.keys.tolist())
        assert after[1] == {"n_removed": 12669, "n_rejected": 131, "n_missing": 0, "n_short": 0}
    a, b, c = restated("move_pose7")
    assert not X.same(X.live(a[0]), X.live(b[0])) and X.same(X.live(c[0]), a[0])  # there and back again


def test_the_constructed_scenes_are_what_they_were_built_to_be():
    key = X.cell_key(X.CELL)
    for name, (ins, rm, want, n_short) in X.saturation_scenes().items():
        first, (t, counts, _) = restated("sat_" + name)
        assert X.payload(t, key) == want, (name, X.payload(t, key))
        assert counts["n_short"] == n_short and counts["n_missing"] == 0 and counts["n_rejected"] == 0, (name, counts)
    ins, rm, _, _ = X.saturation_scenes()["count_3_minus_2_and_3"]
    assert X.payload(restated("sat_count_3_minus_2_and_3")[0][0], key)[0] == 3
    at = np.flatnonzero(V.insert_np(rm[:1], X.IDENT, X.VS).keys[0] == np.array([V.insert_np(rm[i:i + 1], X.IDENT, X.VS).keys[0] for i in range(len(rm))]))
    assert at.tolist() == [0, 1, 102, 103, 104]  # the two runs sit in different wavefronts
    first, (t, counts, _) = restated("sat_count_5_minus_3_larger")
    assert all(v > 0 for v in X.payload(first[0], key)) and counts["n_removed"] == 3
    # remove twice: the second time every point is short and the table stays zero
    ins, once, twice = restated("sat_remove_twice")
    assert _zero(once[0]) and once[1] == {"n_removed": 75, "n_rejected": 0, "n_missing": 0, "n_short": 0}
    assert _zero(twice[0]) and twice[1] == {"n_removed": 75, "n_rejected": 0, "n_missing": 0, "n_short": 75}
    # carve, then remove: the carved voxel's points are short, the zeros stay, the others are removed exactly
    ins, carved, after = restated("sat_carve_then_remove")
    assert X.payload(carved[0], key) == (0, 0, 0, 0, 0) and int((carved[0].ci == 0).sum()) == 1
    assert _zero(after[0]) and after[1] == {"n_removed": 75, "n_rejected": 0, "n_missing": 0, "n_short": 5}
    # a cloud that was never inserted: every kept point is missing, nothing changes
    (tb, _, _), (t, counts, _) = restated("never_inserted")
    assert X.same(t, tb) and counts == {"n_removed": 0, "n_rejected": 131, "n_missing": 12669, "n_short": 0}
    # rejects: the verdict of the insert, counted in n_rejected, on an empty map and on a filled one
    p, kept = T.reject_scene()
    empty, filled, gone = restated("rejects")
    assert len(empty[0].keys) == 0 and empty[1] == {"n_removed": 0, "n_rejected": int((~kept).sum()), "n_missing": int(kept.sum()), "n_short": 0}
    assert _zero(gone[0]) and gone[1] == {"n_removed": int(kept.sum()), "n_rejected": int((~kept).sum()), "n_missing": 0, "n_short": 0}
    # the wavefront shapes: twice in, once out is one insert; twice out is empty; the third time everything is short
    for name, (p, m, vs, md, lg) in T.wave_shapes().items():
        s = restated("wave_" + name)
        assert X.same(s[2][0], s[0][0]) and _zero(s[3][0]) and _zero(s[4][0]), name
        n_in = s[0][2]["n_inserted"]
        assert [x[1]["n_short"] for x in s[2:]] == [0, 0, n_in] and all(x[1]["n_removed"] == n_in for x in s[2:]), name


def test_every_misreading_of_the_contract_changes_a_stated_scene():
    def run(name, variant):
        vs, md, lg, steps = scenes()[name]
        before = restated(name)[-2][0]
        s = steps[-1]
        return X.remove_np(before, s[1], _m(s[2]), vs, md, variant=variant)

    key = X.cell_key(X.CELL)
    # no zeroing at count 0, and isum not cleared with the count: count 5 minus five OTHER records of smaller fractions and
    # intensities, so that saturation alone leaves something in every field
    five = X.saturation_scenes()["count_5_minus_2_own"][0]
    t5 = X.insert(None, five, X.IDENT, X.VS)
    small = X.in_voxel(X.CELL, [(0.0625, 0.0625, 0.0625)] * 5, [1, 1, 1, 1, 1])
    good, _ = X.both(t5, small, X.IDENT, X.VS)
    assert X.payload(good, key) == (0, 0, 0, 0, 0)
    bad, _ = X.remove_np(t5, small, X.IDENT, X.VS, variant="no_zeroing")
    assert X.payload(bad, key) == (0, 145, 5 * 4096, 5 * 12288, 5 * 20480)
    bad, _ = X.remove_np(t5, small, X.IDENT, X.VS, variant="isum_kept")
    assert X.payload(bad, key) == (0, 145, 0, 0, 0)
    # wrapping instead of saturating: count 5 minus three larger
    good = restated("sat_count_5_minus_3_larger")[-1][0]
    bad, _ = run("sat_count_5_minus_3_larger", "wrap")
    assert X.payload(good, key) == (2, 0, 0, 0, 0) and X.payload(bad, key)[0] == 2 and all(v > 1 << 39 for v in X.payload(bad, key)[1:])
    # claiming on absent keys
    good, gc = restated("never_inserted")[-1][:2]
    bad, bc = run("never_inserted", "claim")
    assert len(bad.keys) > len(good.keys) and bc["n_missing"] == 0 and gc["n_missing"] == 12669
    # n_short per voxel instead of per point
    good = restated("sat_remove_twice")[-1][1]
    _, bc = run("sat_remove_twice", "short_per_voxel")
    assert good["n_short"] == 75 and bc["n_short"] == 71
    # and none of them changes the exact inverse: that is why the scenes above exist
    for v in X.VARIANTS:
        if v != "claim":
            t, c = run("main_0.1_dev", v)
            assert X.same(t, restated("main_0.1_dev")[-1][0]) and c == restated("main_0.1_dev")[-1][1], v


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    assert api.voxel_ledger_bytes(4, 1000) == 64000 and api.voxel_ledger_bytes(1, 1) == 16
    n = C.c_size_t(7)
    for bad in ((0, 5), (5, 0), (-1, 5), (5, -1)):
        n.value = 7
        assert L.svo_voxel_ledger_bytes(C.byref(api.VoxelLedgerParams(*bad)), C.byref(n)) == -1 and n.value == 0
        with pytest.raises(api.SvoError):
            api.voxel_ledger_bytes(*bad)
    assert L.svo_voxel_ledger_bytes(None, C.byref(n)) == -1 and L.svo_voxel_ledger_bytes(C.byref(api.VoxelLedgerParams(1, 1)), None) == -1
    buf = (C.c_double * 12)()
    h = C.c_void_p()
    # a null map or ledger is refused by every entry (and destroying a null ledger is a no-op)
    assert L.svo_voxel_map_remove_dev(None, None, 0, buf, None) == -1
    assert L.svo_voxel_map_remove_pose7_dev(None, None, 0, buf, None) == -1
    assert L.svo_voxel_map_remove_sync(None, None, 0, buf, buf) == -1
    assert L.svo_voxel_map_move_dev(None, None, 0, buf, buf, None) == -1
    assert L.svo_voxel_map_move_pose7_dev(None, None, 0, buf, buf, None) == -1
    assert L.svo_voxel_ledger_create(None, C.byref(api.VoxelLedgerParams(1, 1)), C.byref(h)) == -1 and not h.value
    assert L.svo_voxel_ledger_insert_pose7_dev(None, 1, None, 0, buf) == -1
    assert L.svo_voxel_ledger_update_pose7(None, 1, buf, None) == -1
    assert L.svo_voxel_ledger_retire(None, 1) == -1 and L.svo_voxel_ledger_remove(None, 1, None) == -1
    assert L.svo_voxel_ledger_ids(None, buf, 1, buf) == -1 and L.svo_voxel_ledger_get(None, 1, buf, buf, buf) == -1
    L.svo_voxel_ledger_destroy(None)


# ===================================================================================================== GPU
def _counts_buf():
    import torch
    c = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return c


def _apply(vm, step):
    """One step on the map; the removal's counts as a dict (None where the step has none or was told to take none)."""
    kind = step[0]
    if kind == "insert":
        pose = len(np.asarray(step[2]).reshape(-1)) == 7
        T._insert(vm, step[1], **({"pose7": step[2]} if pose else {"m12": step[2]}))
        return None
    if kind == "carve":
        from test_voxel_carve import _carve
        _carve(vm, _carve_map(), R.CAM, T.IDENT, 1, 8, 0, "dev")
        return None
    pts = step[1][::-1] if kind == "remove" and step[3] == "reversed" else step[1]
    t, c = T._dev(pts), _counts_buf()
    pose = len(np.asarray(step[2]).reshape(-1)) == 7
    if kind == "remove":
        cp = None if step[3] == "nocounts" else c.data_ptr()
        vm.remove(t.data_ptr(), len(pts), counts_ptr=cp, **({"pose7": step[2]} if pose else {"m12": step[2]}))
    else:
        cp = c.data_ptr()
        kw = {"from_pose7": step[2], "to_pose7": step[3]} if pose else {"from_m12": step[2], "to_m12": step[3]}
        vm.move(t.data_ptr(), len(pts), counts_ptr=cp, **kw)
    vm.ctx.sync()  # the tensors go out of scope behind this line
    got = c.cpu().tolist()
    if cp is None:
        assert got == [-1] * 4
        return None
    return dict(zip(X.COUNTS, got))


def _assert_table(vm, want, what=""):
    for g, name in zip(T._stored(vm), X.Table._fields):
        assert np.array_equal(g, getattr(want, name)), (what, name)


SCENE_NAMES = sorted(scenes())


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_step_by_step(ctx, name):
    vs, md, lg, steps = scenes()[name]
    want = restated(name)
    vm = T._map(ctx, vs, lg, md)
    for i, (step, (table, counts, stats)) in enumerate(zip(steps, want)):
        keys_before, stats_before = vm.download()["keys"].copy(), vm.stats()
        got = _apply(vm, step)
        if not (step[0] == "remove" and step[3] == "nocounts"):
            assert got == counts, (name, i, got, counts)
        _assert_table(vm, table, (name, i))
        assert vm.stats() == stats, (name, i)
        if step[0] in ("remove", "carve"):  # keys and the map's counters are byte-identical after any removal
            assert np.array_equal(vm.download()["keys"], keys_before) and vm.stats() == stats_before, (name, i)
    if name.startswith("everything"):
        vm2 = T._map(ctx, vs, lg, md)
        for step in steps[:2]:
            _apply(vm2, step)
        assert vm2.extract(1)[1] == 0  # a map emptied by removal extracts nothing
        vm2.close()
    pts, n_total = vm.extract(1)
    ref = V.extract(_as_v(want[-1][0]), vs, 1)
    assert n_total == len(ref) and np.array_equal(V.sort_records(pts), ref), name
    vm.close()


@pytest.mark.gpu
def test_host_counts_and_bit_equal_matrices(ctx):
    """remove_host_counts gives the restatement's counts; a move between matrices equal in every bit launches nothing (by the
    bracket count) and leaves the table's bytes as they were; a move between different ones is one bracket."""
    vs, md, lg, steps = scenes()["main_0.1_dev"]
    want = restated("main_0.1_dev")
    vm = T._map(ctx, vs, lg)
    for step in steps[:2]:
        _apply(vm, step)
    A = T._dev(T.main_scene())
    before = vm.download()
    before = {k: v.copy() for k, v in before.items()}
    c = _counts_buf()
    for sel in ("voxel_move", "voxel_remove", "voxel_insert"):
        ctx.profile_select(sel)
        vm.move(A.data_ptr(), len(T.main_scene()), from_m12=T.MAIN_M, to_m12=T.MAIN_M.copy(), counts_ptr=c.data_ptr())
        vm.move(A.data_ptr(), len(T.main_scene()), from_pose7=POSE_A, to_pose7=POSE_A.copy())
        assert ctx.profile_read()[1] == 0, sel
    assert c.cpu().tolist() == [-1] * 4
    after = vm.download()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    # two real moves, there and back, are two brackets (on a map of its own: a move leaves zero-payload keys behind)
    restated("move_0.1")  # asserts that both positions of the cloud fit the table together
    vm2 = T._map(ctx, vs, lg)
    T._insert(vm2, T.main_scene(), T.MAIN_M)
    ctx.profile_select("voxel_move")
    vm2.move(A.data_ptr(), len(T.main_scene()), from_m12=T.MAIN_M, to_m12=T.ACC_M2)
    vm2.move(A.data_ptr(), len(T.main_scene()), from_m12=T.ACC_M2, to_m12=T.MAIN_M)
    assert ctx.profile_read()[1] == 2
    assert X.same(X.live(X.Table(*T._stored(vm2))), X.table_of(T.main_table(0.1)))
    vm2.close()
    ctx.profile_select("voxel_remove")
    got = vm.remove_host_counts(A.data_ptr(), len(T.main_scene()), m12=T.MAIN_M)
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    assert got == want[2][1]
    _assert_table(vm, want[2][0])
    assert vm.remove_host_counts(A.data_ptr(), 0, m12=T.MAIN_M) == dict.fromkeys(X.COUNTS, 0)
    with pytest.raises(ValueError):
        vm.remove(A.data_ptr(), 5)
    with pytest.raises(ValueError):
        vm.move(A.data_ptr(), 5, from_m12=T.MAIN_M, to_pose7=POSE_A)
    vm.close()


@pytest.mark.gpu
def test_a_probe_chain_of_64_foreign_slots_is_missing(ctx):
    """A full 2^8 table: a key that is not in it is absent after 64 foreign slots; nothing is written; invariants only."""
    n = 3000
    p = T._voxel_records([(i % 10, (i // 10) % 10 - 5, 10 + i // 100) for i in range(n)])
    keys = V.insert_np(p, T.IDENT, 0.1).keys
    assert len(keys) == n and len({V.fmix64(k) & 255 for k in keys.tolist()}) == 256  # every slot is some key's home: the table fills
    vm = T._map(ctx, 0.1, 8)
    T._insert(vm, p, T.IDENT)
    d = vm.download()
    assert (d["keys"] != np.uint64(V.EMPTY)).all()  # full: every probe sequence meets 64 foreign slots or its key
    stored = set(d["keys"].tolist())
    absent = T._voxel_records([(50 + i, 0, 60) for i in range(130)])
    assert not (set(V.insert_np(absent, T.IDENT, 0.1).keys.tolist()) & stored)
    before, stats = {k: v.copy() for k, v in d.items()}, vm.stats()
    got = _apply(vm, ("remove", absent, T.IDENT, "dev"))
    assert got == {"n_removed": 0, "n_rejected": 0, "n_missing": 130, "n_short": 0}
    after = vm.download()
    assert all(np.array_equal(before[k], after[k]) for k in before) and vm.stats() == stats
    # removing everything that was given: what found its slot is removed (one record per voxel: exactly the inserted ones), what
    # was dropped is missing
    got = _apply(vm, ("remove", p, T.IDENT, "dev"))
    assert got == {"n_removed": stats["n_inserted"], "n_rejected": 0, "n_missing": n - stats["n_inserted"], "n_short": 0}
    after = vm.download()
    assert np.array_equal(after["keys"], before["keys"]) and vm.stats() == stats
    assert not any(after[k].any() for k in ("ci", "sx", "sy", "sz"))
    vm.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_the_map_usable(ctx):
    L = ctx.L
    vs, md, lg, steps = scenes()["wave_alternating"]
    want = restated("wave_alternating")
    p, m = steps[0][1], np.ascontiguousarray(steps[0][2])
    vm = T._map(ctx, vs, lg, md)
    _apply(vm, steps[0])
    t, c = T._dev(p), _counts_buf()
    mp, q = m.ctypes.data_as(C.c_void_p), (C.c_double * 7)(1, 0, 0, 0, 0, 0, 0)
    host = (C.c_uint64 * 4)(9, 9, 9, 9)
    calls = [(lambda: L.svo_voxel_map_remove_dev(vm.h, t.data_ptr(), -1, mp, c.data_ptr()), "n must not"),
             (lambda: L.svo_voxel_map_remove_dev(vm.h, None, 5, mp, c.data_ptr()), "points"),
             (lambda: L.svo_voxel_map_remove_dev(vm.h, t.data_ptr(), 5, None, c.data_ptr()), "m12"),
             (lambda: L.svo_voxel_map_remove_dev(vm.h, t.data_ptr() + 2, 5, mp, c.data_ptr()), "aligned"),
             (lambda: L.svo_voxel_map_remove_dev(vm.h, t.data_ptr(), 5, mp, c.data_ptr() + 4), "counts"),
             (lambda: L.svo_voxel_map_remove_pose7_dev(vm.h, t.data_ptr(), 5, None, c.data_ptr()), "pose7"),
             (lambda: L.svo_voxel_map_remove_sync(vm.h, t.data_ptr(), 5, mp, None), "counts"),
             (lambda: L.svo_voxel_map_remove_sync(vm.h, None, 5, mp, host), "points"),
             (lambda: L.svo_voxel_map_move_dev(vm.h, t.data_ptr(), -1, mp, mp, c.data_ptr()), "n must not"),
             (lambda: L.svo_voxel_map_move_dev(vm.h, None, 5, mp, mp, c.data_ptr()), "points"),
             (lambda: L.svo_voxel_map_move_dev(vm.h, t.data_ptr(), 5, None, mp, c.data_ptr()), "from_m12"),
             (lambda: L.svo_voxel_map_move_dev(vm.h, t.data_ptr(), 5, mp, None, c.data_ptr()), "to_m12"),
             (lambda: L.svo_voxel_map_move_pose7_dev(vm.h, t.data_ptr(), 5, None, q, c.data_ptr()), "from_pose7"),
             (lambda: L.svo_voxel_map_move_pose7_dev(vm.h, t.data_ptr(), 5, q, None, c.data_ptr()), "to_pose7")]
    for sel in ("voxel_remove", "voxel_move", "voxel_insert"):
        ctx.profile_select(sel)
        for call, word in calls:
            assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), word
        assert L.svo_voxel_map_remove_dev(vm.h, None, 0, mp, c.data_ptr()) == 0  # n == 0 is a no-op
        assert L.svo_voxel_map_move_dev(vm.h, None, 0, mp, mp, c.data_ptr()) == 0
        assert ctx.profile_read()[1] == 0, sel
    ctx.profile_select(None)
    assert c.cpu().tolist() == [-1] * 4 and list(host) == [9, 9, 9, 9]
    # nothing was removed; the context and the map work
    _assert_table(vm, want[0][0])
    assert vm.stats() == want[0][2]
    for step, (table, counts, stats) in list(zip(steps, want))[1:]:
        assert _apply(vm, step) == counts
        _assert_table(vm, table)
    vm.close()


@pytest.mark.gpu
def test_after_a_removal_carve_copy_render_and_extraction_see_a_map_that_never_held_the_cloud(ctx):
    from test_voxel_carve import A2W, W2B, _carve, carved_by_b, scene, table_a
    from test_voxel_render import _render
    vs, lg = 0.1, 15
    pts, _, _, db = scene()
    extra = pts[::2]
    me = A2W.copy()  # every second record of the scene again, three centimetres aside: in the same voxels and in their neighbours
    me[3] += 0.03
    me[11] += 0.02
    ta, te = table_a(vs), V.insert_np(extra, me, vs)
    assert len(set(ta.keys.tolist()) & set(te.keys.tolist())) > 50  # the two share voxels: the removal has to be exact there
    both = X.insert(X.table_of(ta), extra, me, vs)
    T._fits(both.keys, lg)
    maps = []
    for with_extra in (True, False):
        vm = T._map(ctx, vs, lg)
        T._insert(vm, pts, A2W)
        if with_extra:
            T._insert(vm, extra, me)
            assert _apply(vm, ("remove", extra, me, "dev")) == {"n_removed": te.n_inserted, "n_rejected": te.n_rejected, "n_missing": 0, "n_short": 0}
        maps.append(vm)

    def live(vm):
        keys, ci, sx, sy, sz = T._stored(vm)
        return X.live(X.Table(keys, ci, sx, sy, sz))

    def views(vm):
        out = [V.sort_records(vm.extract(1)[0]), V.sort_records(vm.extract(3)[0])]
        out += list(_render(vm, R.W, R.H, R.CAM, W2B, 8, 1, "dev"))
        dst = T._map(ctx, vs, lg)
        vm.copy_live_to(dst)
        out.append(live(dst))
        out.append(dst.stats()["n_voxels"])
        dst.close()
        return out

    def same(a, b):
        if isinstance(a, X.Table):
            return X.same(a, b)
        if isinstance(a, tuple):
            return tuple(a) == tuple(b)
        return np.array_equal(a, b)

    assert X.same(live(maps[0]), X.table_of(ta)) and X.same(live(maps[1]), X.table_of(ta))
    assert all(same(a, b) for a, b in zip(views(maps[0]), views(maps[1])))
    want, counts = carved_by_b(vs, 1)
    got = [_carve(vm, db, R.CAM, W2B, 1, 8, 0, "dev") for vm in maps]
    assert got[0] == got[1] == counts
    assert X.same(live(maps[0]), X.live(X.table_of(want))) and X.same(live(maps[1]), X.live(X.table_of(want)))
    assert all(same(a, b) for a, b in zip(views(maps[0]), views(maps[1])))
    for vm in maps:
        vm.close()
