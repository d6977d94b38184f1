"""The voxel map (include/svo.h, "voxel map") against its restatement tests/voxel_ref.py, with ==.

CPU: the restatement's two routes agree on every scene used below; each deliberate misreading of the contract changes the main
scene; svo_pose7_to_cam_to_world, the pure entries and the refusals that need no context.
GPU: table (download, sorted by key), counters and extraction (sorted by record bytes) equal the restatement.  For every scene
whose table is meant not to overflow the test first asserts longest_run(occupied(...)) < 64 on the restatement: the condition
under which no thread order can drop a point.

Misreadings, voxels of the main scene (12,800 records, 12,669 inserted, 131 rejected, 9,581 with a negative camera coordinate;
0.1 m, 5,741 voxels) that change: truncation instead of floor 4,521; the f32-rounded w 943; fraction scale 65535 5,285; no clamp
of f 106; tag & 0xFF instead of tag >> 24 5,717; z >= 0 accepted 1 (the holes, all at the camera centre).
Probe runs of the main scene on the restatement: 0.05 m 10,109 voxels, run 44 at log2 14; 0.1 m run 17 at log2 14 and 71 at log2
13 (the overflow case); 0.25 m 1,501 voxels, run 12 at log2 12; the two-cloud scene 10,970 voxels, run 14 at log2 15.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import voxel_ref as V

MAIN_M = V.rot_y(0.7, (1.5, 0.0, -2.0))
MAIN = ((0.05, 14), (0.1, 14), (0.25, 12))  # voxel size, table log2
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)
VARIANTS = ("trunc", "w_f32", "scale_65535", "no_clamp", "tag_low_byte", "z_ge_0")


@functools.lru_cache(maxsize=None)
def main_scene():
    p = V.scene()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def main_table(vs):
    return V.insert_np(main_scene(), MAIN_M, vs)


def _voxel_records(cells, jitter=True):
    """One record per entry of `cells` (integer voxel coordinates at 0.1 m, z >= 1), somewhere inside its voxel."""
    c = np.asarray(cells, np.float64).reshape(-1, 3)
    i = np.arange(len(c))
    off = np.stack([0.011 + 0.0009 * (i % 87), 0.013 + 0.0007 * (i % 101), 0.017 + 0.0005 * (i % 131)], 1) if jitter else 0.05
    xyz = (c * 0.1 + off).astype(np.float32)
    return V.records(xyz[:, 0], xyz[:, 1], xyz[:, 2], (i | ((i * 37 % 256) << 24)).astype(np.uint32))


def _reject(n=1):
    return V.records(np.zeros(n, np.float32), np.zeros(n, np.float32), np.full(n, -1, np.float32), np.full(n, 0x55000000, np.uint32))


@functools.lru_cache(maxsize=None)
def wave_shapes():
    """name -> (records, m12, voxel size, max_depth, table log2): the shapes the wavefront merge has to get right."""
    A, B = (3, -2, 12), (-4, 5, 20)
    out = {}
    for n in (64, 256):
        out[f"one_voxel_{n}"] = _voxel_records([A] * n)
    distinct = lambda n, x0: [(x0 + i, 1, 15) for i in range(n)]
    out["run_of_100_from_30"] = _voxel_records(distinct(30, 10) + [B] * 100 + distinct(70, 50))  # lanes 30..63, a whole wavefront, lanes 0..1
    out["alternating"] = _voxel_records([A, B] * 65)
    sc = main_scene()
    for n in (1, 63, 65, 257):
        out[f"n_{n}"] = sc[4000:4000 + n].copy()
    parts = []
    for k, run in enumerate((3, 1, 7, 64, 2, 40, 5)):  # runs of A and B with 1..3 rejected records between them
        parts += [_voxel_records([A if k % 2 == 0 else B] * run), _reject(1 + k % 3)]
    out["runs_between_rejects"] = np.concatenate(parts)
    return {k: (v, MAIN_M if k.startswith("n_") else IDENT, 0.1, 0.0, 10) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reject_scene():
    """Hand-made records under identity at 0.25 m (a power of two: q = x * 4 exactly), max_depth 5: (records, kept flags)."""
    f32 = np.float32
    nan, inf = f32("nan"), f32("inf")
    rows = [(1.1, 0.3, 2.0, True)]
    for bad in (nan, inf, -inf):
        rows += [(bad, 0.3, 2.0, False), (1.1, bad, 2.0, False), (1.1, 0.3, bad, False)]
    rows += [(1.1, 0.3, 0.0, False), (1.1, 0.3, -0.0, False), (1.1, 0.3, -2.0, False),
             (1.1, 0.3, np.nextafter(f32(5), f32(6)), False), (1.1, 0.3, 5.0, True),
             (-262144.0, 0.3, 2.0, True), (262144.0, 0.3, 2.0, False),                  # q = -2^20 kept, q = 2^20 rejected
             (np.nextafter(f32(262144), f32(0)), 0.3, 2.0, True),
             (0.3, -262144.0, 2.0, True), (0.3, 262144.0, 2.0, False),
             (-1e-30, 0.3, 2.0, True), (0.3, -1e-30, 2.0, True),                         # q - floor(q) rounds to 1.0: the clamp
             (1.1, 0.3, 1e-30, True), (1.2, 0.3, 2.0, True)]
    a = np.array(rows, np.float64)
    p = V.records(a[:, 0].astype(f32), a[:, 1].astype(f32), a[:, 2].astype(f32), (np.arange(len(a)) * 0x01010101 % (1 << 32)).astype(np.uint32))
    return p, a[:, 3].astype(bool)


ACC_M2 = V.rot_y(0.75, (1.6, 0.0, -2.1))


@functools.lru_cache(maxsize=None)
def second_cloud():
    return V.scene(seed=11)


def all_scenes():
    for vs, lg in MAIN:
        yield f"main_{vs}", main_scene(), MAIN_M, vs, 0.0
    for k, (p, m, vs, md, lg) in wave_shapes().items():
        yield k, p, m, vs, md
    yield "rejects", reject_scene()[0], IDENT, 0.25, 5.0
    yield "second_cloud", second_cloud(), ACC_M2, 0.1, 0.0
    yield "main_max_depth", main_scene(), MAIN_M, 0.1, 6.0


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_scene():
    for name, p, m, vs, md in all_scenes():
        a, b = V.insert_np(p, m, vs, md), V.insert_py(p, m, vs, md)
        assert V.same(a, b), name
        assert a.n_inserted + a.n_rejected == len(p)
    # accumulation: going on in the same dict equals merging two whole-array runs
    V.insert_py(main_scene(), MAIN_M, 0.1)
    both = V.insert_py(second_cloud(), ACC_M2, 0.1, into=V.insert_py.last)
    want = V.merge(main_table(0.1), V.insert_np(second_cloud(), ACC_M2, 0.1))
    assert np.array_equal(both.keys, want.keys) and np.array_equal(both.ci, want.ci) and np.array_equal(both.sx, want.sx)
    assert len(want.keys) < len(main_table(0.1).keys) + 5766 and len(want.keys) > 6000  # the clouds overlap, and differ
    # the reject scene keeps what it says it keeps
    p, kept = reject_scene()
    t = V.insert_np(p, IDENT, 0.25, 5.0)
    assert (t.n_inserted, t.n_rejected) == (int(kept.sum()), int((~kept).sum()))
    for i in range(len(p)):
        assert V.insert_np(p[i:i + 1], IDENT, 0.25, 5.0).n_inserted == int(kept[i]), (i, p[i])
    # the clamp case really is one: its fraction would be 65536
    t = V.insert_py(p[np.isclose(p["x"], -1e-30) & (p["x"] < 0)], IDENT, 0.25, 5.0)
    assert int(t.sx[0]) == 65535 and (int(t.keys[0]) & 0x1FFFFF) == (1 << 20) - 1


def test_every_misreading_of_the_contract_changes_the_main_scene():
    base = main_table(0.1)
    p = main_scene()
    assert int(((p["x"] < 0) | (p["y"] < 0)).sum()) == 9581
    got = {v: V.changed_voxels(base, V.insert_np(p, MAIN_M, 0.1, variant=v)) for v in VARIANTS}
    assert got == {"trunc": 4521, "w_f32": 943, "scale_65535": 5285, "no_clamp": 106, "tag_low_byte": 5717, "z_ge_0": 1}, got


def test_the_main_scene_runs_from_one_to_many_pixels_per_voxel():
    p = main_scene()
    heads = [V.run_heads(p, MAIN_M, vs) for vs, _ in MAIN]
    assert heads[0] > 11000 and heads[2] < 6000, heads  # of 12,800: nearly nothing merges at 0.05 m, most does at 0.25 m
    assert [len(main_table(vs).keys) for vs, _ in MAIN] == [10109, 5741, 1501]
    assert [V.longest_run(V.occupied(main_table(vs).keys, lg)) for vs, lg in MAIN] == [44, 17, 12]
    assert V.longest_run(V.occupied(main_table(0.1).keys, 13)) == 71  # the probe bound bites before the table is full
    occ = np.zeros(16, bool)
    occ[[15, 0, 1, 5, 6]] = True
    assert V.longest_run(occ) == 3 and V.longest_run(np.ones(8, bool)) == 8 and V.longest_run(np.zeros(8, bool)) == 0


def test_pose7_to_cam_to_world_on_the_cpu():
    from stereo_vo_amd import api
    rng = np.random.default_rng(3)
    for scale in (1.0, 0.37, 5.0):  # a non-unit quaternion gives the same rotation
        q = rng.normal(size=4)
        pose = np.concatenate([scale * q / np.linalg.norm(q), rng.normal(size=3) * 4])
        m = api.pose7_to_cam_to_world(pose)
        want = V.pose7_matrix(pose)
        assert np.allclose(m, want, rtol=1e-14, atol=1e-14 * np.abs(want).max()), (m - want)
        R = m[:, :3]
        assert np.allclose(R @ R.T, np.eye(3), rtol=0, atol=1e-14)
        # X_world = R^T (X_cam - t): the camera centre of X_cam = R X + t goes back to X
        X = rng.normal(size=3)
        Xc = R.T @ X + pose[4:]
        assert np.allclose(m[:, :3] @ Xc + m[:, 3], X, rtol=0, atol=1e-13)
    assert np.array_equal(api.pose7_to_cam_to_world([1, 0, 0, 0, 0, 0, 0]), np.eye(3, 4))
    assert np.array_equal(api.pose7_to_cam_to_world([2, 0, 0, 0, 1, -2, 3]), np.hstack([np.eye(3), [[-1], [2], [-3]]]))


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    d = api.voxel_map_default_params()
    assert (d.voxel_size, d.capacity_log2, d.max_depth) == (np.float32(0.1), 22, 0.0)
    assert api.voxel_map_bytes(d) == 40 << 22 == 167772160
    for lg in (8, 28):
        assert api.voxel_map_bytes(api.VoxelMapParams(0.5, lg, -1.0)) == 40 << lg
    n = C.c_size_t(7)
    for bad in (api.VoxelMapParams(0.0, 10, 0), api.VoxelMapParams(-0.1, 10, 0), api.VoxelMapParams(float("nan"), 10, 0),
                api.VoxelMapParams(float("inf"), 10, 0), api.VoxelMapParams(0.1, 7, 0), api.VoxelMapParams(0.1, 29, 0)):
        n.value = 7
        assert L.svo_voxel_map_bytes(C.byref(bad), C.byref(n)) == -1 and n.value == 0
        with pytest.raises(api.SvoError):
            api.voxel_map_bytes(bad)
    assert L.svo_voxel_map_bytes(None, C.byref(n)) == -1
    assert L.svo_voxel_map_bytes(C.byref(d), None) == -1
    assert L.svo_voxel_map_default_params(None) == -1
    buf = (C.c_double * 12)()
    assert L.svo_pose7_to_cam_to_world(None, buf) == -1 and L.svo_pose7_to_cam_to_world(buf, None) == -1
    h = C.c_void_p()
    assert L.svo_voxel_map_create(None, C.byref(d), C.byref(h)) == -1 and not h.value
    # a null map is refused by every entry (and destroying it is a no-op)
    assert L.svo_voxel_map_clear(None) == -1
    assert L.svo_voxel_map_insert_dev(None, None, 0, buf) == -1
    assert L.svo_voxel_map_insert_pose7_dev(None, None, 0, buf) == -1
    assert L.svo_voxel_map_stats(None, buf) == -1
    assert L.svo_voxel_map_extract_dev(None, 1, None, 0, buf) == -1
    assert L.svo_voxel_map_extract(None, 1, None, 0, buf, buf) == -1
    assert L.svo_voxel_map_download(None, buf, 96) == -1
    L.svo_voxel_map_destroy(None)
    assert api.VOXEL_MAX_PROBES == V.MAX_PROBES == 64


# ===================================================================================================== GPU
def _dev(pts):
    import torch
    return torch.from_numpy(np.ascontiguousarray(pts).view(np.int32).reshape(-1, 4).copy()).cuda()


def _insert(vm, pts, m12=None, pose7=None):
    t = _dev(pts)
    vm.insert(t.data_ptr(), len(pts), m12=m12, pose7=pose7)
    vm.ctx.sync()  # the tensor goes out of scope behind this line


def _stored(vm):
    d = vm.download()
    occ = d["keys"] != np.uint64(V.EMPTY)
    for k in ("ci", "sx", "sy", "sz"):
        assert not d[k][~occ].any(), k  # an empty slot has no payload
    o = np.argsort(d["keys"][occ])
    return tuple(d[k][occ][o] for k in ("keys", "ci", "sx", "sy", "sz"))


def _assert_equals(vm, want, n_given, what=""):
    got = _stored(vm)
    for g, name in zip(got, ("keys", "ci", "sx", "sy", "sz")):
        assert np.array_equal(g, getattr(want, name)), (what, name)
    assert vm.stats() == {"n_voxels": len(want.keys), "n_inserted": want.n_inserted, "n_rejected": want.n_rejected, "n_dropped": 0}, what
    assert want.n_inserted + want.n_rejected == n_given


def _fits(keys, lg):
    run = V.longest_run(V.occupied(keys, lg))
    assert run < V.MAX_PROBES, (run, lg)


def _map(ctx, vs, lg, md=0.0):
    import stereo_vo_amd as S
    return S.VoxelMap(ctx, voxel_size=vs, capacity_log2=lg, max_depth=md)


@pytest.mark.gpu
@pytest.mark.parametrize("vs,lg", MAIN)
def test_main_scene_table_counters_and_extraction(ctx, vs, lg):
    import torch
    want = main_table(vs)
    _fits(want.keys, lg)
    vm = _map(ctx, vs, lg)
    _insert(vm, main_scene(), MAIN_M)
    _assert_equals(vm, want, len(main_scene()))
    for min_count in (1, 3):
        ref = V.extract(want, vs, min_count)
        assert 0 < len(ref) and (min_count == 1) == (len(ref) == len(want.keys))
        pts, n_total = vm.extract(min_count)
        assert n_total == len(ref) == len(pts)
        assert np.array_equal(V.sort_records(pts), ref), min_count
    # fewer records than voxels: n_stored of them, each one a true record, no two alike, nothing written behind them
    ref = V.extract(want, vs, 1)
    cut = len(ref) // 3
    buf = torch.full((len(ref) + 8, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    vm.extract_dev(1, buf.data_ptr(), cut, cnt.data_ptr())
    ctx.sync()
    assert cnt.cpu().tolist() == [len(ref), cut]
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[cut:] == 0x5A5A5A5A).all()
    have = {r.tobytes() for r in ref}
    assert len({r.tobytes() for r in got[:cut]}) == cut and all(r.tobytes() in have for r in got[:cut])
    # max_points 0 only counts
    vm.extract_dev(3, None, 0, cnt.data_ptr())
    ctx.sync()
    assert cnt.cpu().tolist() == [len(V.extract(want, vs, 3)), 0]
    vm.close()


@pytest.mark.gpu
def test_max_depth_bounds_the_camera_frame_z(ctx):
    want = V.insert_np(main_scene(), MAIN_M, 0.1, 6.0)
    assert want.n_rejected > 2000 and want.n_inserted > 2000
    _fits(want.keys, 14)
    vm = _map(ctx, 0.1, 14, 6.0)
    _insert(vm, main_scene(), MAIN_M)
    _assert_equals(vm, want, len(main_scene()))
    vm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(wave_shapes()))
def test_wavefront_shapes(ctx, name):
    p, m, vs, md, lg = wave_shapes()[name]
    want = V.insert_np(p, m, vs, md)
    if name.startswith("one_voxel"):
        assert len(want.keys) == 1 and int(want.ci[0]) >> 40 == len(p)
    if name == "alternating":
        assert len(want.keys) == 2 and V.run_heads(p, m, vs) == len(p)
    if name == "run_of_100_from_30":
        assert V.run_heads(p, m, vs) == 30 + 3 + 70
    _fits(want.keys, lg)
    vm = _map(ctx, vs, lg, md)
    _insert(vm, p, m)
    _assert_equals(vm, want, len(p), name)
    pts, n_total = vm.extract(1)
    assert n_total == len(want.keys) and np.array_equal(V.sort_records(pts), V.extract(want, vs, 1))
    vm.close()


@pytest.mark.gpu
def test_rejects(ctx):
    p, kept = reject_scene()
    want = V.insert_np(p, IDENT, 0.25, 5.0)
    _fits(want.keys, 8)
    vm = _map(ctx, 0.25, 8, 5.0)
    _insert(vm, p, IDENT)
    _assert_equals(vm, want, len(p))
    s = vm.stats()
    assert s["n_inserted"] + s["n_rejected"] + s["n_dropped"] == len(p) and s["n_inserted"] == int(kept.sum())
    # one record at a time: the same verdict on each
    vm.clear()
    for i in range(len(p)):
        _insert(vm, p[i:i + 1], IDENT)
        assert vm.stats()["n_inserted"] == int(kept[:i + 1].sum()), (i, p[i])
    _assert_equals(vm, want, len(p))
    vm.close()


@pytest.mark.gpu
def test_accumulation_and_clear(ctx):
    a, b = main_table(0.1), V.insert_np(second_cloud(), ACC_M2, 0.1)
    want = V.merge(a, b)
    assert len(want.keys) < len(a.keys) + len(b.keys)
    _fits(want.keys, 15)
    vm = _map(ctx, 0.1, 15)
    _insert(vm, main_scene(), MAIN_M)
    _insert(vm, second_cloud(), ACC_M2)
    _assert_equals(vm, want, len(main_scene()) + len(second_cloud()))
    vm.clear()
    assert vm.stats() == {"n_voxels": 0, "n_inserted": 0, "n_rejected": 0, "n_dropped": 0}
    d = vm.download()
    assert (d["keys"] == np.uint64(V.EMPTY)).all() and not any(d[k].any() for k in ("ci", "sx", "sy", "sz"))
    assert vm.extract(1)[1] == 0
    _insert(vm, second_cloud(), ACC_M2)
    _assert_equals(vm, b, len(second_cloud()))  # as a fresh map
    vm.close()


def _overflow_invariants(vm, want, n_given):
    keys, ci, sx, sy, sz = _stored(vm)
    s = vm.stats()  # returning at all is the bounded time: a probe sequence ends after 64 slots
    true = {int(k): i for i, k in enumerate(want.keys.tolist())}
    assert len(set(keys.tolist())) == len(keys)  # no key twice
    idx = np.array([true.get(int(k), -1) for k in keys.tolist()])
    assert (idx >= 0).all()  # every stored key is a true key
    count = ci >> np.uint64(40)
    assert (count >= 1).all() and (count <= (want.ci[idx] >> np.uint64(40))).all()
    for g, name in ((ci, "ci"), (sx, "sx"), (sy, "sy"), (sz, "sz")):
        assert (g <= getattr(want, name)[idx]).all(), name
    for g in (sx, sy, sz):
        assert (g <= np.uint64(65535) * count).all()
    assert ((ci & np.uint64((1 << 40) - 1)) <= np.uint64(255) * count).all()
    assert s["n_voxels"] == len(keys)
    assert s["n_inserted"] == int(count.sum())
    assert s["n_inserted"] + s["n_rejected"] + s["n_dropped"] == n_given and s["n_rejected"] == want.n_rejected
    return s


@pytest.mark.gpu
def test_overflow_keeps_its_invariants(ctx):
    # the main scene at 0.1 m in 2^13 slots: load 0.70, yet a run of 71 > 64
    want = main_table(0.1)
    assert V.longest_run(V.occupied(want.keys, 13)) > V.MAX_PROBES
    vm = _map(ctx, 0.1, 13)
    _insert(vm, main_scene(), MAIN_M)
    _overflow_invariants(vm, want, len(main_scene()))
    vm.close()
    # 1,000 distinct voxels into 2^8 slots
    p = _voxel_records([(i % 10, (i // 10) % 10 - 5, 10 + i // 100) for i in range(1000)])
    want = V.insert_np(p, IDENT, 0.1)
    assert len(want.keys) == 1000
    vm = _map(ctx, 0.1, 8)
    _insert(vm, p, IDENT)
    s = _overflow_invariants(vm, want, 1000)
    assert s["n_voxels"] <= 256 and s["n_dropped"] >= 1000 - 256
    # the map is still a map: cleared, it takes a scene that fits
    vm.clear()
    q, m, vs, md, lg = wave_shapes()["alternating"]
    _insert(vm, q, m)
    _assert_equals(vm, V.insert_np(q, m, vs, md), len(q))
    vm.close()


@pytest.mark.gpu
def test_bad_arguments_launch_nothing_and_leave_the_map_usable(ctx):
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    L = ctx.L
    for bad, word in ((dict(voxel_size=0.0), "voxel_size"), (dict(voxel_size=float("nan")), "voxel_size"), (dict(voxel_size=float("inf")), "voxel_size"),
                      (dict(capacity_log2=7), "capacity_log2"), (dict(capacity_log2=29), "capacity_log2")):
        with pytest.raises(S.SvoError, match=word):
            S.VoxelMap(ctx, **{**dict(voxel_size=0.1, capacity_log2=8), **bad})
    h = C.c_void_p()
    assert L.svo_voxel_map_create(ctx.h, None, C.byref(h)) == -1 and "params" in L.svo_last_error(ctx.h).decode()
    assert L.svo_voxel_map_create(ctx.h, C.byref(api.voxel_map_default_params()), None) == -1
    p, m, vs, md, lg = wave_shapes()["alternating"]
    want = V.insert_np(p, m, vs, md)
    vm = _map(ctx, vs, lg, md)
    t = _dev(p)
    m12 = np.ascontiguousarray(m)
    mp = m12.ctypes.data_as(C.c_void_p)
    cnt = _dev(np.zeros(1, V.POINT))
    host = np.empty(4, V.POINT)
    nt, ns = C.c_int(-5), C.c_int(-5)
    small = np.empty(5 * vm.capacity - 1, np.uint64)
    ctx.profile_select("voxel_insert")
    calls = [(lambda: L.svo_voxel_map_insert_dev(vm.h, t.data_ptr(), -1, mp), "n must not"),
             (lambda: L.svo_voxel_map_insert_dev(vm.h, None, 5, mp), "points"),
             (lambda: L.svo_voxel_map_insert_dev(vm.h, t.data_ptr(), 5, None), "m12"),
             (lambda: L.svo_voxel_map_insert_pose7_dev(vm.h, t.data_ptr(), 5, None), "pose7"),
             (lambda: L.svo_voxel_map_stats(vm.h, None), "stats")]
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), word
    assert L.svo_voxel_map_insert_dev(vm.h, None, 0, mp) == 0  # n == 0 is a no-op
    assert ctx.profile_read()[1] == 0
    ctx.profile_select("voxel_extract")
    calls = [(lambda: L.svo_voxel_map_extract_dev(vm.h, 0, t.data_ptr(), 4, cnt.data_ptr()), "min_count"),
             (lambda: L.svo_voxel_map_extract_dev(vm.h, 1, t.data_ptr(), -1, cnt.data_ptr()), "max_points"),
             (lambda: L.svo_voxel_map_extract_dev(vm.h, 1, None, 4, cnt.data_ptr()), "points"),
             (lambda: L.svo_voxel_map_extract_dev(vm.h, 1, t.data_ptr(), 4, None), "counts"),
             (lambda: L.svo_voxel_map_extract(vm.h, 0, host.ctypes.data_as(C.c_void_p), 4, C.byref(nt), C.byref(ns)), "min_count"),
             (lambda: L.svo_voxel_map_extract(vm.h, 1, host.ctypes.data_as(C.c_void_p), -1, C.byref(nt), C.byref(ns)), "capacity"),
             (lambda: L.svo_voxel_map_extract(vm.h, 1, None, 4, C.byref(nt), C.byref(ns)), "points"),
             (lambda: L.svo_voxel_map_extract(vm.h, 1, host.ctypes.data_as(C.c_void_p), 4, None, C.byref(ns)), "n_total"),
             (lambda: L.svo_voxel_map_download(vm.h, None, small.nbytes + 8), "host"),
             (lambda: L.svo_voxel_map_download(vm.h, small.ctypes.data_as(C.c_void_p), small.nbytes), "bytes")]
    for call, word in calls:
        assert call() == -1 and word in L.svo_last_error(ctx.h).decode(), word
    assert ctx.profile_read()[1] == 0
    ctx.profile_select(None)
    assert (nt.value, ns.value) == (-5, -5)
    with pytest.raises(ValueError):
        vm.insert(t.data_ptr(), 5)
    # nothing was inserted; the context and the map work
    assert vm.stats() == {"n_voxels": 0, "n_inserted": 0, "n_rejected": 0, "n_dropped": 0}
    vm.insert(t.data_ptr(), len(p), m12=m)
    _assert_equals(vm, want, len(p))
    vm.close()


@pytest.mark.gpu
def test_end_to_end_from_a_stereo_pair(ctx, frames):
    """A session frame cropped to 192 x 96 -> device StereoBM map -> device cloud -> insert under a pose7, nothing copied to the
    host in between; the restatement runs on the downloaded cloud."""
    import torch
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    p, fr = frames
    W, H = 192, 96
    left, right = (np.ascontiguousarray(x[:H, :W]) for x in fr[1])
    cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
    dl, dr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    dm = torch.empty((H, W), dtype=torch.int16, device="cuda")
    dp = torch.zeros((W * H, 4), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.stereo_bm_batch(dl.data_ptr(), dr.data_ptr(), 1, W, H, W, W * H, dm.data_ptr())
    ctx.disparity_cloud(dm.data_ptr(), dl.data_ptr(), 1, W, H, W, W * H, cam, None, api.CloudParams(1, 0.0, W * H), dp.data_ptr(), cnt.data_ptr())
    ctx.sync()
    n = int(cnt.cpu()[1])
    assert n >= 1000, n
    pose7 = np.array([0.9, 0.05, -0.3, 0.02, 0.4, -0.1, 1.2])
    vm = _map(ctx, 0.1, 16)
    vm.insert(dp.data_ptr(), n, pose7=pose7)
    cloud = dp.cpu().numpy().view(np.uint32)[:n].copy().view(V.POINT).reshape(-1)
    host, n_total = ctx.stereo_cloud(left, right, cam)
    assert n_total == n and np.array_equal(host.view(np.uint32), cloud.view(np.uint32))
    want = V.insert_np(cloud, api.pose7_to_cam_to_world(pose7), 0.1)
    assert want.n_inserted == n and len(want.keys) >= 100
    _fits(want.keys, 16)
    _assert_equals(vm, want, n)
    pts, n_total = vm.extract(2)
    assert np.array_equal(V.sort_records(pts), V.extract(want, 0.1, 2))
    vm.close()
