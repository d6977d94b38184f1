"""The ground plan waypoints (include/svo.h, "Ground plan waypoints") against their restatement tests/grid_waypoints_ref.py,
with == on way, way_index, way_len, way_status and all eight counts, and on length by bit pattern.

CPU: the restatement's two routes (plain Python loops, whole arrays in numpy) agree on every case used below; every deliberate
misreading of the contract differs from the reference on one committed input at least; no step of a route-made path is forced when
min_dist2 is 0 (rule 5's theorem); the pure entries and the refusals that need no context; stereo_vo_amd/host/waypoint_args.h walked by
tests/sanitize/grid_waypoints_args_test.cpp under ASan + UBSan.
GPU: route-made paths on seeded grids of 1 x 1, 1 x 40, 40 x 1, 17 x 33, 64 x 64 and 8192 x 3 at three densities and max_look 1, 2, 8 and
255, starts anywhere in the grid (waypoints within max_look of every edge and corner, every route status); straight paths of 1, 2, 3,
max_look, max_look + 1 and max_look + 2 cells; a serpentine of 674 cells on 64 x 64; n_paths 1, 65 and 4,096; path_stride below path_len;
max_way 1, 2 and w - 1; min_dist2 with and without dist2; paths over cells closed after the route was made (forced steps); lists with
non-adjacent and repeated entries, an entry >= na*nb and an entry 0xFFFFFFFF; each route status and no path_status; each optional
output left out alone, no counts, a repeated call byte for byte; the host entry; every refusal with zero brackets.  Every device call runs into sentinel-filled outputs whose guard elements stay, with the inputs between
guard elements.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import grid_route_ref as R
import grid_waypoints_ref as G
from test_host_sanitizers import _run_sanitized

SENT = 0x3333CCCC  # what way and way_index hold before a device call; no cell index and no path index reaches it
OUTPUTS = ("way", "way_index", "way_len", "way_status", "length")
GRIDS = ((1, 1), (1, 40), (40, 1), (17, 33), (64, 64), (8192, 3))
LOOKS = (1, 2, 8, 255)


def _straight(nb, count, at=0):
    return [at + i for i in range(count)]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case: every input the tests below use, made once"""
    c = {}
    for g, (na, nb) in enumerate(GRIDS):
        for d, density in enumerate(G.DENSITIES):
            look = LOOKS[(g + d) % 4]
            big = na == 8192
            c[f"route-{na}x{nb}-{d}-look{look}"] = G.route_case(na, nb, density / 4 if big else density, 4 if big else 8, look, seed=11 + d,
                                                               router=R.route_py if big else None)
    c["route-8192x3-open-look255"] = G.route_case(8192, 3, 0.0, 3, 255, seed=2, router=R.route_py, max_way=40)
    c["route-64x64-open-look255"] = G.route_case(64, 64, 0.01, 8, 255, seed=4)
    c["route-17x33-look255"] = G.route_case(17, 33, 0.18, 16, 255, seed=6)
    c["route-64x64-look2-dist2"] = G.route_case(64, 64, 0.05, 8, 2, seed=8, with_dist2=True, min_dist2=3)
    c.update(G.misreading_cases())
    c["min_dist2-without-dist2"] = c["dist2"]._replace(dist2=None)
    c["serpentine"] = G.serpentine_case()
    c["serpentine-look255"] = G.serpentine_case(max_look=255, max_way=700)
    for max_way in (1, 2):
        c[f"serpentine-max_way{max_way}"] = G.serpentine_case(max_way=max_way)
    w = int(G.waypoints_np(*c["serpentine"]).way_len[0])
    c["serpentine-max_way-w-1"] = G.serpentine_case(max_way=w - 1)
    c["serpentine-max_way-w"] = G.serpentine_case(max_way=w)
    c["paths-65"] = G.route_case(17, 33, 0.18, 65, 8, seed=21, max_way=8)
    c["paths-4096"] = G.route_case(17, 33, 0.1, 4096, 8, seed=22, max_path=24, max_way=6)
    c["stride-below-len"] = G.route_case(17, 33, 0.18, 32, 8, seed=23, max_path=7)
    c["stride-below-len-full"] = G.route_case(17, 33, 0.18, 32, 2, seed=23, max_path=7, max_way=2)
    c["no-status"] = c["route"]._replace(path_status=None)
    L = 8
    lengths = (1, 2, 3, L, L + 1, L + 2)
    c["straight-1x40"] = G.list_case(1, 40, [_straight(40, k) for k in lengths] + [_straight(40, k, 40 - k) for k in lengths], L)
    c["straight-40x1"] = G.list_case(40, 1, [_straight(1, k) for k in lengths], L, max_way=2)
    c["one-cell"] = G.list_case(1, 1, [[0], [0, 0, 0], [0, 0]], 2)
    c["one-cell-closed"] = G.list_case(1, 1, [[0], [0, 0, 0]], 2, blocked=np.ones((1, 1), np.uint8))
    rng = np.random.default_rng(5)
    wild = [rng.integers(0, 17 * 33, 30).tolist() for _ in range(6)] + [[5, 5, 5, 6, 6, 40, 40, 5]]  # non-adjacent and repeated entries
    c["wild-lists"] = G.list_case(17, 33, wild, 8, blocked=(rng.random((17, 33)) < 0.05).astype(np.uint8), max_way=32)
    c["wild-lists-look255"] = c["wild-lists"]._replace(prm=c["wild-lists"].prm._replace(max_look=255))
    n = 17 * 33
    bad = [[1, 2, n, 3], [1, 2, G.NONE], [n - 1, n - 2], [G.NONE], [3, 4, 5, 1 << 31], [7, 8, 9]]
    c["bad-cells"] = G.list_case(17, 33, bad, 8)
    c["bad-cell-beyond-the-stride"] = G.list_case(17, 33, [[1, 2, 3, n + 7], [4, 5, 6, 7]], 8, stride=3)  # only the first m entries count
    c["route-statuses"] = G.list_case(17, 33, [[1, 2, 3]] * 6 + [[n]] * 2, 8, status=[0, 1, 2, 3, 4, 77, 0, 2], path_len=[3, 3, 3, 3, 3, 3, 1, 1])
    c["zero-lengths"] = G.list_case(17, 33, [[1, 2, 3], [4, 5, 6]], 8, path_len=[0, 3])
    edges = [[0 * 33 + b for b in range(33)], [16 * 33 + b for b in range(32, -1, -1)], [a * 33 for a in range(17)], [a * 33 + 32 for a in range(16, -1, -1)],
             [a * 33 + a for a in range(17)], [a * 33 + 32 - a for a in range(17)]]
    for look in (2, 8, 255):
        c[f"edges-and-corners-look{look}"] = G.list_case(17, 33, edges, look, max_way=40)
    return c


NAMES = tuple(cases())
SMALL = tuple(k for k in NAMES if k not in ("paths-4096",))


@functools.lru_cache(maxsize=None)
def want(name):
    r = G.waypoints_np(*cases()[name], fill=SENT)
    for a in r[:5]:
        a.setflags(write=False)
    return r


# ===================================================================================================== CPU
def test_the_two_routes_of_the_restatement_agree_on_every_committed_input():
    for name in NAMES:
        case = cases()[name]
        if name == "paths-4096":
            case = case._replace(path=case.path[:300], path_len=case.path_len[:300], path_status=case.path_status[:300])
            assert G.same(G.waypoints_np(*case, fill=SENT), G.waypoints_py(*case, fill=SENT)), name
        elif name == "serpentine-look255" or name.startswith("route-8192x3"):
            continue  # the loops would take minutes; max_look 255 and 8192 x 3 are compared on the other cases
        else:
            assert G.same(want(name), G.waypoints_py(*case, fill=SENT)), name
    for name in ("route-8192x3-open-look255",):  # its first path alone through the loops
        case = cases()[name]
        case = case._replace(path=case.path[:1], path_len=case.path_len[:1], path_status=case.path_status[:1])
        assert G.same(G.waypoints_np(*case), G.waypoints_py(*case)), name


def test_the_committed_inputs_are_what_the_kernels_paths_need():
    """Conditions on the inputs, asserted on the restatement alone."""
    c = cases()
    w = want("serpentine")
    assert 600 <= int(c["serpentine"].path_len[0]) <= 800 and c["serpentine"].path_status[0] == R.OK and w.way_status[0] == G.FULL
    assert int(want("serpentine-max_way-w").way_status[0]) == 0 and int(want("serpentine-max_way-w-1").way_status[0]) == G.FULL
    assert want("serpentine-look255").counts[6] > 8 * 8 * 2  # segments longer than any at max_look 8
    statuses = set()
    for name in NAMES:
        if c[name].path_status is not None:
            statuses |= set(c[name].path_status.tolist())
    assert statuses >= {R.OK, R.TRUNCATED, R.UNREACHED, R.OUT_OF_GRID, R.NOT_CONVERGED}
    ws = set()
    for name in NAMES:
        ws |= set(want(name).way_status.tolist())
    assert ws == {0, 1, 2, 3, 4, 5}
    assert want("foreign").counts[4] > 0 and want("dist2").counts[4] > 0 and want("min_dist2-without-dist2").counts[4] == 0
    assert want("stride-below-len").counts[0] > 4 and (want("stride-below-len").way_status == G.PATH_TRUNCATED).sum() > 4
    assert want("bad-cells").way_status.tolist() == [5, 5, 0, 5, 5, 0] and want("bad-cell-beyond-the-stride").way_status.tolist() == [1, 1]
    assert want("route-statuses").way_status.tolist() == [0, 0, 4, 4, 4, 4, 5, 4] and want("zero-lengths").way_status.tolist() == [4, 0]
    assert want("one-cell").way_len.tolist() == [1, 2, 2] and want("one-cell-closed").counts[4] == 2  # a closed V forces every step
    assert want("straight-1x40").way_len.tolist() == [1, 2, 2, 2, 2, 3] * 2 and want("straight-1x40").counts[4] == 0
    assert want("paths-4096").counts[0] > 3000 and want("paths-65").counts[0] + want("paths-65").counts[1] == 65
    assert want("route-8192x3-open-look255").counts[6] >= 200 * 200
    # the largest clear j is past a failure somewhere: the two readings differ on a random case
    assert not G.same(G.waypoints_np(*c["route"], variant="first_failure"), G.waypoints_np(*c["route"]))
    # a waypoint within max_look of every edge and corner
    e = want("edges-and-corners-look255")
    assert e.counts[4] == 0 and e.way_len.tolist() == [2, 2, 2, 2, 2, 2]


def test_every_misreading_of_the_contract_differs_on_a_committed_input():
    inputs = G.misreading_cases()
    right = {k: G.waypoints_np(*v) for k, v in inputs.items()}
    for variant in G.VARIANTS:
        where = [k for k, v in inputs.items() if not G.same(G.waypoints_np(*v, variant=variant), right[k])]
        print(variant, where)
        assert where, variant


def test_no_step_of_a_route_made_path_is_forced_without_a_min_dist2():
    n = 0
    for name, case in cases().items():
        if name.startswith(("route", "serpentine", "paths-", "stride-", "short_way", "no-status")) and case.prm.min_dist2 == 0:
            assert want(name).counts[4] == 0, name
            n += 1
    assert n >= 25


def _api_params(prm):
    from stereo_vo_amd import api
    return api.GridWaypointParams(*prm)


def test_pure_entries_and_refusals_without_a_context():
    from stereo_vo_amd import api
    L = api.lib()
    g = api.voxel_grid_default_params(0.1)
    cp = api.grid_clearance_default_params(g, 0.1)
    rp = api.grid_route_default_params(cp)
    d = api.grid_waypoints_default_params(rp, cp)
    assert (d.na, d.nb, d.path_stride, d.max_look, d.min_dist2, d.max_way, d.cell_size) == (256, 256, 4096, 64, 0, 256, cp.cell_size)
    rp.na, rp.nb, rp.max_path = 17, 300, 1 << 20
    cp.cell_size = 0.125
    d = api.grid_waypoints_default_params(rp, cp)
    assert (d.na, d.nb, d.path_stride, d.cell_size) == (17, 300, 1 << 20, 0.125)
    for field, value in (("na", 0), ("nb", 8193), ("na", 8192), ("max_path", 0), ("max_path", (1 << 20) + 1)):  # 8192 x 2049 is beyond 2^24
        bad = api.GridRouteParams(17, 2049, 0, 0, 1, 1, 64, 0)
        setattr(bad, field, value)
        with pytest.raises(api.SvoError):
            api.grid_waypoints_default_params(bad, cp)
    for size in (0.0, -1.0, float("inf"), float("nan")):
        bad = api.GridClearanceParams(17, 2049, 4, 64, size, 0.0)
        with pytest.raises(api.SvoError):
            api.grid_waypoints_default_params(rp, bad)
    assert L.svo_grid_waypoints_default_params(None, C.byref(cp), C.byref(d)) == -1
    assert L.svo_grid_waypoints_default_params(C.byref(rp), None, C.byref(d)) == -1
    assert L.svo_grid_waypoints_default_params(C.byref(rp), C.byref(cp), None) == -1
    assert C.sizeof(api.GridWaypointParams) == 32 and C.sizeof(api.GridWaypointOut) == 40
    assert len(api.GRID_WAY_COUNTS) == 7 and api.GRID_WAY_MAX_PATHS == 4096
    assert (api.GRID_WAY_OK, api.GRID_WAY_PATH_TRUNCATED, api.GRID_WAY_FULL, api.GRID_WAY_SKIPPED, api.GRID_WAY_BAD_CELL) == (G.OK, G.PATH_TRUNCATED, G.FULL, G.SKIPPED, G.BAD_CELL)
    # a null context is refused by every entry before anything else is looked at
    buf = (C.c_double * 12)()
    out = api.GridWaypointOut(C.addressof(buf), None, C.addressof(buf))
    assert L.svo_grid_waypoints_dev(None, buf, None, buf, buf, None, 1, C.byref(d), C.byref(out), None) == -1
    assert L.svo_grid_waypoints(None, buf, None, buf, buf, None, 1, C.byref(d), C.byref(out), None) == -1
    assert L.svo_grid_waypoints_dev(None, None, None, None, None, None, 0, None, None, None) == -1


def test_grid_waypoints_args_every_refusal_the_line_and_clear(tmp_path):
    """host/waypoint_args.h on the CPU under ASan + UBSan: every refusal at its boundary with code and exact message, the order of the
    refusals, the line stepper against the closed formula for every (da, db) with |d| <= 255, CLEAR on hand-made corners, the
    defaults."""
    _run_sanitized(tmp_path, "grid_waypoints_args_test", "grid waypoints args ok")


# ===================================================================================================== GPU
_SENT = {"way": (np.int32, SENT), "way_index": (np.int32, SENT), "way_len": (np.int32, 0x77771111), "way_status": (np.uint8, 0xEE),
         "length": (np.int64, 0x5A5A5A5A5A5A5A5A)}


class _Dev:
    """A case's device buffers: the inputs between guard elements, sentinel-filled outputs with a guard element before and behind each.
    skip: of OUTPUTS, the outputs passed as NULL."""

    def __init__(self, case, skip=(), counts=True):
        import torch
        self.case, self.prm, self.skip, self.counts = case, case.prm, tuple(skip), counts
        self.np = len(case.path_len)

        def guarded(a, t, guard):
            d = torch.full((a.size + 2,), guard, dtype=t, device="cuda")
            d[1:-1] = torch.from_numpy(np.ascontiguousarray(a).ravel()).cuda()
            return d

        # a guard read as a cell would be passable and far, a guard read as a path entry would be cell 0
        self.blocked = guarded(case.blocked, torch.uint8, 0)
        self.dist2 = None if case.dist2 is None else guarded(case.dist2.view(np.int32), torch.int32, -1)
        self.path = guarded(case.path.view(np.int32), torch.int32, 0)
        self.path_len = guarded(case.path_len.view(np.int32), torch.int32, 0)
        self.path_status = None if case.path_status is None else guarded(case.path_status, torch.uint8, 0)
        sizes = {"way": self.np * self.prm.max_way, "way_index": self.np * self.prm.max_way, "way_len": self.np, "way_status": self.np, "length": self.np}
        self.bufs = {k: torch.full((sizes[k] + 2,), v, dtype=getattr(torch, np.dtype(t).name), device="cuda") for k, (t, v) in _SENT.items()}
        self.cnt = torch.full((10,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def ptrs(self):
        return {k: None if k in self.skip else b.data_ptr() + b.element_size() for k, b in self.bufs.items()}

    def call(self, ctx, **over):
        p = _api_params(self.prm._replace(**over))
        ptr = self.ptrs()
        out = ctx.grid_waypoints(self.blocked.data_ptr() + 1, self.path.data_ptr() + 4, self.path_len.data_ptr() + 4, self.np, p,
                                 dist2_ptr=None if self.dist2 is None else self.dist2.data_ptr() + 4,
                                 path_status_ptr=None if self.path_status is None else self.path_status.data_ptr() + 1,
                                 counts_ptr=self.cnt.data_ptr() + 8 if self.counts else None, **{k + "_ptr": v for k, v in ptr.items()})
        assert out["way"] == ptr["way"] and (out["n_paths"], out["max_way"]) == (self.np, p.max_way)
        ctx.sync()

    def read(self, keep=None):
        """{OUTPUTS..., "counts": the eight}, None for what was skipped"""
        case = self.case
        assert np.array_equal(self.blocked.cpu().numpy()[1:-1].reshape(case.blocked.shape), case.blocked)  # only read
        assert np.array_equal(self.path.cpu().numpy()[1:-1].view(np.uint32).reshape(case.path.shape), case.path)
        assert np.array_equal(self.path_len.cpu().numpy()[1:-1].view(np.uint32), case.path_len)
        got = {}
        for k, (t, v) in _SENT.items():
            a = self.bufs[k].cpu().numpy()
            assert a[0] == v and a[-1] == v, k  # nothing beside the outputs is written
            if k in self.skip:
                assert (a == v).all(), k
                got[k] = None
            else:
                got[k] = a[1:-1]
            if keep is not None:
                keep[k] = a.tobytes()
        c = self.cnt.cpu().numpy()
        assert c[0] == c[-1] == -1 and (self.counts or (c == -1).all())
        got["counts"] = tuple(int(v) for v in c[1:9]) if self.counts else None
        if keep is not None:
            keep["counts"] = c.tobytes()
        for k in ("way", "way_index"):
            if got[k] is not None:
                got[k] = got[k].view(np.uint32).reshape(self.np, self.prm.max_way)
        if got["way_len"] is not None:
            got["way_len"] = got["way_len"].view(np.uint32)
        if got["length"] is not None:
            got["length"] = got["length"].view(np.float64)
        return got


def _eq(got, w, what=""):
    if got["counts"] is not None:
        assert got["counts"] == tuple(w.counts) + (0,), (what, got["counts"], w.counts)
    for k in ("way_len", "way_status", "way_index", "way"):
        if got[k] is not None:
            x = getattr(w, k)
            assert np.array_equal(got[k], x), (what, k, int((got[k] != x).sum()), got[k].ravel()[:12], x.ravel()[:12])
    if got["length"] is not None:
        assert got["length"].tobytes() == w.length.tobytes(), (what, "length", got["length"][:6], w.length[:6])


def _run(ctx, case, how="dev", skip=(), counts=True, keep=None):
    if how == "host":
        from stereo_vo_amd import api
        r = ctx.grid_waypoints_host(case.blocked, case.path, case.path_len, _api_params(case.prm), dist2=case.dist2, path_status=case.path_status)
        assert tuple(r["counts"]) == api.GRID_WAY_COUNTS
        fill = lambda a: np.where(a == G.NONE, SENT, a).astype(np.uint32)  # the host entry's fill for the device tests'
        return {"way": fill(r["way"]), "way_index": fill(r["way_index"]), "way_len": r["way_len"], "way_status": r["way_status"], "length": r["length"],
                "counts": tuple(r["counts"].values()) + (0,)}
    d = _Dev(case, skip, counts)
    d.call(ctx)
    return d.read(keep)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_every_committed_input(ctx, name):
    got = _run(ctx, cases()[name])
    print(name, "counts", got["counts"])
    _eq(got, want(name), name)


@pytest.mark.gpu
def test_the_host_entry_against_the_device_entry(ctx):
    for name in ("route", "dist2", "foreign", "short_way", "bad-cells", "route-statuses", "no-status", "serpentine-max_way2", "one-cell", "paths-65"):
        case = cases()[name]
        host, dev = _run(ctx, case, "host"), _run(ctx, case)
        _eq(host, want(name), (name, "host"))
        _eq(dev, want(name), name)
        assert all(np.array_equal(host[k], dev[k]) for k in OUTPUTS[:4]) and host["length"].tobytes() == dev["length"].tobytes()
    # the caller's way comes back where nothing is written; single outputs; no counts
    from stereo_vo_amd import api
    case, w = cases()["bad-cells"], want("bad-cells")
    p = _api_params(case.prm)
    way = np.full(w.way.shape, 0x11112222, np.uint32)
    wlen = np.full(len(case.path_len), 0x77771111, np.uint32)
    assert ctx.L.svo_grid_waypoints(ctx.h, case.blocked.ctypes.data, None, case.path.ctypes.data, case.path_len.ctypes.data, None, len(case.path_len),
                                    C.byref(p), C.byref(api.GridWaypointOut(way.ctypes.data, None, wlen.ctypes.data, None, None)), None) == 0
    assert np.array_equal(way, np.where(w.way == SENT, 0x11112222, w.way)) and np.array_equal(wlen, w.way_len)
    length = np.full(len(case.path_len), -1.0)
    assert ctx.L.svo_grid_waypoints(ctx.h, case.blocked.ctypes.data, None, case.path.ctypes.data, case.path_len.ctypes.data, None, len(case.path_len),
                                    C.byref(p), C.byref(api.GridWaypointOut(None, None, None, None, length.ctypes.data)), None) == 0
    assert length.tobytes() == w.length.tobytes()


@pytest.mark.gpu
def test_optional_outputs_no_counts_and_a_repeated_call_byte_for_byte(ctx):
    case, w = cases()["foreign"], want("foreign")
    for skip in [("way_index",), ("way_status",), ("length",), ("way", "way_len"), ("way", "way_len", "way_index", "way_status"),
                 ("way", "way_len", "way_index", "length"), ("way_index", "way_status", "length")]:
        got = _run(ctx, case, skip=skip)
        assert all((got[k] is None) == (k in skip) for k in OUTPUTS)
        _eq(got, w, skip)
    _eq(_run(ctx, case, counts=False), w, "no counts")
    _eq(_run(ctx, case, skip=("way", "way_len", "way_index", "way_status"), counts=False), w, "length alone")
    # twice into the same buffers: the same bytes in every output
    for name in ("foreign", "serpentine", "serpentine-look255", "route-8192x3-open-look255", "paths-4096", "wild-lists-look255"):
        case, w = cases()[name], want(name)
        d = _Dev(case)
        first, second = {}, {}
        d.call(ctx)
        _eq(d.read(first), w, name)
        d.call(ctx)
        _eq(d.read(second), w, (name, "again"))
        assert first == second and set(first) == set(_SENT) | {"counts"}


@pytest.mark.gpu
def test_bad_calls_launch_nothing_and_leave_the_context_usable(ctx):
    from stereo_vo_amd import api
    L = ctx.L
    case, w = cases()["dist2"], want("dist2")
    good = case.prm
    d = _Dev(case)
    O = api.GridWaypointOut
    P = d.ptrs()
    full = lambda **kw: O(**{**P, **kw})
    A = dict(blocked=d.blocked.data_ptr() + 1, dist2=d.dist2.data_ptr() + 4, path=d.path.data_ptr() + 4, path_len=d.path_len.data_ptr() + 4,
             status=d.path_status.data_ptr() + 1, np=d.np, counts=d.cnt.data_ptr() + 8)

    def dev(prm=good, out=None, null_prm=False, null_out=False, **kw):
        a = {**A, **kw}
        o = out if out is not None else full()
        p = _api_params(prm)
        return L.svo_grid_waypoints_dev(ctx.h, a["blocked"], a["dist2"], a["path"], a["path_len"], a["status"], a["np"], None if null_prm else C.byref(p),
                                        None if null_out else C.byref(o), a["counts"])

    r = good._replace
    hlen = np.full(d.np, 0x77771111, np.uint32)
    hway = np.full((d.np, good.max_way), 0x11112222, np.uint32)

    def host(prm=good, blocked=case.blocked.ctypes.data, path=case.path.ctypes.data, path_len=case.path_len.ctypes.data, np_=d.np, out=None,
             null_out=False, null_prm=False):
        o = out if out is not None else O(hway.ctypes.data, None, hlen.ctypes.data, None, None)
        return L.svo_grid_waypoints(ctx.h, blocked, None, path, path_len, None, np_, None if null_prm else C.byref(_api_params(prm)),
                                    None if null_out else C.byref(o), None)

    none = O(None, None, None, None, None)
    calls = [(lambda: dev(blocked=None), "null blocked"), (lambda: dev(null_prm=True), "null params"), (lambda: dev(path=None), "grid_waypoints: null path"),
             (lambda: dev(path_len=None), "null path_len"), (lambda: dev(null_out=True), "null out"),
             (lambda: dev(r(na=0), path_len=None), "null path_len"),  # the nulls before the ranges
             (lambda: dev(r(na=0)), "na outside"), (lambda: dev(r(na=8193)), "na outside"), (lambda: dev(r(nb=0)), "nb outside"),
             (lambda: dev(r(nb=8193)), "nb outside"), (lambda: dev(r(na=8192, nb=2049)), "na * nb"),
             (lambda: dev(r(path_stride=0)), "path_stride"), (lambda: dev(r(path_stride=(1 << 20) + 1)), "path_stride"),
             (lambda: dev(r(max_look=0)), "max_look"), (lambda: dev(r(max_look=256)), "max_look"),
             (lambda: dev(r(min_dist2=(1 << 26) + 1)), "min_dist2"),
             (lambda: dev(r(max_way=0)), "max_way"), (lambda: dev(r(max_way=(1 << 20) + 1)), "max_way"),
             (lambda: dev(r(cell_size=0.0)), "cell_size"), (lambda: dev(r(cell_size=float("inf"))), "cell_size"),
             (lambda: dev(r(cell_size=float("nan"))), "cell_size"), (lambda: dev(r(cell_size=-1.0)), "cell_size"),
             (lambda: dev(np=0), "n_paths"), (lambda: dev(np=4097), "n_paths"), (lambda: dev(np=-1), "n_paths"),
             (lambda: dev(r(max_look=0, max_way=0)), "max_look"),  # in the order of the fields
             (lambda: dev(r(cell_size=0.0), np=0), "cell_size"),  # the fields before n_paths
             (lambda: dev(out=full(way=None)), "go together"), (lambda: dev(out=full(way_len=None)), "go together"),
             (lambda: dev(out=none), "every output is null"), (lambda: dev(out=none, np=0), "n_paths"),
             (lambda: dev(out=full(way=None), dist2=A["dist2"] + 2), "go together"),  # the outputs' rules before the alignments
             (lambda: dev(dist2=A["dist2"] + 2), "dist2 must be 4-byte"), (lambda: dev(path=A["path"] + 1), "path must be 4-byte"),
             (lambda: dev(path_len=A["path_len"] + 2), "path_len must be 4-byte"),
             (lambda: dev(out=full(way=P["way"] + 1)), "way must be 4-byte"), (lambda: dev(out=full(way_index=P["way_index"] + 2)), "way_index must be 4-byte"),
             (lambda: dev(out=full(way_len=P["way_len"] + 3)), "way_len must be 4-byte"),
             (lambda: dev(out=full(length=P["length"] + 4)), "length must be 8-byte"), (lambda: dev(counts=A["counts"] + 4), "counts must be 8-byte"),
             (lambda: dev(out=full(way_len=P["way_len"] + 2), counts=A["counts"] + 4), "way_len must be 4-byte"),  # the 4-byte ones first
             (lambda: host(blocked=None), "null blocked"), (lambda: host(null_prm=True), "null params"), (lambda: host(path=None), "grid_waypoints: null path"),
             (lambda: host(path_len=None), "null path_len"), (lambda: host(null_out=True), "null out"), (lambda: host(r(max_look=0)), "max_look"),
             (lambda: host(np_=4097), "n_paths"), (lambda: host(out=none), "every output is null"),
             (lambda: host(out=O(hway.ctypes.data, None, None, None, None)), "go together")]
    ctx.profile_select("grid_waypoints")
    for call, word in calls:
        assert call() == -1, word
        msg = L.svo_last_error(ctx.h).decode()
        assert msg == word if word.startswith("grid_waypoints:") else word in msg, (word, msg)
    assert ctx.profile_read()[1] == 0
    ctx.sync()
    for k, (t, v) in _SENT.items():
        assert (d.bufs[k].cpu().numpy() == v).all(), k
    assert (d.cnt.cpu().numpy() == -1).all() and (hlen == 0x77771111).all() and (hway == 0x11112222).all()
    # the boundaries' accepted sides in one call: one bracket
    assert dev(r(max_look=255, min_dist2=1 << 26, max_way=1, cell_size=1e300), status=None, counts=None, out=full(way_index=None, length=None)) == 0
    assert ctx.profile_read()[1] == 1
    ctx.profile_select(None)
    with pytest.raises(api.SvoError):
        ctx.grid_waypoints(A["blocked"], A["path"], A["path_len"], d.np, _api_params(good), way_ptr=P["way"])  # way without way_len
    with pytest.raises(api.SvoError):
        ctx.grid_waypoints_host(case.blocked, case.path, case.path_len, _api_params(good._replace(max_look=0)))
    with pytest.raises(api.SvoError):
        ctx.grid_waypoints_host(case.blocked, np.zeros((0, good.path_stride), np.uint32), np.zeros(0, np.uint32), _api_params(good))
    with pytest.raises(ValueError):
        ctx.grid_waypoints_host(case.blocked, case.path, case.path_len, _api_params(good._replace(na=5)))
    with pytest.raises(ValueError):
        ctx.grid_waypoints_host(case.blocked, case.path[:, :5], case.path_len, _api_params(good))
    with pytest.raises(ValueError):
        ctx.grid_waypoints_host(case.blocked, case.path, case.path_len, _api_params(good), dist2=case.dist2[:5])
    # the context is what it was, and gives the waypoints
    _eq(_run(ctx, case), w)
    _eq(_run(ctx, case, "host"), w)
