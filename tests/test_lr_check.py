"""Left-right check (include/svo.h "left-right check"): the numpy restatement's two routes against each other (CPU), and
the device's cost entry, batch entry and host entry against the restatement, compared with == everywhere (the contract depends on
no order).  The check is NOT idempotent (a removed pixel no longer votes): no test asserts that it is.

The scenes (tests/lr_check_ref.py) and what tests/lr_check_ref.py::branch_counts measured on them while the test was written:

  occlusion   96 x 192, noise background at d = 4, noise rectangle at d = 20, StereoBM(32, 9): 12,710 valid pixels; max_diff16 16
              removes 107 (62 saved by one consistent look-up, 142 vote collisions), max_diff16 0 removes 134.
  band        stereo_bm_ref.scene(96, 192, 32, 2), StereoBM(32, 9): 8,870 valid; 16 removes 419, 0 removes 450.  At 16: 529
              collisions, 59 columns won on equal cost (all 59 between different d: "ties go to the larger x" changes 79 pixels),
              21 pixels saved by an empty column, 93 by one consistent look-up, 130 values with fraction 8/16, 41 with 7/16, 500 with
              15/16, 5,035 with 0; the vote without rounding changes 23 pixels, FILTERED allowed to vote 7, `&&` -> `||` 114.
              `>` -> `>=` changes nothing at 16 on either image scene (no difference lands on the threshold: at_diff = 0), which
              is what the designed maps are for.
  designed    runs of values from a pool with every fraction the rules split on, negative values, pairs exactly 16 and 17 apart and
              shifts that leave the row; costs 0..3.  E.g. 256 x 37, seed 0, max_diff16 16: 8,846 valid, 699 removed, 699 saved by
              one look-up, 16 by an empty column, 731 by an out-of-range look-up, 740 dropped votes, 1,057 collisions, 237 ties,
              52 differences exactly 16 and 61 exactly 17, 2,564 negative values; `>=` changes 9 pixels.
  hand rows   nine rows of 3 to 6 pixels whose expected result is written out by hand.
  int32       one row of 3,100 on which an int16 difference wraps and keeps a pixel that int32 removes.
"""
import ctypes as C
import os

import numpy as np
import pytest

import lr_check_ref as R
import stereo_bm_ref as BM

gpu = pytest.mark.gpu

WIDTHS, HEIGHTS = (1, 2, 63, 64, 65, 255, 256, 257, 700, 1280), (1, 37)
ALL_BRANCHES = ("removed", "kept", "saved_by_one", "saved_by_empty", "saved_by_range", "collisions", "ties", "ties_matter", "dropped_votes",
                "at_diff", "over_by_one", "negative", "frac0", "frac7", "frac8", "frac15", "split_lookups")


def _build_scenes():
    """name -> dict(maps: three (disp, cost) of one shape, max_diff, expect: branch keys the FIRST map must reach)."""
    S = {}
    occ = R.image_maps(*R.occlusion_pair())
    occ2 = R.image_maps(*R.occlusion_pair(seed=8))
    band = R.image_maps(*R.band_pair())
    band2 = R.image_maps(*R.band_pair(seed=3))
    mirror = lambda m: (np.ascontiguousarray(m[0][:, ::-1]), np.ascontiguousarray(m[1][:, ::-1]))
    for md in (16, 0):
        S[f"occlusion_{md}"] = dict(maps=[occ, mirror(occ), occ2], max_diff=md,
                                    expect=("removed", "saved_by_one", "collisions", "split_lookups", "frac0", "frac15"))
        S[f"band_{md}"] = dict(maps=[band, mirror(band), band2], max_diff=md,
                               expect=("removed", "saved_by_one", "saved_by_empty", "collisions", "ties", "ties_matter", "frac0", "frac7", "frac8", "frac15"))
    for W in WIDTHS:
        for H in HEIGHTS:
            if W >= 63 and H == 37:
                expect = ALL_BRANCHES
            elif H == 37:
                expect = ("dropped_votes", "saved_by_range", "negative", "frac0", "frac7", "frac8", "frac15")
            else:
                expect = ("valid",)
            S[f"designed_{W}x{H}"] = dict(maps=[R.designed(W, H, s) for s in range(3)], max_diff=16, expect=expect)
    S["designed_257x37_diff0"] = dict(maps=[R.designed(257, 37, s) for s in range(3, 6)], max_diff=0, expect=("removed", "at_diff", "over_by_one"))
    S["designed_65x37_diff65535"] = dict(maps=[R.designed(65, 37, s) for s in range(3)], max_diff=65535, expect=("kept",))
    d, c, md = R.int32_row()
    S["int32"] = dict(maps=R.variants(d, c), max_diff=md, expect=("removed", "negative"))
    for name, drow, crow, md, _ in R.hand_rows():
        S["hand_" + name] = dict(maps=R.variants(np.array([drow], np.int16), np.array([crow], np.uint16)), max_diff=md, expect=("valid",))
    for s in S.values():
        for d, c in s["maps"]:
            d.setflags(write=False)
            c.setflags(write=False)
    return S


SCENES = _build_scenes()
NAMES = list(SCENES)
# the scene written for each mutation (every one of them must change its result)
MUTATIONS = {"tie_larger_x": "band_16", "either": "occlusion_16", "no_round": "band_16", "ge": "designed_256x37", "filtered_votes": "band_16"}
_WANT = {}


def _want(name, v):
    """(expected map, n_removed) of map v of the scene: computed once, shared, read-only."""
    if (name, v) not in _WANT:
        s = SCENES[name]
        out, n = R.check_arrays(*s["maps"][v], s["max_diff"])
        out.setflags(write=False)
        _WANT[name, v] = (out, n)
    return _WANT[name, v]


# ------------------------------------------------------------------------------------------------ CPU: the restatement
@pytest.mark.parametrize("name", NAMES)
def test_both_routes_agree(name):
    s = SCENES[name]
    for v, (d, c) in enumerate(s["maps"]):
        a, na = R.check_rows(d, c, s["max_diff"])
        b, nb = _want(name, v)
        assert np.array_equal(a, b) and na == nb == int((a != d).sum()), (name, v)
        assert ((a == d) | (a == R.FILTERED)).all()


@pytest.mark.parametrize("name", NAMES)
def test_scene_reaches_the_branches_it_is_for(name):
    s = SCENES[name]
    c = R.branch_counts(*s["maps"][0], s["max_diff"])
    print(name, c)
    assert c["removed"] == _want(name, 0)[1] and c["removed"] + c["kept"] == c["valid"]
    for k in s["expect"]:
        assert c[k] > 0, (name, k, c)


def test_the_image_scenes_have_the_recorded_counts():
    """The table of the docstring (band: the figures the contract was first tried on)."""
    for name, valid, removed in (("occlusion_16", 12710, 107), ("occlusion_0", 12710, 134), ("band_16", 8870, 419), ("band_0", 8870, 450)):
        d, _ = SCENES[name]["maps"][0]
        assert int((d != R.FILTERED).sum()) == valid and _want(name, 0)[1] == removed, name
    c = R.branch_counts(*SCENES["band_16"]["maps"][0], 16)
    assert (c["saved_by_empty"], c["frac8"], c["frac0"], c["at_diff"]) == (21, 130, 5035, 0)
    assert R.branch_counts(*SCENES["occlusion_16"]["maps"][0], 16)["at_diff"] == 0


@pytest.mark.parametrize("name,drow,crow,md,want", R.hand_rows(), ids=[r[0] for r in R.hand_rows()])
def test_hand_rows(name, drow, crow, md, want):
    d, c = np.array([drow], np.int16), np.array([crow], np.uint16)
    assert R.check_rows(d, c, md)[0][0].tolist() == want
    assert R.check_arrays(d, c, md)[0][0].tolist() == want


def test_hand_rows_turn_on_the_rule_they_are_for():
    rows = {r[0]: r for r in R.hand_rows()}

    def run(name, **mut):
        _, drow, crow, md, _ = rows[name]
        return R.check_arrays(np.array([drow], np.int16), np.array([crow], np.uint16), md, **mut)[0][0].tolist()

    F = R.FILTERED
    assert run("diff_at_max", ge=True) == [F, F, F, 16, F, F]           # a difference exactly at max_diff16 stays only under `>`
    assert run("tie_smaller_x", tie_larger_x=True) == [F, F, F, F, 32, F]
    assert run("empty_saves", filtered_votes=True) != run("empty_saves")  # x=0 (FILTERED) would vote column 1 and fill it
    assert run("diff_17_both", either=True) == run("diff_17_both")      # both bad: `||` changes nothing here


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_a_mutated_restatement_fails(mutation):
    """Ties to the larger x, `&&` -> `||`, no rounding in the vote, `>` -> `>=`, FILTERED allowed to vote: each changes the result of
    the scene written for it, by both routes alike (so the agreement test and every device test would fail on a check with that
    mistake)."""
    name = MUTATIONS[mutation]
    s = SCENES[name]
    d, c = s["maps"][0]
    a, _ = R.check_rows(d, c, s["max_diff"], **{mutation: True})
    b, _ = R.check_arrays(d, c, s["max_diff"], **{mutation: True})
    assert np.array_equal(a, b)
    assert not np.array_equal(a, _want(name, 0)[0]), mutation
    changed = [n for n in NAMES if not np.array_equal(R.check_arrays(*SCENES[n]["maps"][0], SCENES[n]["max_diff"], **{mutation: True})[0], _want(n, 0)[0])]
    print(mutation, "changes", int((a != _want(name, 0)[0]).sum()), "pixels of", name, "and", len(changed), "scenes")
    assert len(changed) >= 2


def test_int32_differences():
    d, c, md = R.int32_row()
    out, n = R.check_arrays(d, c, md)
    assert n == 1 and out[0, 3047] == R.FILTERED and out[0, 0] == -16000
    wrapped = int(np.int16(np.int32(-16000) - np.int32(32752) + 65536))
    assert abs(wrapped) <= md < 48752  # what an int16 difference would have compared


def test_min_sad_marks_exactly_the_filtered_pixels():
    for L, Rr in (R.occlusion_pair(), R.band_pair()):
        m, c = R.image_maps(L, Rr)
        assert ((c == R.NO_COST) == (m == R.FILTERED)).all() and c[c != R.NO_COST].max() <= R.IMAGE_BLOCK ** 2 * 62
        assert (m != R.FILTERED).sum() > 8000


def test_abi():
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    L = S.lib()
    names = ["svo_stereo_bm_cost_batch_dev", "svo_disparity_lr_check_batch_dev", "svo_disparity_lr_check",
             "svo_pipeline_set_keyframe_lr_check", "svo_pipeline_group_set_keyframe_lr_check"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svo.h")).read()
    for n in names:
        assert n in api.SYMBOLS and n + "(" in header, n
        f = getattr(L, n)
        assert f.argtypes is not None and f.restype is C.c_int, n
    assert len(L.svo_stereo_bm_cost_batch_dev.argtypes) == 12 and len(L.svo_disparity_lr_check_batch_dev.argtypes) == 8
    assert len(L.svo_disparity_lr_check.argtypes) == 7
    assert C.sizeof(api.LrCheckParams) == 4 and [f[0] for f in api.LrCheckParams._fields_] == ["max_diff16"]
    assert "typedef struct svo_lr_check_params" in header and f"#define SVO_LR_CHECK_MAX_WIDTH {api.LR_CHECK_MAX_WIDTH}\n" in header
    assert api.LR_CHECK_MAX_WIDTH >= 1280 and 6 * api.LR_CHECK_MAX_WIDTH <= 64 * 1024  # needs no dynamic-LDS grant
    assert '"lr_check"' in header
    for w in ("Context.stereo_bm_cost_batch", "Context.lr_check", "Context.lr_check_dev", "Pipeline.set_keyframe_lr_check",
              "PipelineGroup.set_keyframe_lr_check"):
        cls, meth = w.split(".")
        assert callable(getattr(getattr(api, cls), meth)), w


# ------------------------------------------------------------------------------------------------ GPU
GUARD = 4096  # bytes behind every output that must stay as they were


def _device_check(ctx, torch, disps, costs, max_diff, want_removed=True):
    """The batch entry on (B, H, W) maps -> (checked maps, n_removed or None); checks the guard bands and that the costs are not
    written."""
    from stereo_vo_amd import api
    B, H, W = disps.shape
    n = B * H * W
    buf = np.full(n + GUARD // 2, 0x5A5A, np.uint16).view(np.int16)
    buf[:n] = disps.reshape(-1)
    dm = torch.from_numpy(buf).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(costs).view(np.int16).reshape(-1).copy()).cuda()
    dn = torch.full((B + 8,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.lr_check_dev(dm.data_ptr(), dc.data_ptr(), B, W, H, api.LrCheckParams(max_diff), dn.data_ptr() if want_removed else None)
    ctx.sync()
    got = dm.cpu().numpy()
    assert (got[n:].view(np.uint16) == 0x5A5A).all(), "bytes behind the maps changed"
    assert np.array_equal(dc.cpu().numpy().view(np.uint16), np.ascontiguousarray(costs).reshape(-1)), "the costs changed"
    nr = dn.cpu().numpy()
    assert (nr[B:] == -7).all()
    if not want_removed:
        assert (nr == -7).all()
    return got[:n].reshape(B, H, W), (nr[:B] if want_removed else None)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_batch_entry_equals_the_restatement(ctx, name):
    """Batch 3 of different maps per scene."""
    import torch
    s = SCENES[name]
    disps, costs = np.stack([m[0] for m in s["maps"]]), np.stack([m[1] for m in s["maps"]])
    got, n = _device_check(ctx, torch, disps, costs, s["max_diff"])
    for v in range(3):
        want, nw = _want(name, v)
        print(name, "map", v, "differing pixels", int((got[v] != want).sum()), "removed", nw, int(n[v]))
        assert np.array_equal(got[v], want), (name, v, int((got[v] != want).sum()))
        assert n[v] == nw, (name, v)


@gpu
@pytest.mark.parametrize("name", ["band_16", "designed_257x37", "designed_1x1"])
def test_batch_entry_with_null_n_removed_and_batch_1(ctx, name):
    import torch
    s = SCENES[name]
    d, c = s["maps"][0]
    got, n = _device_check(ctx, torch, d[None].copy(), c[None].copy(), s["max_diff"], want_removed=False)
    assert n is None and np.array_equal(got[0], _want(name, 0)[0])


@gpu
@pytest.mark.parametrize("name", ["occlusion_16", "band_0", "designed_1280x37", "designed_2x1", "designed_65x37_diff65535", "int32", "hand_negative_wins"])
def test_host_form_equals_the_restatement_and_leaves_its_input(ctx, name):
    s = SCENES[name]
    d, c = s["maps"][0]
    want, nw = _want(name, 0)
    src, cst = d.copy(), c.copy()
    got, n = ctx.lr_check(src, cst, s["max_diff"])
    assert np.array_equal(src, d) and np.array_equal(cst, c)
    assert np.array_equal(got, want) and n == nw, (name, int((got != want).sum()), n, nw)


_PAIRS = {}


def _cost_case(w, h, ndisp, block):
    """Three pairs (a band scene, its left-right mirror, another seed) and the restatement's (map, cost) of each, once per session."""
    key = (w, h, ndisp, block)
    if key not in _PAIRS:
        a, b = BM.scene(h, w, ndisp, 2), BM.scene(h, w, ndisp, 3)
        pairs = [a, (np.ascontiguousarray(a[0][:, ::-1]), np.ascontiguousarray(a[1][:, ::-1])), b]
        ref = [(BM.stereo_bm(L, Rr, ndisp, block), R.min_sad(L, Rr, ndisp, block)) for L, Rr in pairs]
        for m, c in ref:
            m.setflags(write=False)
            c.setflags(write=False)
        _PAIRS[key] = (pairs, ref)
    return _PAIRS[key]


def _device_cost(ctx, torch, pairs, ndisp, block):
    """svo_stereo_bm_cost_batch_dev on the pairs -> (maps, costs) (B, H, W); guard bands behind both outputs."""
    B = len(pairs)
    h, w = pairs[0][0].shape
    n = B * h * w
    dl = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    dr = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    dm = torch.from_numpy(np.full(n + GUARD // 2, 0x5A5A, np.uint16).view(np.int16)).cuda()
    dc = torch.from_numpy(np.full(n + GUARD // 2, 0x3C3C, np.uint16).view(np.int16)).cuda()
    torch.cuda.synchronize()
    ctx.stereo_bm_cost_batch(dl.data_ptr(), dr.data_ptr(), B, w, h, w, w * h, dm.data_ptr(), dc.data_ptr(), ndisp, block)
    ctx.sync()
    m, c = dm.cpu().numpy(), dc.cpu().numpy().view(np.uint16)
    assert (m[n:].view(np.uint16) == 0x5A5A).all() and (c[n:] == 0x3C3C).all(), "bytes behind an output changed"
    plain = torch.zeros(n, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.stereo_bm_batch(dl.data_ptr(), dr.data_ptr(), B, w, h, w, w * h, plain.data_ptr(), ndisp, block)
    ctx.sync()
    assert m[:n].tobytes() == plain.cpu().numpy().tobytes(), "the cost form's map differs from svo_stereo_bm_batch_dev's"
    return m[:n].reshape(B, h, w), c[:n].reshape(B, h, w)


@gpu
@pytest.mark.parametrize("w,h,ndisp,block", [(192, 96, 32, 9), (131, 61, 16, 5), (496, 160, 48, 21)])
def test_cost_entry_equals_the_restatement(ctx, w, h, ndisp, block):
    import torch
    pairs, ref = _cost_case(w, h, ndisp, block)
    maps, costs = _device_cost(ctx, torch, pairs, ndisp, block)
    for v, (m, c) in enumerate(ref):
        print((w, h, ndisp, block), v, "map differs at", int((maps[v] != m).sum()), "cost differs at", int((costs[v] != c).sum()), "valid", int((m != R.FILTERED).sum()))
        assert np.array_equal(maps[v], m), v
        assert np.array_equal(costs[v], c), v
        assert ((costs[v] == R.NO_COST) == (maps[v] == R.FILTERED)).all() and (m != R.FILTERED).sum() >= 100


@gpu
@pytest.mark.parametrize("max_diff", [16, 0])
def test_chain_cost_entry_then_check(ctx, max_diff):
    """The check run on the device's own (map, cost) equals the restatement run on the reference's (map, cost)."""
    import torch
    pairs, ref = _cost_case(192, 96, 32, 9)
    maps, costs = _device_cost(ctx, torch, pairs, 32, 9)
    got, n = _device_check(ctx, torch, maps, costs, max_diff)
    for v, (m, c) in enumerate(ref):
        want, nw = R.check_arrays(m, c, max_diff)
        assert nw >= 100 and np.array_equal(got[v], want) and n[v] == nw, (v, nw, int(n[v]))


@gpu
def test_one_bracket_per_call(ctx):
    import torch
    s = SCENES["designed_65x37"]
    disps, costs = np.stack([m[0] for m in s["maps"]]), np.stack([m[1] for m in s["maps"]])
    ctx.profile_select("lr_check")
    _device_check(ctx, torch, disps, costs, 16)
    ctx.lr_check(disps[0], costs[0], 16)
    launches = ctx.profile_read()[1]
    ctx.profile_select(None)
    assert launches == 2


@gpu
def test_bad_arguments_are_refused_without_a_launch(ctx):
    import torch
    from stereo_vo_amd import api
    s = SCENES["designed_65x37"]
    d0, c0 = s["maps"][0]
    H, W = d0.shape
    dm = torch.from_numpy(d0.copy()).cuda()
    dc = torch.from_numpy(c0.view(np.int16).copy()).cuda()
    dn = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    img = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    Lb, m, c, n, im = ctx.L, dm.data_ptr(), dc.data_ptr(), dn.data_ptr(), img.data_ptr()
    ok = C.byref(api.LrCheckParams(16))
    host, hcost = d0.copy(), c0.copy()
    hp, hc = host.ctypes.data_as(C.c_void_p), hcost.ctypes.data_as(C.c_void_p)
    wide = api.LR_CHECK_MAX_WIDTH + 1
    cases = {
        "max_diff16": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, c, 1, W, H, C.byref(api.LrCheckParams(-1)), n),
        "disp16": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, None, c, 1, W, H, ok, n),
        "cost16": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, None, 1, W, H, ok, n),
        "params": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, c, 1, W, H, None, n),
        "batch": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, c, 0, W, H, ok, n),
        "batch ": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, c, 65536, W, H, ok, n),
        "width": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, c, 1, 0, H, ok, n),
        "height": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, c, 1, W, 0, ok, n),
        "height ": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, c, 1, W, -3, ok, n),
        "SVO_LR_CHECK_MAX_WIDTH": lambda: Lb.svo_disparity_lr_check_batch_dev(ctx.h, m, c, 1, wide, 1, ok, n),
        "max_diff16 ": lambda: Lb.svo_disparity_lr_check(ctx.h, hp, hc, W, H, C.byref(api.LrCheckParams(-2)), None),
        "disp16 ": lambda: Lb.svo_disparity_lr_check(ctx.h, None, hc, W, H, ok, None),
        "cost16 ": lambda: Lb.svo_disparity_lr_check(ctx.h, hp, None, W, H, ok, None),
        "params ": lambda: Lb.svo_disparity_lr_check(ctx.h, hp, hc, W, H, None, None),
        "width ": lambda: Lb.svo_disparity_lr_check(ctx.h, hp, hc, 0, H, ok, None),
        "height  ": lambda: Lb.svo_disparity_lr_check(ctx.h, hp, hc, W, 0, ok, None),
        "SVO_LR_CHECK_MAX_WIDTH ": lambda: Lb.svo_disparity_lr_check(ctx.h, hp, hc, wide, 1, ok, None),
    }
    ctx.profile_select("lr_check")
    for word, call in cases.items():
        assert call() == -1, word
        assert word.strip() in Lb.svo_last_error(ctx.h).decode(), (word, Lb.svo_last_error(ctx.h))
    launches = ctx.profile_read()[1]
    ctx.profile_select("stereo_dense_batch")
    assert Lb.svo_stereo_bm_cost_batch_dev(ctx.h, im, im, 1, W, H, W, W * H, 16, 5, m, None) == -1
    assert "cost16" in Lb.svo_last_error(ctx.h).decode()
    assert Lb.svo_stereo_bm_cost_batch_dev(ctx.h, im, im, 1, W, H, W, W * H, 16, 5, None, c) == -1
    assert "disp16" in Lb.svo_last_error(ctx.h).decode()
    launches += ctx.profile_read()[1]
    ctx.profile_select(None)
    assert launches == 0
    assert np.array_equal(dm.cpu().numpy(), d0) and np.array_equal(dc.cpu().numpy().view(np.uint16), c0) and int(dn.cpu()[0]) == -7
    assert np.array_equal(host, d0) and np.array_equal(hcost, c0)
    # the context works afterwards
    got, nr = ctx.lr_check(d0, c0, 16)
    assert np.array_equal(got, _want("designed_65x37", 0)[0]) and nr == _want("designed_65x37", 0)[1]
