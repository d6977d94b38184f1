"""Corner detection against an independent restatement (tests/corner_ref.py), on scenes that reach every branch of
csrc/corner.hip: the response maximum on each border line (it sets the threshold although a border pixel is never a candidate),
candidates on the ring next to the border, pairs of candidates at exactly min_distance (strict <, the f32-rounded square), groups of
equal responses cut by max_corners (raster-index-descending tie-break), dependency chains of several hundred links, both forms of
corner_select_kernel at their hand-over (n <= 12288), grid cells smaller than min_distance (12.5, 2.5, [1, 1.5)), every strip
geometry (60 / 62 columns, 48 rows, sides of 3 to 5), the strided batched device entry and the capacity answers.

Every comparison is ==.  Not covered: the raw-list overflow of the fused pass (status bit 8).  It needs more than W*H/4 recorded local
maxima and what is recorded depends on timing; no deterministic scene for it is known."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import corner_ref as CR
import oracle_lib as O

gpu = pytest.mark.gpu

CASES = CR.cases()
IDS = list(CASES)
RESPONSE_IDS = [c for c in IDS if c.startswith(("border-", "strips-"))]
DENSE_RANGE = {"dense-lds": (11800, 12288), "dense-global": (12289, 14000)}
# the capacity scene: per-pixel noise at the KITTI size, quality 0
CAP_SHAPE, CAP_SEED = (376, 1241), 41
SMALL_SHAPE, SMALL_SEED = (200, 200), 51   # for a context of its own with max_candidates 1024


@functools.lru_cache(maxsize=None)
def _ref(cid):
    img, maxc, q, md = CASES[cid]
    xy = CR.detect(img, maxc, q, md)
    xy.setflags(write=False)
    return xy


@functools.lru_cache(maxsize=None)
def _ref_response(cid):
    e = CR.response(CASES[cid][0])
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def _stats(cid):
    img, maxc, q, md = CASES[cid]
    return CR.counters(img, maxc, q, md, with_rounds=cid.startswith("chain-"))


def _same_list(got, want, what):
    if got.shape != want.shape or not np.array_equal(got, want):
        k = next((i for i in range(min(len(got), len(want))) if not np.array_equal(got[i], want[i])), min(len(got), len(want)))
        print(what, "lengths", len(got), len(want), "first difference at", k, got[k:k + 4].tolist(), want[k:k + 4].tolist())
    assert got.shape == want.shape and np.array_equal(got, want), what


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("cid", IDS)
def test_reference_equals_the_oracle(cid):
    """Two restatements of SURVEY A.1 by different routes (per-pixel loops, std::sort and a cell grid; whole-array operations, a
    lexicographic sort and a greedy scan against every accepted corner) give the same response bits and the same corner list.  The
    grid loses nothing even where its cell, rint(min_distance), is smaller than min_distance: integer coordinates in non-adjacent
    cells lie at least cell + 1 > min_distance apart."""
    img, maxc, q, md = CASES[cid]
    assert np.array_equal(_ref_response(cid).view(np.uint32), O.corner_response(img).view(np.uint32))
    _same_list(O.corner_detect(img, maxc, q, md), _ref(cid), cid)


def test_scenes_reach_every_decision():
    """Floors on the restatement's own counters (conditions on the inputs; the scenes were tuned on the restatement alone).

    Measured:
      border-top / bottom / left / right: maximum on the border line, 1.30 / 1.30 / 1.44 / 1.37 times the interior maximum; candidates
        13 / 14 / 14 / 13, of them on the ring next to the border 2 / 2 / 2 / 2; candidates that a maximum over the interior alone
        would add 4 / 4 / 5 / 3.
      lattice-pitch5 (187 candidates, all of one value): min_distance 5.0 -> 346 pairs at exactly 25, 187 accepted; 5.0001 -> 94;
        sqrt 50 -> 320 pairs at exactly 50 (offset (5, 5)), 94 accepted; max_corners 40 cuts inside the group at 5.0 and 7.5.
      lattice-sheared (offset (7, 1), 104 candidates of one value): sqrt 50 -> 185 pairs at exactly 50, 104 accepted; 7.08 -> 52;
        max_corners 25 cuts inside the group.
      lattice-sq41 (offset (5, 4), 117 candidates of one value): f32(sqrt 41)^2 = 41.0000012 rounds DOWN to 41.0f, 203 pairs at
        exactly 41, 117 accepted (an unrounded square would leave 56, as min_distance 6.4032 does); max_corners 30 cuts inside.
      chain-row: 131 candidates of 131 values, 66 accepted, 131 rounds.  chain-zigzag: 399 candidates (262 in two tie groups), 200
        accepted, 399 rounds.
      dense-lds 12,281 candidates (LDS form, 12 per thread, blocker indices up to 12,280); dense-global 13,232 (global form by count).
      cells: 1,045 candidates, 540 8-adjacent pairs (360 candidates tied); accepted 1,045 / 775 / 578 / 92 at 1.0 / 1.49 / 2.5 / 12.5.
      strips: 0 to 756 candidates per shape; the maximum is on the border at 9 of the 14 shapes.
    The 8 x 8-block noise of tests/test_corner.py, same counters: maximum on the border 0 of 6 inputs, tied candidates 0 (30 of 24,062 at
    376 x 1241), no cut inside a tie group, 5 to 10 rounds; pairs of candidates at exactly min_distance do occur in it (21 to 7,447).
    """
    for cid in IDS:
        print(cid, CASES[cid][0].shape, CASES[cid][1:], {k: v for k, v in _stats(cid).items() if v})
    for side in CR.BORDER_SIDES:
        st = _stats("border-" + side)
        assert st["max_on_border"] and st["lost_to_border_max"] >= 1 and st["ring_candidates"] >= 1 and st["candidates"] >= 8, (side, st)
    lat = {c: _stats(c) for c in IDS if c.startswith("lattice-")}
    for c in ("lattice-pitch5-0", "lattice-pitch5-2", "lattice-sheared-0", "lattice-sq41-0"):
        assert lat[c]["exact_pairs"] >= 50, (c, lat[c])
        assert c == "lattice-pitch5-2" or lat[c]["accepted"] == lat[c]["candidates"], (c, lat[c])   # at exactly the distance: both stay
    for c, strict in (("lattice-pitch5-1", "lattice-pitch5-0"), ("lattice-sheared-1", "lattice-sheared-0"), ("lattice-sq41-1", "lattice-sq41-0")):
        assert lat[c]["accepted"] <= 0.6 * lat[strict]["accepted"], (c, lat[c])      # just above the distance: every second blob goes
    assert lat["lattice-sq41-0"]["square_rounds_down"] and not lat["lattice-sheared-0"]["square_rounds_down"]
    for c, st in lat.items():
        assert st["tied"] >= 100, (c, st)
    for c in ("lattice-pitch5-3", "lattice-pitch5-4", "lattice-sheared-2", "lattice-sq41-2"):
        assert lat[c]["cut_in_tie"] and lat[c]["accepted"] == CASES[c][1], (c, lat[c])
    assert _stats("chain-zigzag")["rounds"] >= 300 and _stats("chain-row")["rounds"] >= 100   # a row of 790 columns holds 131 blobs
    assert _stats("chain-row")["tied"] == 0 and _stats("chain-zigzag")["tied"] >= 100
    for c in ("chain-row", "chain-zigzag"):
        assert abs(2 * _stats(c)["accepted"] - _stats(c)["candidates"]) <= 1                  # acceptance alternates along the chain
    for c, (lo, hi) in DENSE_RANGE.items():
        st = _stats(c)
        assert lo <= st["candidates"] <= hi and st["accepted_uncut"] <= 16384, (c, st)
    cells = [_stats("cells-%g" % md) for md in CR.CELLS_MD]
    assert cells[0]["adjacent_pairs"] >= 100 and cells[0]["accepted"] == cells[0]["candidates"]
    assert cells[0]["accepted"] > cells[1]["accepted"] > cells[2]["accepted"] > cells[3]["accepted"] > 0
    assert sum(_stats("strips-%dx%d" % s)["max_on_border"] for s in CR.STRIPS) >= 3
    assert sum(_stats("strips-%dx%d" % s)["candidates"] > 0 for s in CR.STRIPS) >= 10


def test_capacity_scene_accepts_more_than_the_select_kernel_holds():
    """376 x 1241 per-pixel noise, quality 0: 30,840 candidates; at min_distance 2.0 the greedy scan accepts more than 16,384 (it
    is stopped there; the oracle accepts all 30,840, two strict local maxima are never 8-adjacent)."""
    img = CR.pixel_noise(*CAP_SHAPE, CAP_SEED)
    eig = CR.response(img)
    cand = CR.order(eig, CR.candidates(eig, 0.0))
    assert 16384 < len(cand) <= 1 << 17
    assert len(CR.select(cand, CAP_SHAPE[1], 2.0, 16385)) == 16385
    small = CR.response(CR.pixel_noise(*SMALL_SHAPE, SMALL_SEED))
    print("candidates of the small capacity scene", len(CR.candidates(small, 0.0)))
    assert len(CR.candidates(small, 0.0)) > 2 * 1024


# ------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("cid", IDS)
def test_detect_reaches_every_decision(ctx, cid):
    """svo_corner_detect: the fused response + non-maximum pass, the exact threshold and the select kernel."""
    img, maxc, q, md = CASES[cid]
    _same_list(ctx.corner_detect(img, maxc, q, md), _ref(cid), cid)


@gpu
@pytest.mark.parametrize("cid", RESPONSE_IDS)
def test_response_map_at_borders_and_strip_edges(ctx, cid):
    got = ctx.corner_response(CASES[cid][0])
    want = _ref_response(cid)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        ys, xs = np.nonzero(bad)
        print(cid, "differing pixels", int(bad.sum()), "rows", sorted(set(ys.tolist()))[:12], "columns", sorted(set(xs.tolist()))[:12])
    assert not bad.any()


@gpu
def test_two_pass_form_reaches_every_decision(tmp_path):
    """SVO_CORNER_TWO_PASS=1 (corner_response_kernel + corner_nms_kernel) on every case, in one fresh process: the flag is read once."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "two_pass.npz")
    e = dict(os.environ)
    e["SVO_CORNER_TWO_PASS"] = "1"
    run = subprocess.run([sys.executable, os.path.join(root, "tests", "_corner_two_pass_worker.py"), out], env=e, capture_output=True,
                         text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    with np.load(out) as res:
        assert sorted(res.files) == sorted(IDS)
        for cid in IDS:
            _same_list(res[cid], _ref(cid), "two-pass " + cid)


def _batch_sets():
    b = [CR.border_max(s)[0] for s in ("top", "left", "right")]
    n = [CR.pixel_noise(97, 121, s) for s in (51, 52, 53)]
    return [(np.stack(b), 64, 0.02, 4.0), (np.stack(n), 4096, 0.0, 2.0)]


@gpu
@pytest.mark.parametrize("k", [0, 1])
def test_batched_device_entry_strided(ctx, k):
    """svo_corner_detect_batch_dev: batch 3, row_stride = W + 5, image_stride = row_stride * H + 64, the gaps filled with noise."""
    import torch
    imgs, maxc, q, md = _batch_sets()[k]
    B, H, W = imgs.shape
    rs = W + 5
    ist = rs * H + 64
    buf = np.random.default_rng(7).integers(0, 256, B * ist, dtype=np.uint8)
    for b in range(B):
        buf[b * ist:b * ist + rs * H].reshape(H, rs)[:, :W] = imgs[b]
    d_img = torch.from_numpy(buf).cuda()
    d_xy = torch.full((B, maxc, 2), -7.0, dtype=torch.float32, device="cuda")
    d_n = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.corner_detect_batch_dev(d_img, B, W, H, rs, ist, maxc, q, md, d_xy, d_n)
    ctx.sync()
    xy, n = d_xy.cpu().numpy(), d_n.cpu().numpy()
    assert np.array_equal(d_img.cpu().numpy(), buf)              # the images and the bytes between them are unchanged
    for b in range(B):
        want = CR.detect(imgs[b], maxc, q, md)
        assert 3 <= len(want) and (k == 0 or len(want) > 500)
        _same_list(xy[b, :n[b]], want, "batch %d image %d" % (k, b))
        _same_list(ctx.corner_detect(imgs[b], maxc, q, md), want, "single image %d" % b)
        assert (xy[b, n[b]:] == -7.0).all()                      # nothing written behind the list


def _refused(ctx, what, img, maxc, q, md):
    import stereo_vo_amd as S
    with pytest.raises(S.api.SvoError) as err:
        ctx.corner_detect(img, maxc, q, md)
    assert "rc=-3" in str(err.value) and what in str(err.value), str(err.value)   # SVO_ERR_CAPACITY with its own message


def _still_right(ctx, ids=("lattice-pitch5-1", "strips-97x121")):
    for cid in ids:
        img, maxc, q, md = CASES[cid]
        _same_list(ctx.corner_detect(img, maxc, q, md), _ref(cid), "after a refusal: " + cid)


@gpu
def test_capacity_answers_and_the_context_afterwards(ctx):
    """Each bound answers SVO_ERR_CAPACITY with its own message and leaves the context usable.
    More than 16,384 accepted corners: in the rounds path (global form; min_distance 2.0 — at 1.0 the grid of this image, one cell
    per pixel, is itself larger than the workspace of a 1280 x 720 context and answers first) and in the top-K path (min_distance 0).
    A grid larger than the workspace: min_distance 1.0 at the context's full size, and on the KITTI-size noise."""
    noise = CR.pixel_noise(*CAP_SHAPE, CAP_SEED)
    _refused(ctx, "more accepted corners than the select kernel holds", noise, 4096, 0.0, 2.0)
    _still_right(ctx)
    _refused(ctx, "more accepted corners than the select kernel holds", noise, 4096, 0.0, 0.0)
    _still_right(ctx)
    _refused(ctx, "min-distance grid larger than the workspace", noise, 4096, 0.0, 1.0)
    _still_right(ctx)
    _refused(ctx, "min-distance grid larger than the workspace", CR.block_noise(720, 1280, 6), 4096, 0.01, 1.0)
    _still_right(ctx)


@gpu
def test_max_candidates_answer_on_a_small_context():
    """Status bit 1.  svo_create raises max_candidates to at least 1024; 200 x 200 per-pixel noise at quality 0 has 2,636 candidates."""
    import stereo_vo_amd as S
    c = S.Context(256, 256, max_candidates=1024)
    try:
        img = CR.pixel_noise(*SMALL_SHAPE, SMALL_SEED)
        for md in (2.0, 0.0):
            _refused(c, "more NMS candidates than svo_limits.max_candidates", img, 4096, 0.0, md)
            _still_right(c, ("lattice-pitch5-1", "lattice-sheared-0"))       # 187 and 104 candidates: within the bound
    finally:
        c.close()
