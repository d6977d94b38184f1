"""numpy restatement of the left-right check of include/svo.h ("left-right check"), by two routes that share no code,
the cost map it feeds on, and the scenes the tests use.

  check_rows   route (a): the contract as written, one row at a time, x ascending, plain Python integers.
  check_arrays route (b): whole-array: every vote packed as (cost << 32 | x) and reduced per right-view column with
               np.minimum.at, the look-ups by fancy indexing.
  min_sad      the winner's SAD per pixel of StereoBM (0xFFFF where the map is FILTERED), from stereo_bm_ref.prefilter and _box:
               independent of the kernels and of the oracle.

Both routes take the same mutation switches (each one mistake a device implementation could make); the tests require every
mutation to change the result of the scene written for it.  All of it is exact integer arithmetic: `==` is the comparison."""
import numpy as np

import stereo_bm_ref as BM

FILTERED = -16
NO_COST = 0xFFFF
MUTATIONS = ("tie_larger_x", "either", "no_round", "ge", "filtered_votes")


def _maps(disp, cost):
    d = np.asarray(disp)
    c = np.asarray(cost)
    assert d.dtype == np.int16 and c.dtype == np.uint16 and d.ndim == 2 and d.shape == c.shape
    return d, c


# ------------------------------------------------------------------------------------------------ route (a)
def _row_d2(drow, crow, tie_larger_x=False, no_round=False, filtered_votes=False):
    """-> (d2, c2, votes, at_best, dropped): per right-view column the winner's d (None: empty) and cost, the number of votes it got and
    how many of them carry the winning cost, and the number of votes of this row that fell outside the row."""
    W = len(drow)
    d2, c2, votes, at_best, dropped = [None] * W, [None] * W, [0] * W, [0] * W, 0
    for x in range(W):
        d, c = int(drow[x]), int(crow[x])
        if d == FILTERED and not filtered_votes:
            continue
        x2 = x - ((d + (0 if no_round else 8)) >> 4)
        if x2 < 0 or x2 >= W:
            dropped += 1
            continue
        votes[x2] += 1
        at_best[x2] = 1 if (d2[x2] is None or c2[x2] > c) else at_best[x2] + (c2[x2] == c)
        if d2[x2] is None or c2[x2] > c or (tie_larger_x and c2[x2] == c):
            d2[x2], c2[x2] = d, c
    return d2, c2, votes, at_best, dropped


def check_rows(disp, cost, max_diff, tie_larger_x=False, either=False, no_round=False, ge=False, filtered_votes=False):
    """-> (checked copy, n_removed)."""
    disp, cost = _maps(disp, cost)
    H, W = disp.shape
    out = disp.copy()
    for y in range(H):
        d2 = _row_d2(disp[y], cost[y], tie_larger_x, no_round, filtered_votes)[0]
        for x in range(W):
            d = int(disp[y, x])
            if d == FILTERED:
                continue
            bad = []
            for xq in (x - (d >> 4), x - ((d + 15) >> 4)):
                if xq < 0 or xq >= W or d2[xq] is None:
                    bad.append(False)
                else:
                    diff = abs(d2[xq] - d)
                    bad.append(diff >= max_diff if ge else diff > max_diff)
            if (bad[0] or bad[1]) if either else (bad[0] and bad[1]):
                out[y, x] = FILTERED
    return out, int((out != disp).sum())


# ------------------------------------------------------------------------------------------------ route (b)
def check_arrays(disp, cost, max_diff, tie_larger_x=False, either=False, no_round=False, ge=False, filtered_votes=False):
    """-> (checked copy, n_removed)."""
    disp, cost = _maps(disp, cost)
    H, W = disp.shape
    d = disp.astype(np.int64)
    xs = np.broadcast_to(np.arange(W, dtype=np.int64), (H, W))
    ys = np.broadcast_to(np.arange(H, dtype=np.int64)[:, None], (H, W))
    valid = d != FILTERED
    voter = np.ones_like(valid) if filtered_votes else valid
    x2 = xs - ((d + (0 if no_round else 8)) >> 4)
    voter = voter & (x2 >= 0) & (x2 < W)
    order = (W - 1 - xs) if tie_larger_x else xs              # the smaller packed key wins: the larger x under the mutation
    packed = (cost.astype(np.int64) << 32) | order
    empty = np.int64(1) << 62
    best = np.full(H * W, empty, np.int64)
    np.minimum.at(best, (ys * W + x2)[voter], packed[voter])
    best = best.reshape(H, W)
    has = best != empty
    wx = best & 0xFFFFFFFF
    if tie_larger_x:
        wx = W - 1 - wx
    d2 = np.where(has, np.take_along_axis(d, np.where(has, wx, 0), 1), 0)

    def bad(xq):
        inside = (xq >= 0) & (xq < W)
        q = np.clip(xq, 0, W - 1)
        diff = np.abs(np.take_along_axis(d2, q, 1) - d)
        return inside & np.take_along_axis(has, q, 1) & ((diff >= max_diff) if ge else (diff > max_diff))

    a, b = bad(xs - (d >> 4)), bad(xs - ((d + 15) >> 4))
    gone = valid & ((a | b) if either else (a & b))
    out = np.where(gone, FILTERED, disp).astype(np.int16)
    return out, int(gone.sum())


def branch_counts(disp, cost, max_diff):
    """How often each decision of the contract is taken (written a third way, on top of route (a)'s vote table only)."""
    disp, cost = _maps(disp, cost)
    H, W = disp.shape
    keys = ("valid", "removed", "kept", "saved_by_one", "saved_by_empty", "saved_by_range", "collisions", "ties", "ties_matter", "dropped_votes",
            "at_diff", "over_by_one", "negative", "frac0", "frac7", "frac8", "frac15", "split_lookups")
    c = dict.fromkeys(keys, 0)
    for y in range(H):
        d2, c2, votes, at_best, dropped = _row_d2(disp[y], cost[y])
        d2_last = _row_d2(disp[y], cost[y], tie_larger_x=True)[0]
        c["dropped_votes"] += dropped
        c["collisions"] += sum(v - 1 for v in votes if v > 1)
        c["ties"] += sum(n > 1 for n in at_best)                       # columns whose winning cost more than one vote carries
        c["ties_matter"] += sum(a != b for a, b in zip(d2, d2_last))   # ... and the tied votes differ in d
        for x in range(W):
            d = int(disp[y, x])
            if d == FILTERED:
                continue
            c["valid"] += 1
            c["negative"] += d < 0
            for f in (0, 7, 8, 15):
                c["frac%d" % f] += (d & 15) == f
            state = []
            xa, xb = x - (d >> 4), x - ((d + 15) >> 4)
            c["split_lookups"] += xa != xb
            for xq in (xa, xb):
                if xq < 0 or xq >= W:
                    state.append("range")
                elif d2[xq] is None:
                    state.append("empty")
                else:
                    diff = abs(d2[xq] - d)
                    c["at_diff"] += diff == max_diff
                    c["over_by_one"] += diff == max_diff + 1
                    state.append("bad" if diff > max_diff else "good")
            if state == ["bad", "bad"]:
                c["removed"] += 1
                continue
            c["kept"] += 1
            c["saved_by_one"] += sorted(state) == ["bad", "good"]
            c["saved_by_empty"] += "empty" in state and "good" not in state
            c["saved_by_range"] += "range" in state and "good" not in state and "empty" not in state
    return c


# ------------------------------------------------------------------------------------------------ the cost map
def min_sad(L, R, ndisp, block):
    """uint16 (H, W): the smallest SAD over the disparities where StereoBM(ndisp, block) keeps the pixel, 0xFFFF where its map is
    FILTERED (outside the valid rectangle, no texture, not unique)."""
    L, R = np.asarray(L, np.uint8), np.asarray(R, np.uint8)
    H, W = L.shape
    out = np.full((H, W), NO_COST, np.int64)
    x0, x1, y0, y1 = BM.valid_rect(H, W, ndisp, block)
    if x1 > x0 and y1 > y0:
        lp, rp = BM.prefilter(L).astype(np.int64), BM.prefilter(R).astype(np.int64)
        lc = lp[:, ndisp - 1:]
        best = None
        for d in range(ndisp):
            s = BM._box(np.abs(lc - rp[:, ndisp - 1 - d:W - d]), block)
            best = s if best is None else np.minimum(best, s)
        out[y0:y1, x0:x1] = best
    out[BM.stereo_bm(L, R, ndisp, block) == FILTERED] = NO_COST
    assert out.max() <= NO_COST
    return out.astype(np.uint16)


# ------------------------------------------------------------------------------------------------ scenes
IMAGE_NDISP, IMAGE_BLOCK = 32, 9


def occlusion_pair(h=96, w=192, seed=7):
    """(L, R): a noise background at disparity 4 and a noise rectangle in front of it at disparity 20: the 16 columns of
    background left of the rectangle are seen by the left camera only."""
    rng = np.random.default_rng(seed)
    T = rng.integers(0, 256, (h, w + 32)).astype(np.uint8)
    F = rng.integers(0, 256, (h // 2, w // 3)).astype(np.uint8)
    L, R = T[:, :w].copy(), T[:, 4:4 + w].copy()
    r0, c0 = h // 4, w // 2 - 10
    L[r0:r0 + F.shape[0], c0:c0 + F.shape[1]] = F
    R[r0:r0 + F.shape[0], c0 - 20:c0 - 20 + F.shape[1]] = F
    return L, R


def band_pair(h=96, w=192, seed=2):
    return BM.scene(h, w, IMAGE_NDISP, seed)


def image_maps(L, R):
    return BM.stereo_bm(L, R, IMAGE_NDISP, IMAGE_BLOCK), min_sad(L, R, IMAGE_NDISP, IMAGE_BLOCK)


# values a designed row draws from: every fraction the rounding rules split on (0, 7, 8, 15) at several integer parts, negative
# non-FILTERED values (-16 itself is FILTERED), pairs exactly 16 and 17 apart (32 / 48 / 49, 16 / 33, 0 / 16, -1 / 16), and shifts
# that leave a narrow row
POOL = (0, 7, 8, 15, 16, 23, 24, 31, 32, 33, 39, 40, 47, 48, 49, 64, -1, -8, -9, -15, -17, -24, -32, 160, 4000, -4000, FILTERED, FILTERED)


def designed(W, H, seed):
    """(disp16, cost16): runs of 1..12 equal values from POOL (so consistent stretches exist beside the conflicts), costs 0..3 (equal
    costs at nearly every collision), now and then 27,342 (the largest SAD) or 0xFFFF."""
    rng = np.random.default_rng(1000 * W + 10 * H + seed)
    disp = np.empty((H, W), np.int16)
    for y in range(H):
        x = 0
        while x < W:
            n = int(rng.integers(1, 13))
            disp[y, x:x + n] = POOL[int(rng.integers(len(POOL)))]
            x += n
    cost = rng.integers(0, 4, (H, W)).astype(np.uint16)
    r = rng.random((H, W))
    cost[r < 0.03] = 27342
    cost[r < 0.01] = NO_COST
    return disp, cost


def int32_row():
    """One row of 3,100: the pixel at x = 3047 with d = 32,752 looks column 1000 up, whose only vote is x = 0 with d = -16,000.
    |-16000 - 32752| = 48,752 > 20,000: removed; an int16 difference would wrap to 16,784 and keep it."""
    disp = np.full((1, 3100), FILTERED, np.int16)
    cost = np.full((1, 3100), NO_COST, np.uint16)
    disp[0, 0], cost[0, 0] = -16000, 5
    disp[0, 3047], cost[0, 3047] = 32752, 6
    return disp, cost, 20000


def hand_rows():
    """Rows small enough to work out by hand: [(name, disp row, cost row, max_diff, expected row)]."""
    F = FILTERED
    return [
        # x=3 (d=16, cost 3) and x=4 (d=32, cost 5) both vote column 2; 3 wins.  x=4 looks column 2 up twice: |16 - 32| = 16
        ("diff_at_max", [F, F, F, 16, 32, F], [9, 9, 9, 3, 5, 9], 16, [F, F, F, 16, 32, F]),
        ("diff_over_max", [F, F, F, 16, 32, F], [9, 9, 9, 3, 5, 9], 15, [F, F, F, 16, F, F]),
        # x=4, d=33: votes column 2 ((33+8)>>4 = 2) and loses to x=3 on cost; xa = 2 (d2 = 16), xb = 4 - 3 = 1 (d2 = 16 from x=2):
        # |16 - 33| = 17 twice
        ("diff_17_both", [F, F, 16, 16, 33, F], [9, 9, 1, 3, 5, 9], 16, [F, F, 16, 16, F, F]),
        # the same without the vote of x=2: column 1 is empty, which saves x=4
        ("empty_saves", [F, F, F, 16, 33, F], [9, 9, 9, 3, 5, 9], 16, [F, F, F, 16, 33, F]),
        # equal costs: x=3 (d=16) and x=4 (d=32) tie on column 2, the smaller x wins, so x=4 goes and x=3 stays
        ("tie_smaller_x", [F, F, F, 16, 32, F], [9, 9, 9, 4, 4, 9], 0, [F, F, F, 16, F, F]),
        # x=1, d=40 (2.5 px): votes column 1 - 3 = -2: dropped; xa = 1 - 2 = -1 and xb = 1 - 3 = -2 are out of range: kept
        ("out_of_range", [0, 40, 0], [1, 0, 1], 0, [0, 40, 0]),
        # x=2, d=24 (fraction 8): the vote rounds up to column 0, xa = 2 - 1 = 1, xb = 2 - 2 = 0.  Column 1 holds x=1 (d=0): bad;
        # column 0 holds x=0 (d=0, cost 0 < 7): bad as well -> removed.  Without rounding the vote would go to column 1
        ("fraction_8", [0, 0, 24, F], [0, 2, 7, 9], 16, [0, 0, F, F]),
        # negative, not FILTERED: x=0, d=-8 votes column 0 ((-8+8)>>4 = 0); xa = 0 - (-8>>4) = 1 (d2 = -8, the vote of x=1), xb = 0
        ("negative", [-8, -8, F], [3, 3, 9], 0, [-8, -8, F]),
        # x=0, d=-17: votes column 0 - ((-9)>>4) = 1 and wins it on cost; x=1 (d=0) finds d2[1] = -17: |−17 − 0| = 17 > 16 twice
        ("negative_wins", [-17, 0, F], [0, 5, 9], 16, [-17, F, F]),
    ]


def variants(disp, cost):
    """Three different maps from one: as it is, mirrored left-right, rows in reverse order with the costs of row y taken from row
    H-1-y mirrored (just another map)."""
    return [(disp, cost), (np.ascontiguousarray(disp[:, ::-1]), np.ascontiguousarray(cost[:, ::-1])),
            (np.ascontiguousarray(disp[::-1]), np.ascontiguousarray(cost[:, ::-1]))]
