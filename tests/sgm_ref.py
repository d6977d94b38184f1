"""Restatement of the semi-global matching contract (include/svo.h, "semi-global matching"), two routes that share no
code.  Neither imports the oracle, neither follows the kernels (no lanes, no tiles, no shuffles).

  route (a)  whole arrays: stereo_bm_ref.prefilter, one |lp - rp| plane per disparity box-summed by stereo_bm_ref._box, then for
             each of the four paths ONE Python loop over the path's steps, vectorised over the other axis and over d; the
             selection is whole-array arithmetic.  `mutation` switches on one of five deliberate mistakes; `counts` receives how
             often each candidate of the min wins.
  route (b)  pixel by pixel in Python integers: its own prefilter, its own window sums, dictionaries of lists for the path costs
             and StereoBM's selection loop written out.  Small shapes only.

Disparities are indexed i = ndisp - 1 - d as StereoBM indexes its SADs (the first minimum in i is the largest d); the recursion is
symmetric in d, so d +- 1 is i -+ 1.  All arithmetic is exact (int64 / Python int): `==` is the comparison."""
import numpy as np

import stereo_bm_ref as BM

FILTERED = -16
NO_COST = 0xFFFF
MAX_P2 = 32767
MUTATIONS = ("d2", "one_neighbour", "no_m", "three_paths", "same_direction")
_BIG = 1 << 40


def default_params(block):
    return 2 * block * block, 8 * block * block


# ------------------------------------------------------------------------------------------------ route (a)
def cost_volume(L, R, ndisp, block):
    """-> (C int64 (vh, vw, ndisp), texture sums int64 (vh, vw)) over the valid rectangle, or None when it is empty."""
    L, R = np.asarray(L, np.uint8), np.asarray(R, np.uint8)
    H, W = L.shape
    x0, x1, y0, y1 = BM.valid_rect(H, W, ndisp, block)
    if x1 <= x0 or y1 <= y0:
        return None
    lp, rp = BM.prefilter(L).astype(np.int64), BM.prefilter(R).astype(np.int64)
    lc = lp[:, ndisp - 1:]
    C = np.empty((y1 - y0, x1 - x0, ndisp), np.int64)
    for d in range(ndisp):
        C[:, :, ndisp - 1 - d] = BM._box(np.abs(lc - rp[:, ndisp - 1 - d:W - d]), block)
    return C, BM._box(np.abs(lc - BM.CAP), block)


def _path(C, axis, backwards, p1, p2, mutation=None, counts=None):
    """L_r over the whole rectangle for the path that walks along `axis` (0: y, 1: x), from the far end when `backwards`."""
    A = np.moveaxis(C, axis, 0)
    if backwards:
        A = A[::-1]
    n, nd = A.shape[0], A.shape[2]
    Lr = np.empty_like(A)
    Lr[0] = A[0]
    k = 2 if mutation == "d2" else 1
    for t in range(1, n):
        q = Lr[t - 1]
        m = q.min(-1, keepdims=True)
        lo = np.full_like(q, _BIG)
        hi = np.full_like(q, _BIG)
        lo[:, k:] = q[:, :-k] + p1
        if mutation != "one_neighbour":
            hi[:, :-k] = q[:, k:] + p1
        adj = np.minimum(lo, hi)
        far = np.broadcast_to(m + p2, q.shape)
        best = np.minimum(np.minimum(q, adj), far)
        Lr[t] = A[t] + best - (0 if mutation == "no_m" else m)
        if counts is not None:
            same = q == best
            adjw = ~same & (adj == best)
            counts["same"] += int(same.sum())
            counts["adjacent"] += int(adjw.sum())
            counts["far"] += int((~same & ~adjw).sum())
            counts["same_ties_far"] += int((same & (far == best)).sum())
    if backwards:
        Lr = Lr[::-1]
    return np.moveaxis(Lr, 0, axis)


def aggregate(C, p1, p2, mutation=None, counts=None, l_max=None):
    """S = the sum of the four L_r, int64 (vh, vw, ndisp).  counts: dict that receives same / adjacent / far / same_ties_far; l_max: a
    one-element list that receives the largest L_r."""
    assert 0 <= p1 <= p2 <= MAX_P2
    if counts is not None:
        counts.update(same=0, adjacent=0, far=0, same_ties_far=0)
    plan = [(1, False), (1, True), (0, False), (0, True)]   # left->right, right->left, top->bottom, bottom->top
    if mutation == "three_paths":       # right->left is missing
        del plan[1]
    if mutation == "same_direction":    # both directions of each axis run forward
        plan = [(1, False), (1, False), (0, False), (0, False)]
    S = np.zeros_like(C)
    top = 0
    for axis, backwards in plan:
        Lr = _path(C, axis, backwards, p1, p2, mutation, counts)
        top = max(top, int(Lr.max()))
        S += Lr
    if l_max is not None:
        l_max[:] = [top]
    return S


def select(S, tsum):
    """StereoBM's selection with s := S -> (values int64 (vh, vw) with FILTERED, cost form int64 (vh, vw) with NO_COST)."""
    s = np.moveaxis(S, 2, 0)
    nd = s.shape[0]
    mind = s.argmin(0)                                                  # the first minimum in i = the largest d
    m = s.min(0)
    thresh = m + m * BM.UNIQUENESS_RATIO // 100                         # m >= 0
    far = np.abs(np.arange(nd)[:, None, None] - mind[None]) > 1
    rival = (far & (s <= thresh[None])).any(0)
    ext = np.concatenate([s[1:2], s, s[nd - 2:nd - 1]], 0)              # ext[i + 1] = s[i], mirrored ends
    p = np.take_along_axis(ext, (mind + 2)[None], 0)[0]
    n = np.take_along_axis(ext, mind[None], 0)[0]
    dd = p + n - 2 * m + np.abs(p - n)
    num = (p - n) * 256
    term = np.where(dd != 0, np.sign(num) * (np.abs(num) // np.maximum(dd, 1)), 0)   # truncated toward zero
    value = ((nd - mind - 1) * 256 + term + 15) >> 4
    kept = (tsum >= BM.TEXTURE_THRESHOLD) & ~rival
    return np.where(kept, value, FILTERED), np.where(kept, np.minimum((m + 2) >> 2, 0xFFFE), NO_COST)


def sgm(L, R, ndisp, block, p1=None, p2=None, mutation=None, counts=None, info=None):
    """-> (map int16 (H, W), cost uint16 (H, W)).  p1 / p2 None: the defaults.  info: dict that receives l_max and s_max."""
    L = np.asarray(L, np.uint8)
    H, W = L.shape
    d1, d2 = default_params(block)
    p1 = d1 if p1 is None else p1
    p2 = d2 if p2 is None else p2
    disp = np.full((H, W), FILTERED, np.int16)
    cost = np.full((H, W), NO_COST, np.uint16)
    vol = cost_volume(L, R, ndisp, block)
    if vol is None:
        if counts is not None:
            counts.update(same=0, adjacent=0, far=0, same_ties_far=0)
        return disp, cost
    top = []
    S = aggregate(vol[0], p1, p2, mutation, counts, top)
    if info is not None:
        info["l_max"], info["s_max"] = top[0], int(S.max())
    v, c = select(S, vol[1])
    x0, x1, y0, y1 = BM.valid_rect(H, W, ndisp, block)
    disp[y0:y1, x0:x1] = v
    cost[y0:y1, x0:x1] = c
    return disp, cost


# ------------------------------------------------------------------------------------------------ route (b)
def _pf_pixel(img, x, y):
    H, W = len(img), len(img[0])
    if x <= 0 or x >= W - 1 or ((H & 1) and y == H - 1):
        return 31
    ya = y - 1 if y - 1 >= 0 else (1 if H > 1 else 0)
    yb = y + 1 if y + 1 < H else (H - 2 if H > 1 else 0)
    v = (img[ya][x + 1] - img[ya][x - 1]) + 2 * (img[y][x + 1] - img[y][x - 1]) + (img[yb][x + 1] - img[yb][x - 1])
    return max(-31, min(31, v)) + 31


def sgm_pixels(L, R, ndisp, block, p1, p2):
    """The same function one pixel at a time, Python integers only -> (map, cost) as nested lists."""
    L = [[int(v) for v in row] for row in np.asarray(L)]
    R = [[int(v) for v in row] for row in np.asarray(R)]
    H, W = len(L), len(L[0])
    half = block // 2
    xs = list(range(ndisp - 1 + half, W - half))
    ys = list(range(half, H - half))
    disp = [[FILTERED] * W for _ in range(H)]
    cost = [[NO_COST] * W for _ in range(H)]
    if not xs or not ys:
        return disp, cost
    lp = [[_pf_pixel(L, x, y) for x in range(W)] for y in range(H)]
    rp = [[_pf_pixel(R, x, y) for x in range(W)] for y in range(H)]
    C, T = {}, {}
    for y in ys:
        for x in xs:
            win = [(xx, yy) for yy in range(y - half, y + half + 1) for xx in range(x - half, x + half + 1)]
            C[x, y] = [sum(abs(lp[yy][xx] - rp[yy][xx - d]) for xx, yy in win) for d in range(ndisp)]   # indexed by d here
            T[x, y] = sum(abs(lp[yy][xx] - 31) for xx, yy in win)
    S = {k: [0] * ndisp for k in C}
    walks = [[[(x, y) for x in xs] for y in ys], [[(x, y) for x in reversed(xs)] for y in ys],
             [[(x, y) for y in ys] for x in xs], [[(x, y) for y in reversed(ys)] for x in xs]]
    for lines in walks:
        for line in lines:
            prev = None
            for pos in line:
                c = C[pos]
                if prev is None:
                    cur = list(c)
                else:
                    m = min(prev)
                    cur = []
                    for d in range(ndisp):
                        cands = [prev[d], m + p2]
                        if d - 1 >= 0:
                            cands.append(prev[d - 1] + p1)
                        if d + 1 < ndisp:
                            cands.append(prev[d + 1] + p1)
                        cur.append(c[d] + min(cands) - m)
                for d in range(ndisp):
                    S[pos][d] += cur[d]
                prev = cur
    for (x, y), s in S.items():
        if T[x, y] < 10:
            continue
        m = min(s)
        best = max(d for d in range(ndisp) if s[d] == m)                 # the largest d among equal minima
        limit = m + (m * 15) // 100
        if any(abs(d - best) > 1 and s[d] <= limit for d in range(ndisp)):
            continue
        # in StereoBM's index i = ndisp - 1 - d: p = s[i + 1] = S at d - 1, n = s[i - 1] = S at d + 1, mirrored at the ends
        p = s[best - 1] if best - 1 >= 0 else s[1]
        n = s[best + 1] if best + 1 < ndisp else s[ndisp - 2]
        dd = p + n - 2 * m + abs(p - n)
        term = 0
        if dd != 0:
            num = (p - n) * 256
            term = abs(num) // dd if num >= 0 else -(abs(num) // dd)
        disp[y][x] = (best * 256 + term + 15) >> 4
        cost[y][x] = min((m + 2) >> 2, 0xFFFE)
    return disp, cost


# ------------------------------------------------------------------------------------------------ scenes
def planes_pair(h=96, w=192, seed=5, amp=3, noise=3):
    """Two half-planes at d = 6 (left half) and d = 18, texture 100 +- amp, independent +- noise per eye: weak texture."""
    rng = np.random.default_rng(seed)
    T = 100 + rng.integers(-amp, amp + 1, (h, w + 32))
    L = T[:, :w].copy()
    R = np.empty_like(L)
    R[:, :w // 2] = T[:, 6:6 + w // 2]
    R[:, w // 2:] = T[:, 18 + w // 2:18 + w]
    if noise:
        L = L + rng.integers(-noise, noise + 1, L.shape)
        R = R + rng.integers(-noise, noise + 1, R.shape)
    return L.astype(np.uint8), R.astype(np.uint8)
