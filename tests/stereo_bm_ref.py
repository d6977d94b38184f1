"""numpy restatement of cv::StereoBM::compute as SURVEY.md Appendix A.2 publishes it (X-Sobel prefilter cap 31, minDisparity 0,
textureThreshold 10, uniquenessRatio 15, no speckle pass, no L-R check), plus a scene builder whose bands reach every decision of it.

Independent of oracle/ora_stereo.cpp and of the kernels (neither is imported, neither was its structure followed): the oracle walks
one pixel at a time over a window; here every disparity is one |lp - rp| plane, box-summed with a 2-D cumulative sum, and the
selection is whole-array arithmetic.  All of it is exact integer arithmetic in int64, so `==` is the comparison."""
import numpy as np

CAP = 31
TEXTURE_THRESHOLD = 10
UNIQUENESS_RATIO = 15
FILTERED = -16
N_BANDS = 8

STAT_KEYS = ("texture", "texture_edge", "uniq", "uniq_edge", "kept", "d_max", "d_zero", "tie_adj", "neg", "pos", "peq")


def prefilter(img, cap=CAP):
    """X-Sobel, rows reflected (row -1 = row 1, row H = row H-2), clipped to +-cap, plus cap; columns 0 and W-1 and the last row of
    an odd-height image are cap."""
    a = np.asarray(img, np.uint8).astype(np.int64)
    H, W = a.shape
    out = np.full((H, W), cap, np.int64)
    if H >= 2 and W >= 3:
        pad = np.concatenate([a[1:2], a, a[H - 2:H - 1]], 0)
        dx = pad[:, 2:] - pad[:, :-2]                       # (H + 2, W - 2): I[., x+1] - I[., x-1]
        out[:, 1:-1] = np.clip(dx[:-2] + 2 * dx[1:-1] + dx[2:], -cap, cap) + cap
    if H & 1:
        out[H - 1] = cap
    return out.astype(np.uint8)


def _box(a, k):
    """Sums over every k x k window of the last two axes: (..., h, w) -> (..., h - k + 1, w - k + 1)."""
    c = np.zeros(a.shape[:-2] + (a.shape[-2] + 1, a.shape[-1] + 1), np.int64)
    c[..., 1:, 1:] = a.cumsum(-2).cumsum(-1)
    return c[..., k:, k:] - c[..., :-k, k:] - c[..., k:, :-k] + c[..., :-k, :-k]


def valid_rect(h, w, ndisp, block):
    """(x0, x1, y0, y1): x in [x0, x1), y in [y0, y1) is where StereoBM computes; everything else is FILTERED."""
    half = block // 2
    return ndisp - 1 + half, w - half, half, h - half


def _solve(L, R, ndisp, block):
    """-> (map int16 (H, W), masks: dict of bool (H, W) arrays, one per STAT_KEYS, False outside the valid rectangle)."""
    L, R = np.asarray(L, np.uint8), np.asarray(R, np.uint8)
    H, W = L.shape
    assert R.shape == (H, W)
    out = np.full((H, W), FILTERED, np.int16)
    masks = {k: np.zeros((H, W), bool) for k in STAT_KEYS}
    x0, x1, y0, y1 = valid_rect(H, W, ndisp, block)
    if x1 <= x0 or y1 <= y0:
        return out, masks
    lp, rp = prefilter(L).astype(np.int64), prefilter(R).astype(np.int64)
    # a window centred on a valid x starts at x - half >= ndisp - 1: only columns ndisp - 1 .. W - 1 of the left image are ever summed
    lc = lp[:, ndisp - 1:]
    planes = np.empty((ndisp, H, W - ndisp + 1), np.int64)
    for d in range(ndisp):
        planes[ndisp - 1 - d] = np.abs(lc - rp[:, ndisp - 1 - d:W - d])      # index i = ndisp - 1 - d
    s = _box(planes, block)                                                   # (ndisp, y1 - y0, x1 - x0)
    tsum = _box(np.abs(lc - CAP), block)
    assert s.shape[1:] == (y1 - y0, x1 - x0) == tsum.shape

    mind = s.argmin(0)                                                        # the first minimum
    m = s.min(0)
    thresh = m + m * UNIQUENESS_RATIO // 100                                  # m >= 0: floor == C division
    far = np.abs(np.arange(ndisp)[:, None, None] - mind[None]) > 1
    not_unique = (far & (s <= thresh[None])).any(0)
    at_thresh = (far & (s == thresh[None])).any(0)
    ext = np.concatenate([s[1:2], s, s[ndisp - 2:ndisp - 1]], 0)              # ext[i + 1] = s[i]; s[-1] = s[1], s[ndisp] = s[ndisp - 2]
    p = np.take_along_axis(ext, (mind + 2)[None], 0)[0]
    n = np.take_along_axis(ext, mind[None], 0)[0]
    dd = p + n - 2 * m + np.abs(p - n)                                        # = 2 (max(p, n) - m) >= 0
    num = (p - n) * 256
    term = np.where(dd != 0, np.sign(num) * (np.abs(num) // np.maximum(dd, 1)), 0)   # C division: truncated toward zero
    value = ((ndisp - mind - 1) * 256 + term + 15) >> 4                       # arithmetic shift

    textured = tsum >= TEXTURE_THRESHOLD
    kept = textured & ~not_unique
    out[y0:y1, x0:x1] = np.where(kept, value, FILTERED).astype(np.int16)

    inner = {
        "texture": ~textured,
        "texture_edge": (tsum >= TEXTURE_THRESHOLD) & (tsum < TEXTURE_THRESHOLD + 4),
        "uniq": textured & not_unique,
        "uniq_edge": textured & at_thresh,
        "kept": kept,
        "d_max": kept & (mind == 0),
        "d_zero": kept & (mind == ndisp - 1),
        "tie_adj": kept & (mind + 1 < ndisp) & (p == m),                      # p = s[mind + 1] unless mirrored
        "neg": kept & (p < n),
        "pos": kept & (p > n),
        "peq": kept & (p == n),
    }
    for k in STAT_KEYS:
        masks[k][y0:y1, x0:x1] = inner[k]
    return out, masks


def stereo_bm(L, R, ndisp, block, stats=None):
    """The CV_16S map (4 fractional bits) of StereoBM(ndisp, block); `stats`, when a dict, receives the count of each STAT_KEYS
    category over the valid rectangle."""
    out, masks = _solve(L, R, ndisp, block)
    if stats is not None:
        for k in STAT_KEYS:
            stats[k] = int(masks[k].sum())
    return out


def categories(L, R, ndisp, block):
    """-> (map, dict of bool (H, W) masks per STAT_KEYS): which pixels took which decision (for reports and point selection)."""
    return _solve(L, R, ndisp, block)


def disparity_at(L, R, xy, ndisp, block, disp16=None):
    """convertTo(CV_32F, 1/16) of the map sampled at ((int)x, (int)y) — truncation toward zero; -1.0 outside the valid rectangle.
    `disp16`: the map of this pair if the caller already has it."""
    m = stereo_bm(L, R, ndisp, block) if disp16 is None else disp16
    H, W = m.shape
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    x = np.trunc(xy[:, 0]).astype(np.int64)
    y = np.trunc(xy[:, 1]).astype(np.int64)
    x0, x1, y0, y1 = valid_rect(H, W, ndisp, block)
    ok = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    v = np.full(len(xy), FILTERED, np.int16)
    v[ok] = m[y[ok], x[ok]]
    return v.astype(np.float32) * np.float32(1.0 / 16.0)


def band_rows(h):
    """Row ranges of the eight bands: equal height h // 8; the h % 8 rows left over continue the last band."""
    bh = h // N_BANDS
    return [(k * bh, (k + 1) * bh if k < N_BANDS - 1 else h) for k in range(N_BANDS)]


def reverse_bands(img):
    """The same bands, last one on top."""
    return np.ascontiguousarray(np.concatenate([img[a:b] for a, b in reversed(band_rows(img.shape[0]))], 0))


def scene(h, w, ndisp, seed):
    """(L, R) uint8 (h, w): eight horizontal bands, each cut from one wide texture T as L = T[:, :w], R = T[:, d:d + w].

      1 noise 0..255, d = 0               winners at d = 0 (index ndisp - 1: the mirrored border s[ndisp] = s[ndisp - 2])
      2 noise 0..255, d = ndisp - 1       winners at the largest disparity (index 0: s[-1] = s[1])
      3 noise 0..255, d = ndisp // 3      ordinary winners
      4 constant 77, d = 5                no texture at all
      5 100, plus 1 with a probability per pixel that rises along the row from 0.0005 to 0.04, d = 3
                                          texture sums on both sides of the threshold.  One such pixel adds 8 to the texture sum of a
                                          window that holds it whole, so the sum straddles 10 where a window holds one or two: near
                                          0.004 for a 21 x 21 window, near 0.03 for 7 x 7 — the rise passes through both
      6 vertical stripes ((x // 3) % 2) * 40 + 80, d = 4         period 6 < ndisp: equal minima, fails uniqueness at equality
      7 4 x 4 blocks of 100 or 109, d = 7  low contrast: unclipped prefilter values, sub-pixel terms of both signs
      8 two-level noise (100 or 140) with every column doubled, R the rounded mean of the shifts 6 and 7 (d = 6.5): ties between
                                          adjacent disparities.  The noise is sparse (probability per column pair rising along the row
                                          from 0.003 to 0.15): the left image of a lone pair and the right image of it mirror each other
                                          about a point half a pixel between the shifts 6 and 7, so both SADs are EQUAL wherever a window
                                          holds lone pairs whole.  Dense noise 0..255 ties only by chance: 0 to 3 pixels per scene with a
                                          21 x 21 window
    """
    rng = np.random.default_rng(seed)
    wt = w + ndisp + 8
    L = np.empty((h, w), np.uint8)
    R = np.empty((h, w), np.uint8)
    xs = np.arange(wt)
    for k, (a, b) in enumerate(band_rows(h)):
        bh = b - a
        if k < 3:
            T = rng.integers(0, 256, (bh, wt))
            d = (0, ndisp - 1, ndisp // 3)[k]
        elif k == 3:
            T, d = np.full((bh, wt), 77), 5
        elif k == 4:
            T, d = 100 + (rng.random((bh, wt)) < 0.0005 * 80.0 ** (xs / (wt - 1))).astype(np.int64), 3
        elif k == 5:
            T, d = np.broadcast_to(((xs // 3) % 2) * 40 + 80, (bh, wt)), 4
        elif k == 6:
            T = 100 + 9 * np.kron(rng.integers(0, 2, (bh // 4 + 1, wt // 4 + 1)), np.ones((4, 4), np.int64))[:bh, :wt]
            d = 7
        else:
            dens = 0.003 * 50.0 ** (np.arange(wt // 2 + 1) / (wt // 2))
            T = 100 + 40 * np.kron(rng.random((bh, wt // 2 + 1)) < dens, np.ones((1, 2), np.int64))[:, :wt]
            L[a:b] = T[:, :w]
            R[a:b] = (T[:, 6:6 + w] + T[:, 7:7 + w] + 1) // 2
            continue
        L[a:b] = T[:, :w]
        R[a:b] = T[:, d:d + w]
    return L, R
