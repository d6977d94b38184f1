"""A second statement of SURVEY Appendix A.1 (Shi-Tomasi corners, cv::goodFeaturesToTrack with blockSize 3) in numpy, by another route than
oracle/ora_corner.cpp: reflect-101 by np.pad, whole-array f32 operations, the 3x3 box as nine shifted f64 adds, a stable lexicographic
sort, and a plain greedy selection against EVERY accepted corner with exact integer distances (no grid).  It imports nothing from the
oracle or the library.  Declared arithmetic: Sobel, products and the eigenvalue in f32, one rounding per operation, no fused
multiply-add; the box sum in f64 (nine f32 products whose exponents span < 2^29: exact in any order), rounded once to f32.

Also here: the decision counters of a detection (how often an input reaches each branch of the function) and the scenes of
tests/test_corner_paths.py.  Every scene is small and comes from a fixed seed."""
import numpy as np

F32 = np.float32
K1 = F32(1.0 / (4.0 * 3.0 * 255.0))
K0 = F32(2.0 / (4.0 * 3.0 * 255.0))


# ------------------------------------------------------------------------------------------------ the function
def response(img):
    """Minimum eigenvalue map (H, W) f32 of the 3x3 gradient covariance."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    assert h >= 3 and w >= 3
    p = np.pad(img.astype(np.int32), 1, mode="reflect")          # pixels reflect: (H + 2, W + 2)
    l, m, r = p[:, :-2], p[:, 1:-1], p[:, 2:]                    # row pass on every (padded) row
    rdx = (r - l).astype(F32)
    rdy = m.astype(F32) * K0 + (l + r).astype(F32) * K1
    dx = (rdx[:-2] + rdx[2:]) * K1 + rdx[1:-1] * K0              # column pass
    dy = rdy[2:] - rdy[:-2]
    assert dx.dtype == F32 and dy.dtype == F32 and dx.shape == (h, w)

    def box(c):
        q = np.pad(c, 1, mode="reflect").astype(np.float64)      # covariance COORDINATES reflect: cov(-1) = cov(1), cov(n) = cov(n - 2)
        s = np.zeros((h, w), np.float64)
        for j in range(3):
            for i in range(3):
                s += q[j:j + h, i:i + w]
        return s.astype(F32)

    a = box(dx * dx) * F32(0.5)
    b = box(dx * dy)
    c = box(dy * dy) * F32(0.5)
    d = a - c
    eig = (a + c) - np.sqrt(d * d + b * b)
    assert eig.dtype == F32
    return eig


def threshold(maxv, quality):
    return F32(np.float64(maxv) * np.float64(quality))


def candidates(eig, quality, maxv=None):
    """Raster indices (ascending) of the candidates: interior pixels above the threshold that equal the 3x3 maximum of the thresholded map."""
    h, w = eig.shape
    thr = threshold(eig.max() if maxv is None else maxv, quality)
    t = np.where(eig > thr, eig, F32(0))
    q = np.pad(t, 1, mode="constant", constant_values=-np.inf)   # neighbours outside the image are ignored
    mx = np.full((h, w), -np.inf, F32)
    for j in range(3):
        for i in range(3):
            mx = np.maximum(mx, q[j:j + h, i:i + w])
    ok = (t != 0) & (t == mx)
    ok[0, :] = ok[-1, :] = False
    ok[:, 0] = ok[:, -1] = False
    return np.flatnonzero(ok.ravel())


def order(eig, idx):
    """Value descending, then raster index descending."""
    v = eig.ravel()[idx]
    return idx[np.lexsort((idx, v))[::-1]]


def md2_f32(min_distance):
    return F32(min_distance) * F32(min_distance)                 # rounded to f32


def select(idx, w, min_distance, limit=None):
    """Greedy over the ordered candidates: accept unless an accepted corner lies at integer dx^2 + dy^2 < f32(md) * f32(md).
    min_distance < 1: no distance test.  Stops at limit.  Returns the accepted raster indices in acceptance order."""
    n = len(idx) if limit is None else min(limit, len(idx))
    if min_distance < 1.0:
        return idx[:n].copy()
    md2 = float(md2_f32(min_distance))
    xs, ys = (idx % w).astype(np.int64), (idx // w).astype(np.int64)
    ax, ay = np.empty(len(idx), np.int64), np.empty(len(idx), np.int64)
    out = np.empty(len(idx), idx.dtype)
    k = 0
    for i in range(len(idx)):
        ddx, ddy = ax[:k] - xs[i], ay[:k] - ys[i]
        if k and ((ddx * ddx + ddy * ddy) < md2).any():
            continue
        ax[k], ay[k], out[k] = xs[i], ys[i], idx[i]
        k += 1
        if k == n:
            break
    return out[:k].copy()


def to_xy(idx, w):
    return np.stack([idx % w, idx // w], 1).astype(F32).reshape(-1, 2)


def detect(img, max_corners, quality, min_distance):
    """(n, 2) f32 corners (x, y), strongest first."""
    eig = response(img)
    return to_xy(select(order(eig, candidates(eig, quality)), eig.shape[1], min_distance, max_corners), eig.shape[1])


# ------------------------------------------------------------------------------------------------ decision counters
def rounds(idx, w, min_distance):
    """Rounds that the plain monotone fixed point needs over the ordered candidates: per round (all at once) a candidate is accepted
    when every stronger candidate within min_distance is rejected, rejected when one of them is accepted.  That is the length of the
    longest chain of 'stronger candidate within min_distance, still undecided' links.  Also returns the accepted set it ends with."""
    if min_distance < 1.0 or len(idx) == 0:
        return (1 if len(idx) else 0), idx.copy()
    md2 = float(md2_f32(min_distance))
    xs, ys = (idx % w).astype(np.int64), (idx // w).astype(np.int64)
    rd = np.zeros(len(idx), np.int64)
    acc = np.zeros(len(idx), bool)
    for i in range(len(idx)):
        ddx, ddy = xs[:i] - xs[i], ys[:i] - ys[i]
        near = (ddx * ddx + ddy * ddy) < md2
        hit = near & acc[:i]
        if hit.any():
            rd[i] = 1 + rd[:i][hit].min()
        else:
            acc[i] = True
            rd[i] = 1 + (rd[:i][near].max() if near.any() else 0)
    return int(rd.max()), idx[acc]


def pairs_at(idx, h, w, d2):
    """Unordered candidate pairs at squared distance exactly d2 (an integer)."""
    m = np.zeros((h, w), bool)
    m.ravel()[idx] = True
    n = 0
    r = int(np.sqrt(d2)) + 1
    for dy in range(0, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy != d2 or (dy == 0 and dx <= 0):
                continue
            a = m[:h - dy, max(0, -dx):w - max(0, dx)]
            b = m[dy:, max(0, dx):w - max(0, -dx)]
            n += int((a & b).sum())
    return n


def counters(img, max_corners, quality, min_distance, with_rounds=False):
    """The decisions of one detection, from this restatement alone."""
    eig = response(img)
    h, w = eig.shape
    cand = order(eig, candidates(eig, quality))
    full = select(cand, w, min_distance)                          # without the max_corners cut
    v = eig.ravel()
    md2 = float(md2_f32(min_distance)) if min_distance >= 1.0 else 0.0
    _, cnt = np.unique(v[cand], return_counts=True)
    inner = eig[1:-1, 1:-1].max() if h > 2 and w > 2 else -np.inf
    on_border = bool(eig.max() > inner)
    lost = 0
    if on_border:
        lost = len(np.setdiff1d(candidates(eig, quality, maxv=inner), cand))
    st = {
        "candidates": len(cand),
        "accepted": min(len(full), max_corners),
        "accepted_uncut": len(full),
        "exact_pairs": pairs_at(cand, h, w, int(md2)) if md2 >= 1.0 and md2 == int(md2) else 0,
        # the unrounded square of f32(md) lies above the integer md2: the rounding of the product alone keeps the exact pairs apart
        "square_rounds_down": bool(md2 >= 1.0 and md2 == int(md2) and float(F32(min_distance)) ** 2 > md2),
        "adjacent_pairs": pairs_at(cand, h, w, 1) + pairs_at(cand, h, w, 2),
        "ring_candidates": int(((cand % w == 1) | (cand % w == w - 2) | (cand // w == 1) | (cand // w == h - 2)).sum()),
        "tied": int(cnt[cnt > 1].sum()),
        "tie_groups": int((cnt > 1).sum()),
        "cut_in_tie": bool(len(full) > max_corners and v[full[max_corners - 1]] == v[full[max_corners]]),
        "max_on_border": on_border,
        "lost_to_border_max": lost,
    }
    if with_rounds:
        st["rounds"], acc = rounds(cand, w, min_distance)
        assert np.array_equal(np.sort(acc), np.sort(full))
    return st


# ------------------------------------------------------------------------------------------------ scenes
def pixel_noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def block_noise(h, w, seed):
    """8 x 8 blocks plus per-pixel noise (the texture of tests/test_corner.py)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2)).astype(np.uint8)
    img = np.kron(base, np.ones((8, 8), np.uint8))[:h, :w]
    return (img // 2 + rng.integers(0, 128, (h, w))).astype(np.uint8)


BORDER_SIDES = ("top", "bottom", "left", "right")
BORDER_SHAPE = (50, 125)       # one strip of rows plus two; three fused strips of columns, the last five columns wide
BORDER_SEED = {"top": 6, "bottom": 7, "left": 25, "right": 8}     # found by search on this restatement: the maximum falls on the border line


def border_max(side, seed=None):
    """A flat field, three full-contrast 3 x 3 random patches that touch one border line, and 24 faint patches of graded contrast
    inside.  Returns (image, quality): the quality puts the threshold of the true (border) maximum above one interior candidate and
    the threshold of the interior maximum below it, so a maximum taken over the interior alone keeps a corner that A.1 drops."""
    h, w = BORDER_SHAPE
    rng = np.random.default_rng(1000 * BORDER_SIDES.index(side) + (BORDER_SEED[side] if seed is None else seed))
    img = np.full((h, w), 100, np.uint8)
    for k in range(24):
        y, x = 8 + 9 * (k // 6) + int(rng.integers(0, 3)), 8 + 19 * (k % 6) + int(rng.integers(0, 5))
        amp = 20 + 3 * k
        img[y:y + 3, x:x + 3] = 100 + rng.integers(-amp // 2, amp // 2 + 1, (3, 3))
    for k in range(3):
        patch = rng.integers(0, 256, (3, 3))
        if side in ("top", "bottom"):
            x = 10 + 45 * k + int(rng.integers(0, 9))
            y = 0 if side == "top" else h - 3
        else:
            y = 4 + 17 * k + int(rng.integers(0, 5))
            x = 0 if side == "left" else w - 3
        img[y:y + 3, x:x + 3] = patch
    eig = response(img)
    inner = np.float64(eig[1:-1, 1:-1].max())
    cand = order(eig, candidates(eig, 0.0))
    v = np.float64(eig.ravel()[cand[len(cand) // 2]])            # the median candidate
    return img, float(v / ((np.float64(eig.max()) + inner) / 2))


def lattice(h, w, u, lo=100, hi=200):
    """Identical one-pixel blobs on the square lattice spanned by u = (ux, uy) and (-uy, ux)."""
    ux, uy = u
    img = np.full((h, w), lo, np.uint8)
    r = (h + w) // max(abs(ux), abs(uy)) + 2
    i, j = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    x, y = (3 + i * ux - j * uy).ravel(), (3 + i * uy + j * ux).ravel()
    ok = (x >= 3) & (x < w - 3) & (y >= 3) & (y < h - 3)
    img[y[ok], x[ok]] = hi
    return img


LATTICE = {
    # name: (shape, u)
    "pitch5": ((60, 90), (5, 0)),
    "sheared": ((64, 96), (7, 1)),
    "sq41": ((61, 93), (5, 4)),
}
SQRT50 = float(np.sqrt(50.0))
# f32(sqrt 41) = 6.4031243 and its square is 41.0000012...: above 41, but f32 rounds the product to 41.0, so blobs at offset (5, 4)
# are NOT closer than min_distance.  (f32(sqrt 50)^2 = 49.99999997 rounds to 50.0 from below: no such crossing at 50.)
SQRT41 = float(np.sqrt(41.0))


def lattice_params(name):
    if name == "pitch5":
        return [(4096, 0.01, 5.0), (4096, 0.01, 5.0001), (4096, 0.01, SQRT50), (40, 0.01, 5.0), (40, 0.01, 7.5)]
    if name == "sheared":
        return [(4096, 0.01, SQRT50), (4096, 0.01, 7.08), (25, 0.01, SQRT50)]
    return [(4096, 0.01, SQRT41), (4096, 0.01, 6.4032), (30, 0.01, SQRT41)]


CHAIN_MD = 6.5
CHAIN_STEP = 6


def _blob(img, x, y, amp):
    img[y, x] = 20 + amp


def chain_row(w=790, h=9):
    """One row of one-pixel blobs of strictly increasing contrast, CHAIN_STEP apart (under CHAIN_MD): acceptance alternates."""
    img = np.full((h, w), 20, np.uint8)
    xs = np.arange(4, w - 4, CHAIN_STEP)
    for k, x in enumerate(xs):
        _blob(img, int(x), h // 2, 235 - len(xs) + 1 + k)
    return img


def chain_zigzag(w=790, h=64):
    """A snake of one-pixel blobs CHAIN_STEP apart whose total order (value descending, raster index descending) falls along it:
    bottom row right to left with EQUAL contrast (the raster index orders them), up the left side, second row left to right with
    strictly decreasing contrast, up the right side, third row right to left with equal, lower contrast, and so on.  Rows lie three
    steps apart, so links exist only along the snake."""
    img = np.full((h, w), 20, np.uint8)
    xs = [int(x) for x in np.arange(4, w - 4, CHAIN_STEP)]
    path = []                                                    # (x, y, contrast), strongest first
    amp = 235
    y = h - 5
    leftward = True
    while y >= 4 and (leftward or amp - len(xs) >= 5):
        if leftward:
            path += [(x, y, amp) for x in reversed(xs)]
            x_end = xs[0]
        else:
            amp -= 1
            for x in xs:
                path.append((x, y, amp))
                amp -= 1
            x_end = xs[-1]
        if y - 3 * CHAIN_STEP < 4:
            break
        amp -= 1
        for s in (1, 2):                                         # the connector climbs with decreasing contrast
            path.append((x_end, y - s * CHAIN_STEP, amp))
            amp -= 1
        y -= 3 * CHAIN_STEP
        leftward = not leftward
    for x, yy, a in path:
        _blob(img, x, yy, a)
    return img


DENSE = {"lds": (256, 736), "global": (256, 790)}               # widths tuned on this restatement alone (test_corner_paths.DENSE_RANGE)
DENSE_PARAMS = (16384, 0.0, 5.0)


def dense(which):
    h, w = DENSE[which]
    return pixel_noise(256, 800, 21)[:h, :w].copy()


CELLS_MD = (1.0, 1.49, 2.5, 12.5)


def cells_scene():
    """Left: per-pixel noise; right: 2 x 2 bright blocks at pitch 9.  A block is mirror symmetric about both of its half-pixel axes, so
    its four pixels have the same response bit for bit: four mutually 8-adjacent equal candidates, which min_distance 1.0 keeps
    (1 < 1 is false) and 1.49 thins to one."""
    img = np.full((96, 200), 60, np.uint8)
    img[:, :110] = pixel_noise(96, 110, 31)
    for y in range(6, 88, 9):
        for x in range(118, 192, 9):
            img[y:y + 2, x:x + 2] = 180
    return img


STRIPS = [(3, 3), (3, 5), (4, 4), (3, 121), (4, 59), (47, 60), (48, 61), (49, 62), (50, 63), (97, 121), (97, 3), (48, 5), (49, 59), (50, 4)]
STRIPS_PARAMS = (4096, 0.0, 2.0)


def strips(h, w):
    return pixel_noise(h, w, 1000 * h + w)


# ------------------------------------------------------------------------------------------------ the cases of test_corner_paths.py
def cases():
    """id -> (image, max_corners, quality, min_distance), in a fixed order."""
    out = {}
    for side in BORDER_SIDES:
        img, q = border_max(side)
        out["border-" + side] = (img, 4096, q, 4.0)
    for name, (shape, u) in LATTICE.items():
        img = lattice(*shape, u)
        for k, p in enumerate(lattice_params(name)):
            out["lattice-%s-%d" % (name, k)] = (img,) + p
    out["chain-row"] = (chain_row(), 4096, 0.0, CHAIN_MD)
    out["chain-zigzag"] = (chain_zigzag(), 4096, 0.0, CHAIN_MD)
    for which in DENSE:
        out["dense-" + which] = (dense(which),) + DENSE_PARAMS
    cs = cells_scene()
    for md in CELLS_MD:
        out["cells-%g" % md] = (cs, 4096, 0.01, md)
    for h, w in STRIPS:
        out["strips-%dx%d" % (h, w)] = (strips(h, w),) + STRIPS_PARAMS
    for v in out.values():
        v[0].setflags(write=False)
    return out
