"""The voxel map sight lines (include/svo.h, "Voxel map sight lines") restated without a GPU.  The walk is stated by
two routes that share no code:

  (a) walk_a: the contract's incremental rule in Python integers: the X of the three axes, the smallest one steps;
  (b) walk_b: every boundary crossing of every moving axis listed as the exact fraction n / |D| (fractions.Fraction), sorted by
      (t, axis), then followed in that order.  No X, no w, no running state but the cell.

The set-up is restated twice as well (setup_a in Python floats as the contract writes it, setup_b with every floor taken of an
exact Fraction), and so is the coarse volume (coarse_np: a reshape and an any; coarse_py: bit by bit).  walk_skip is a third
statement of the walk, the block-skipping form over the coarse volume, which must give what (a) gives and also says how many
cells it jumped.  `variant` states one deliberate misreading of the contract each; every one must change a stated scene
(tests/test_voxel_rays.py)."""
import math
from fractions import Fraction

import numpy as np

RAY = np.dtype([("ox", np.float32), ("oy", np.float32), ("oz", np.float32), ("max_range", np.float32), ("dx", np.float32), ("dy", np.float32),
                ("dz", np.float32), ("tag", np.uint32)])
HIT_T = np.dtype([("cell", np.uint32), ("steps", np.uint32), ("dist", np.float32), ("status", np.uint32)])
HIT, LEFT, RANGE, OUTSIDE, REJECTED = range(5)
CODES = ("n_hit", "n_left", "n_range", "n_outside", "n_rejected")
NO_CELL = 0xFFFFFFFF
LIMIT = 1048560.0
STILL = 1 << 62
FILTERED = -16
VARIANTS = ("tie_largest", "range_after", "neg_n", "D_trunc", "min_step_off", "z_ray", "coarse_world")


def occupancy_words(dims):
    return dims[0] // 64 * dims[1] * dims[2]


def coarse_dims(dims):
    return tuple((d + 7) >> 3 for d in dims)


def coarse_words(dims):
    c = coarse_dims(dims)
    return (c[0] * c[1] * c[2] + 63) >> 6


def bits_of(cells, dims):
    """The volume's words with the bits of `cells` (j triples inside the volume) set."""
    w = [0] * occupancy_words(dims)
    for j in cells:
        assert all(0 <= j[r] < dims[r] for r in range(3)), j
        B = j[0] + dims[0] * (j[1] + dims[1] * j[2])
        w[B >> 6] |= 1 << (B & 63)
    return np.array(w, np.uint64)


class Volume:
    """A volume's words for the walks: bit(B) of the fine volume, cbit(Bc) of a coarse volume."""
    def __init__(self, words, dims, coarse=None):
        self.dims = tuple(int(v) for v in dims)
        self.fine = np.ascontiguousarray(words, np.uint64).view(np.uint8).tobytes()  # little-endian words: byte B >> 3 holds bit B & 7
        self.coarse = None if coarse is None else np.ascontiguousarray(coarse, np.uint64).view(np.uint8).tobytes()
        assert len(self.fine) == 8 * occupancy_words(self.dims)

    def bit(self, B):
        return self.fine[B >> 3] >> (B & 7) & 1

    def cbit(self, Bc):
        return self.coarse[Bc >> 3] >> (Bc & 7) & 1


# ------------------------------------------------------------------------------------------------ item 1: the coarse volume
def coarse_np(words, dims, origin=(0, 0, 0), variant=None):
    d0, d1, d2 = dims
    c0, c1, c2 = coarse_dims(dims)
    cells = np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder="little").reshape(d2, d1, d0)
    if variant == "coarse_world":  # the block of the unshifted world index: wrong wherever the origin is no multiple of 8
        out = np.zeros((c2, c1, c0), np.uint8)
        for j2, j1, j0 in np.argwhere(cells):
            b = [((j + int(o)) >> 3) - (int(o) >> 3) for j, o in zip((j0, j1, j2), origin)]
            if b[0] < c0 and b[1] < c1 and b[2] < c2:
                out[b[2], b[1], b[0]] = 1
    else:
        pad = np.zeros((8 * c2, 8 * c1, 8 * c0), np.uint8)
        pad[:d2, :d1, :d0] = cells
        out = pad.reshape(c2, 8, c1, 8, c0, 8).any(axis=(1, 3, 5)).astype(np.uint8)
    flat = np.zeros(64 * coarse_words(dims), np.uint8)
    flat[:c0 * c1 * c2] = out.reshape(-1)
    return np.packbits(flat, bitorder="little").view(np.uint64)


def coarse_py(words, dims):
    d0, d1, d2 = dims
    c0, c1, c2 = coarse_dims(dims)
    w = [0] * coarse_words(dims)
    for i, word in enumerate(int(v) for v in words):
        while word:
            low = word & -word
            B = 64 * i + low.bit_length() - 1
            word ^= low
            j0, j1, j2 = B % d0, B // d0 % d1, B // (d0 * d1)
            Bc = (j0 >> 3) + c0 * ((j1 >> 3) + c1 * (j2 >> 3))
            w[Bc >> 6] |= 1 << (Bc & 63)
    return np.array(w, np.uint64)


# ------------------------------------------------------------------------------------------------ item 2: the set-up
class Setup:
    __slots__ = ("p", "D", "L", "S", "m")

    def key(self):
        return (tuple(self.p), tuple(self.D), tuple(self.L), self.S, self.m)


def _finite(v):
    return not (math.isnan(v) or math.isinf(v))


def setup_a(o, d, max_range, voxel_size, origin, variant=None):
    """o, d: three Python floats each (a record's f32 widened); None: REJECTED."""
    vs = float(np.float32(voxel_size))
    if not all(_finite(v) for v in (*o, *d, max_range)) or max_range < 0.0:
        return None
    m = max(abs(d[0]), abs(d[1]), abs(d[2]))
    if m == 0.0:
        return None
    q = [o[r] / vs for r in range(3)]
    if not all(-LIMIT <= v < LIMIT for v in q):
        return None
    s = Setup()
    s.p = [int(math.floor(q[r] * 256.0)) - 256 * int(origin[r]) for r in range(3)]
    if variant == "D_trunc":
        s.D = [int((d[r] / m) * 16384.0) for r in range(3)]
    else:
        s.D = [int(math.floor((d[r] / m) * 16384.0 + 0.5)) for r in range(3)]
    s.S = s.D[0] ** 2 + s.D[1] ** 2 + s.D[2] ** 2
    R = (max_range / vs) * 256.0
    s.L = [int(min(math.floor((R * float(abs(s.D[r]))) / math.sqrt(float(s.S))), 2.0 ** 40)) for r in range(3)]
    s.m = m
    return s


def setup_b(o, d, max_range, voxel_size, origin):
    """The same with every floor taken of an exact rational: a floor of a double is a property of its value, however it is taken."""
    vs = float(np.float32(voxel_size))
    vals = list(o) + list(d) + [max_range]
    if any(v != v or v in (math.inf, -math.inf) for v in vals) or max_range < 0:
        return None
    m = sorted(abs(v) for v in d)[-1]
    if m == 0:
        return None
    q = [o[r] / vs for r in range(3)]
    if any(Fraction(v) < Fraction(-1048560) or Fraction(v) >= Fraction(1048560) for v in q):
        return None
    s = Setup()
    s.p = [(Fraction(q[r]) * 256).__floor__() - 256 * int(origin[r]) for r in range(3)]  # * 256 is exact in f64
    s.D = [Fraction((d[r] / m) * 16384.0 + 0.5).__floor__() for r in range(3)]
    s.S = sum(v * v for v in s.D)
    R = (max_range / vs) * 256.0
    root = float(np.sqrt(np.float64(s.S)))
    s.L = [min(Fraction((R * float(abs(s.D[r]))) / root).__floor__(), 1 << 40) for r in range(3)]
    s.m = m
    return s


# ------------------------------------------------------------------------------------------------ item 3: the walk
def _cell(c, dims):
    return c[0] + dims[0] * (c[1] + dims[1] * c[2])


def _tested(k, min_step, variant):
    return k > min_step if variant == "min_step_off" else k >= min_step


def walk_a(s, vol, min_step, variant=None):
    """(code, axis, cell, steps, n_a, |D_a|) by the incremental rule."""
    dims = vol.dims
    c = [s.p[r] >> 8 for r in range(3)]
    f = [s.p[r] & 255 for r in range(3)]
    if not all(0 <= c[r] < dims[r] for r in range(3)):
        return (OUTSIDE, 3, NO_CELL, 0, 0, 1)
    k = 0
    cell = _cell(c, dims)
    if _tested(0, min_step, variant) and vol.bit(cell):
        return (HIT, 3, cell, 0, 0, 1)
    aD = [abs(v) for v in s.D]
    n = [(256 - f[r]) if (s.D[r] > 0 or variant == "neg_n") else f[r] for r in range(3)]
    w = [max(aD[(r + 1) % 3], 1) * max(aD[(r + 2) % 3], 1) for r in range(3)]
    X = [n[r] * w[r] if s.D[r] else STILL for r in range(3)]
    for _ in range(dims[0] + dims[1] + dims[2]):
        lo = min(X)
        a = max(r for r in range(3) if X[r] == lo) if variant == "tie_largest" else X.index(lo)
        if variant != "range_after" and n[a] > s.L[a]:
            return (RANGE, a, cell, k, n[a], aD[a])
        c[a] += 1 if s.D[a] > 0 else -1
        if not 0 <= c[a] < dims[a]:
            return (LEFT, a, cell, k, n[a], aD[a])
        k += 1
        cell = _cell(c, dims)
        if _tested(k, min_step, variant) and vol.bit(cell):
            return (HIT, a, cell, k, n[a], aD[a])
        if variant == "range_after" and n[a] > s.L[a]:
            return (RANGE, a, cell, k, n[a], aD[a])
        n[a] += 256
        X[a] += 256 * w[a]
    raise AssertionError("the walk outran d0 + d1 + d2")


def walk_b(s, vol, min_step):
    """The same by the sorted list of all crossings, each at the exact t = n / |D|."""
    dims = vol.dims
    c = [v // 256 for v in s.p]
    if any(not 0 <= c[r] < dims[r] for r in range(3)):
        return (OUTSIDE, 3, NO_CELL, 0, 0, 1)
    cell = _cell(c, dims)
    if min_step <= 0 and vol.bit(cell):
        return (HIT, 3, cell, 0, 0, 1)
    crossings = []
    for r in range(3):
        if s.D[r] == 0:
            continue
        frac = s.p[r] - 256 * c[r]
        first = 256 - frac if s.D[r] > 0 else frac
        crossings += [(Fraction(first + 256 * i, abs(s.D[r])), r, first + 256 * i) for i in range(dims[r] + 1)]
    crossings.sort(key=lambda t: (t[0], t[1]))
    k = 0
    for _, a, na in crossings:
        if na > s.L[a]:
            return (RANGE, a, cell, k, na, abs(s.D[a]))
        c[a] += (s.D[a] > 0) - (s.D[a] < 0)
        if not 0 <= c[a] < dims[a]:
            return (LEFT, a, cell, k, na, abs(s.D[a]))
        k += 1
        cell = _cell(c, dims)
        if k >= min_step and vol.bit(cell):
            return (HIT, a, cell, k, na, abs(s.D[a]))
    raise AssertionError("the list of crossings ran out inside the volume")


def walk_skip(s, vol, min_step):
    """The block-skipping walk over vol.coarse: (walk_a's tuple, cells jumped, jumps)."""
    dims = vol.dims
    cd = coarse_dims(dims)
    c = [s.p[r] >> 8 for r in range(3)]
    if not all(0 <= c[r] < dims[r] for r in range(3)):
        return (OUTSIDE, 3, NO_CELL, 0, 0, 1), 0, 0
    cell = _cell(c, dims)
    if min_step == 0 and vol.bit(cell):
        return (HIT, 3, cell, 0, 0, 1), 0, 0
    sg = [(v > 0) - (v < 0) for v in s.D]
    aD = [abs(v) for v in s.D]
    n = [(256 - (s.p[r] & 255)) if sg[r] > 0 else (s.p[r] & 255) for r in range(3)]
    w = [max(aD[(r + 1) % 3], 1) * max(aD[(r + 2) % 3], 1) for r in range(3)]
    X = [n[r] * w[r] if sg[r] else STILL for r in range(3)]
    k = jumped = jumps = 0
    while True:
        if not vol.cbit((c[0] >> 3) + cd[0] * ((c[1] >> 3) + cd[1] * (c[2] >> 3))):
            e = [min(8 - (c[r] & 7), dims[r] - c[r]) if sg[r] > 0 else (c[r] & 7) + 1 for r in range(3)]
            Xe = [X[r] + 256 * w[r] * (e[r] - 1) if sg[r] else STILL for r in range(3)]
            a = Xe.index(min(Xe))
            ms = [0, 0, 0]
            for r in range(3):
                if r == a:
                    ms[r] = e[r] - 1
                elif sg[r]:
                    ms[r] = sum(1 for i in range(8) if (X[r] + 256 * w[r] * i <= Xe[a] if r < a else X[r] + 256 * w[r] * i < Xe[a]))
                    assert ms[r] <= 7
            if all(ms[r] == 0 or n[r] + 256 * (ms[r] - 1) <= s.L[r] for r in range(3)):
                for r in range(3):
                    c[r] += sg[r] * ms[r]
                    n[r] += 256 * ms[r]
                    X[r] += 256 * w[r] * ms[r] if sg[r] else 0
                k += sum(ms)
                jumped += sum(ms)
                jumps += 1 if sum(ms) else 0
                cell = _cell(c, dims)
        a = X.index(min(X))
        if n[a] > s.L[a]:
            return (RANGE, a, cell, k, n[a], aD[a]), jumped, jumps
        c[a] += sg[a]
        if not 0 <= c[a] < dims[a]:
            return (LEFT, a, cell, k, n[a], aD[a]), jumped, jumps
        k += 1
        cell = _cell(c, dims)
        if k >= min_step and vol.bit(cell):
            return (HIT, a, cell, k, n[a], aD[a]), jumped, jumps
        n[a] += 256
        X[a] += 256 * w[a]


# ------------------------------------------------------------------------------------------------ items 4 to 6: records and counts
def record(end, s, voxel_size):
    code, axis, cell, k, na, ad = end
    vs = float(np.float32(voxel_size))
    dist = 0.0 if axis == 3 else ((float(na) * math.sqrt(float(s.S))) / float(ad)) / 256.0 * vs
    return (cell, k, np.float32(dist), code | axis << 8)


REJECTED_RECORD = (NO_CELL, 0, np.float32(0.0), REJECTED | 3 << 8)


def widen(ray):
    return [float(ray["ox"]), float(ray["oy"]), float(ray["oz"])], [float(ray["dx"]), float(ray["dy"]), float(ray["dz"])], float(ray["max_range"])


def rays(words, origin, dims, recs, min_step, voxel_size, route="a", variant=None, coarse=None):
    """(n HIT_T records, [n_hit, n_left, n_range, n_outside, n_rejected, n_steps]).  route: "a", "b" or "skip" (needs coarse)."""
    vol = Volume(words, dims, coarse)
    out = np.zeros(len(recs), HIT_T)
    counts = [0] * 6
    for i, ray in enumerate(recs):
        o, d, mr = widen(ray)
        s = setup_b(o, d, mr, voxel_size, origin) if route == "b" else setup_a(o, d, mr, voxel_size, origin, variant)
        if s is None:
            out[i] = REJECTED_RECORD
            counts[REJECTED] += 1
            continue
        end = walk_b(s, vol, min_step) if route == "b" else (walk_skip(s, vol, min_step)[0] if route == "skip" else walk_a(s, vol, min_step, variant))
        out[i] = record(end, s, voxel_size)
        counts[end[0]] += 1
        counts[5] += end[3]
    return out, counts


def make_rays(rows):
    """rows of (ox, oy, oz, max_range, dx, dy, dz[, tag]) -> RAY records."""
    out = np.zeros(len(rows), RAY)
    for i, row in enumerate(rows):
        out[i] = tuple(np.float32(v) for v in row[:7]) + (np.uint32(row[7] if len(row) > 7 else i),)
    return out


# ------------------------------------------------------------------------------------------------ item 8: the camera form
def pixel_ray(m12, cam, x, y):
    focal, cx, cy, _ = cam
    v0, v1 = (float(x) - cx) / focal, (float(y) - cy) / focal
    d = [m12[4 * r] * v0 + m12[4 * r + 1] * v1 + m12[4 * r + 2] for r in range(3)]
    return [m12[4 * r + 3] for r in range(3)], d


def disp16_of(end, s, cam, voxel_size, variant=None):
    code, axis, cell, k, na, ad = end
    if code != HIT or k < 1:
        return FILTERED
    focal, _, _, baseline = cam
    vs = float(np.float32(voxel_size))
    if variant == "z_ray":
        z = ((float(na) * math.sqrt(float(s.S))) / float(ad)) / 256.0 * vs
    else:
        num, den = float(na) * vs * 64.0, float(ad) * s.m
        z = num / den if num else 0.0
    if z == 0.0:
        return FILTERED  # a crossing at n = 0: the quotient is infinite and fails the range
    v = (focal * baseline) / z * 16.0 + 0.5
    if not _finite(v):
        return FILTERED
    d16 = math.floor(v)
    return int(d16) if 1.0 <= d16 <= 32767.0 else FILTERED


def raycast(words, origin, dims, width, height, cam, m12, max_range, min_step, voxel_size, route="a", variant=None, coarse=None):
    """cam = (focal, cx, cy, baseline); m12: 12 floats, camera -> world.  (disp16 int16 (H, W), cell uint32 (H, W), seven counts)."""
    vol = Volume(words, dims, coarse)
    m12 = [float(v) for v in np.asarray(m12, np.float64).reshape(12)]
    disp = np.full((height, width), FILTERED, np.int16)
    cell = np.full((height, width), NO_CELL, np.uint32)
    counts = [0] * 7
    mr = float(np.float32(max_range))
    for y in range(height):
        for x in range(width):
            o, d = pixel_ray(m12, cam, x, y)
            s = setup_b(o, d, mr, voxel_size, origin) if route == "b" else setup_a(o, d, mr, voxel_size, origin, variant)
            if s is None:
                counts[REJECTED] += 1
                continue
            end = walk_b(s, vol, min_step) if route == "b" else (walk_skip(s, vol, min_step)[0] if route == "skip" else walk_a(s, vol, min_step, variant))
            counts[end[0]] += 1
            counts[5] += end[3]
            v = disp16_of(end, s, cam, voxel_size, variant)
            if v != FILTERED:
                disp[y, x], cell[y, x] = v, end[2]
                counts[6] += 1
    return disp, cell, counts


def origin_of(T, voxel_size, dims):
    """The locate's step c."""
    vs = float(np.float32(voxel_size))
    return tuple(int(math.floor(T[r] / vs)) - dims[r] // 2 for r in range(3))
