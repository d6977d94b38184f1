"""Restatement of the voxel map distance field (include/svo.h, "Voxel map distance field"), by two routes that share no
code and neither of which copies the kernels' search:

  brute(occ, max_dist)  every cell against the list of sources, in numpy integers; the tie is the `min` over the bit numbers of the
                        sources that attain the minimum.  For volumes of up to about 50,000 cells.  The misreadings of the rules
                        are its `variant=`.
  sweep(occ, max_dist)  whole-array: per axis, the minimum over shifted copies of the array of (value + shift^2, bit number) keys.

occ is a bool array of shape (d2, d1, d0), so that its flat order is the bit number B = j0 + d0*(j1 + d1*j2).  Both return
(dist2 uint16, nearest uint32) of that shape.  finish() turns them into rules 4 to 6, field() runs it all from the volume's words,
query() restates rule 9.
"""
import numpy as np

NONE16 = 0xFFFF
NONE32 = 0xFFFFFFFF
LIMIT = 1048560.0
FREE, COLLIDES, OUTSIDE, REJECTED = 0, 1, 2, 3
VARIANTS = ("tie_larger", "lt_cap", "cube", "chessboard", "manhattan", "left_only", "none_sources", "swap_d1_d2", "row_wrap")
Sphere = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("radius", np.float32)])
SphereHit = np.dtype([("cell", np.uint32), ("dist2", np.uint32), ("clearance", np.float32), ("code", np.uint32)])


def unpack_bits(words, dims):
    """The volume's little-endian u64 words as a bool array (d2, d1, d0)."""
    d0, d1, d2 = (int(v) for v in dims)
    b = np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")
    return b[:d0 * d1 * d2].reshape(d2, d1, d0).astype(bool)


def pack_bits(occ):
    """A bool array (d2, d1, d0), d0 a multiple of 64, as the volume's u64 words."""
    return np.packbits(np.ascontiguousarray(occ).reshape(-1), bitorder="little").view("<u8").astype(np.uint64)


def r2_of(inflate_radius, voxel_size, max_dist):
    """Rule 4's R2: floor((r / vs)^2) in doubles, each f32 widened first, clamped to max_dist^2; an overflow takes the clamp."""
    with np.errstate(over="ignore"):
        rc = np.float64(np.float32(inflate_radius)) / np.float64(np.float32(voxel_size))
        q = rc * rc
    cap = float(max_dist * max_dist)
    return int(np.floor(q)) if q < cap else int(cap)


def brute(occ, max_dist, variant=None, chunk=1024):
    assert variant is None or variant in VARIANTS
    occ = np.asarray(occ, bool)
    d2_, d1_, d0_ = occ.shape
    if variant == "swap_d1_d2":  # the bit number read as j0 + d0*(j2 + d2*j1): the same words are another volume
        a, b = brute(occ.reshape(d1_, d2_, d0_), max_dist)
        return a.reshape(occ.shape), b.reshape(occ.shape)
    cap = max_dist * max_dist
    n = occ.size
    dist2, nearest = np.full(n, NONE16, np.uint16), np.full(n, NONE32, np.uint32)
    src = np.argwhere(occ).astype(np.int64)  # rows (j2, j1, j0)
    if len(src):
        sbit = src[:, 2] + d0_ * (src[:, 1] + d1_ * src[:, 0])
        cells = np.arange(n, dtype=np.int64)
        c0, c1, c2 = cells % d0_, cells // d0_ % d1_, cells // (d0_ * d1_)
        for lo in range(0, n, chunk):
            s = slice(lo, min(lo + chunk, n))
            o0, o1, o2 = (np.abs(c[s, None] - src[None, :, k]) for c, k in ((c0, 2), (c1, 1), (c2, 0)))
            if variant == "chessboard":
                tot = np.maximum(np.maximum(o0, o1), o2) ** 2
            elif variant == "manhattan":
                tot = (o0 + o1 + o2) ** 2
            else:
                tot = o0 * o0 + o1 * o1 + o2 * o2
            if variant == "row_wrap":  # axis 0 runs on: a source k bits away in the words counts as k cells away
                lin = np.abs(cells[s, None] - sbit[None, :])
                tot = np.where(lin <= max_dist, np.minimum(tot, lin * lin), tot)
            if variant == "cube":
                ok = (o0 <= max_dist) & (o1 <= max_dist) & (o2 <= max_dist)
            elif variant == "lt_cap":
                ok = tot < cap
            else:
                ok = tot <= cap
            if variant == "left_only":
                ok &= src[None, :, 2] <= c0[s, None]
            big = np.int64(1) << 40
            tot = np.where(ok, tot, big)
            m = tot.min(axis=1)
            some = m < big
            attain = tot == m[:, None]
            if variant == "tie_larger":
                at = np.where(attain, sbit[None, :], -1).max(axis=1)
            else:
                at = np.where(attain, sbit[None, :], big).min(axis=1)
            assert int(m[some].max(initial=0)) < NONE16
            dist2[s] = np.where(some, m, NONE16).astype(np.uint16)
            nearest[s] = np.where(some, at, NONE32).astype(np.uint32)
    if variant == "none_sources":
        nearest[dist2 == 0] = NONE32
        dist2[dist2 == 0] = NONE16
    return dist2.reshape(occ.shape), nearest.reshape(occ.shape)


def sweep(occ, max_dist):
    occ = np.asarray(occ, bool)
    d2_, d1_, d0_ = occ.shape
    cap, big = max_dist * max_dist, np.int64(1) << 62
    key = np.where(occ, np.arange(occ.size, dtype=np.int64).reshape(occ.shape), big)  # value << 32 | bit number
    for ax in (2, 1, 0):  # axis 0 of the volume is the array's last
        L = key.shape[ax]
        out = key.copy()
        for k in range(1, min(max_dist, L - 1) + 1):
            add = np.int64(k * k) << 32
            near, far = [slice(None)] * 3, [slice(None)] * 3
            near[ax], far[ax] = slice(0, L - k), slice(k, L)
            near, far = tuple(near), tuple(far)
            out[near] = np.minimum(out[near], key[far] + add)  # the entry k further on
            out[far] = np.minimum(out[far], key[near] + add)   # the entry k further back
        out[(out >> 32) > cap] = big  # everything at or above `big` too
        key = out
    some = key < big
    dist2 = np.where(some, key >> 32, NONE16).astype(np.uint16)
    nearest = np.where(some, key & 0xFFFFFFFF, NONE32).astype(np.uint32)
    return dist2, nearest


def clearance_of(dist2, voxel_size):
    """Rule 5 for uint16 dist2 (NONE16: +inf)."""
    d = np.asarray(dist2)
    with np.errstate(invalid="ignore"):
        c = (np.sqrt(d.astype(np.float64)) * np.float64(np.float32(voxel_size))).astype(np.float32)
    return np.where(d == NONE16, np.float32(np.inf), c).astype(np.float32)


def finish(dist2, nearest, r2, voxel_size):
    """Rules 4 to 6 from rules 2 and 3: flat arrays, the inflated words and the four counts."""
    d = dist2.reshape(-1)
    infl = d <= r2  # NONE16 is above every R2
    counts = [int((d == 0).sum()), int(((d != 0) & (d != NONE16)).sum()), int((d == NONE16).sum()), int(infl.sum())]
    return {"dist2": d.copy(), "nearest": nearest.reshape(-1).copy(), "clearance": clearance_of(d, voxel_size), "inflated": pack_bits(infl),
            "counts": counts, "r2": r2}


def field(words, dims, max_dist, inflate_radius, voxel_size, route="sweep", variant=None):
    occ = unpack_bits(words, dims)
    d, a = sweep(occ, max_dist) if route == "sweep" else brute(occ, max_dist, variant)
    return finish(d, a, r2_of(inflate_radius, voxel_size, max_dist), voxel_size)


def query(dist2, origin, dims, spheres, voxel_size):
    """Rule 9: (SphereHit records, the six counts) for Sphere records over a flat uint16 field."""
    s = np.asarray(spheres, dtype=Sphere).reshape(-1)
    n = len(s)
    hits = np.zeros(n, SphereHit)
    hits["cell"], hits["dist2"], hits["clearance"], hits["code"] = NONE32, NONE32, np.inf, REJECTED
    vs = np.float64(np.float32(voxel_size))
    dist2 = np.asarray(dist2).reshape(-1)
    beyond = 0
    with np.errstate(all="ignore"):
        rad = s["radius"].astype(np.float64)
        q = np.stack([s[k].astype(np.float64) / vs for k in ("x", "y", "z")], axis=1) if n else np.zeros((0, 3))
        ok = (rad >= 0) & np.isfinite(rad) & np.all((q >= -LIMIT) & (q < LIMIT), axis=1)
        for i in np.flatnonzero(ok):
            j = [int(np.floor(q[i, r])) - int(origin[r]) for r in range(3)]
            if any(j[r] < 0 or j[r] >= int(dims[r]) for r in range(3)):
                hits["code"][i] = OUTSIDE
                continue
            B = j[0] + int(dims[0]) * (j[1] + int(dims[1]) * j[2])
            d = int(dist2[B])
            wide = NONE32 if d == NONE16 else d
            beyond += d == NONE16
            rc = rad[i] / vs
            hits[i] = (B, wide, clearance_of(np.uint16(d), voxel_size), COLLIDES if float(wide) <= np.floor(rc * rc) else FREE)
    code = hits["code"]
    return hits, [n, int((code == FREE).sum()), int((code == COLLIDES).sum()), int((code == OUTSIDE).sum()), int((code == REJECTED).sum()), int(beyond)]
