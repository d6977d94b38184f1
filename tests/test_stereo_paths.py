"""Every StereoBM matcher of the library against an independent integer restatement (tests/stereo_bm_ref.py), on scenes that reach every
decision of the function: the texture threshold on both sides, the uniqueness test at equality, winners at d = 0 and at d = ndisp - 1
(the mirrored borders of the sub-pixel step), ties between adjacent disparities, sub-pixel terms of both signs.

Matchers: stereo_dense_kernel (Context.stereo_bm), stereo_dense_batch_kernel (Context.stereo_bm_batch) and the three compiled forms of
stereo_at_block_t (Context.stereo_disparity_at): <21, 48>, <0, 0> with block 21 (packed SAD, run-time range), <0, 0> with block < 21
(byte loop).  All integer arithmetic: every comparison is ==.

Sizes: W = 0, 1 and 63 (mod 64), H = 0, 1 and 7 (mod 8), five odd heights (the prefilter's leftover row), two to four tile columns and
16 to 21 tile rows of the dense kernels; the 21 x 21 entries have H = 7 (mod 8), which gives band 8 — the last one takes the rows left
over — six or seven rows of windows that lie in it alone.  ndisp + 1 (mod 3 slots per pass) = 1, 2, 2, 0, 2, 2."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import stereo_bm_ref as SR

gpu = pytest.mark.gpu

#        ndisp block   H    W  seed
GRID = {
    "G1": (48, 21, 167, 191, 2),   # the <21, 48> instance
    "G2": (64, 21, 167, 193, 6),   # packed SAD, run-time range, deepest sRp reads
    "G3": (16, 21, 159, 128, 6),   # packed SAD, run-time range
    "G4": (32, 11, 137, 129, 3),   # byte loop
    "G5": (64, 7, 152, 192, 2),    # byte loop
    "G6": (16, 5, 121, 127, 3),    # byte loop
}
IDS = list(GRID)
# the inputs of test_frontend.test_hip_stereo_odd_sizes
KRON = [((75, 131), 32, 11), ((64, 200), 64, 21), ((61, 90), 16, 5)]
# a single valid column: W = ndisp - 1 + block
NARROW = {"G1": (48, 21, 131, 68, 7), "G6": (16, 5, 130, 20, 7)}

FLOORS = {"texture": 500, "uniq": 500, "d_max": 500, "d_zero": 500, "uniq_edge": 100, "neg": 500, "pos": 500, "peq": 100, "tie_adj": 1}
SPARSE_FLOOR = 20  # of each of texture, uniq, d_max, d_zero among the sparse matcher's points


class Case:
    """A scene, its reversed twin, and the reference's map / decision masks of both: computed once, never modified."""

    def __init__(self, nd, blk, h, w, seed):
        self.nd, self.blk, self.h, self.w = nd, blk, h, w
        self.L, self.R = SR.scene(h, w, nd, seed)
        self.Lr, self.Rr = SR.reverse_bands(self.L), SR.reverse_bands(self.R)
        self.ref, self.masks = SR.categories(self.L, self.R, nd, blk)
        self.ref_r, self.masks_r = SR.categories(self.Lr, self.Rr, nd, blk)
        self.stats = {k: int(v.sum()) for k, v in self.masks.items()}
        for a in (self.L, self.R, self.Lr, self.Rr, self.ref, self.ref_r, *self.masks.values(), *self.masks_r.values()):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _case(gid, narrow=False):
    return Case(*(NARROW if narrow else GRID)[gid])


def _kron_pair(shape):
    rng = np.random.default_rng(shape[0])
    tex = np.kron(rng.integers(0, 255, (shape[0] // 3 + 1, shape[1] // 3 + 30)), np.ones((3, 3))).astype(np.uint8)
    return np.ascontiguousarray(tex[:shape[0], 12:12 + shape[1]]), np.ascontiguousarray(tex[:shape[0], 19:19 + shape[1]])


def _points(c):
    """The sparse matcher's points: a lattice of about 2,000 (+0.37: truncation), the corners of the valid rectangle with their outside
    neighbours, and points outside the image on every side."""
    x0, x1, y0, y1 = SR.valid_rect(c.h, c.w, c.nd, c.blk)
    step = (c.w * c.h / 2000.0) ** 0.5
    ys, xs = np.meshgrid(np.arange(0, c.h, step), np.arange(0, c.w, step), indexing="ij")
    pts = [np.stack([xs.ravel(), ys.ravel()], 1) + 0.37]
    corners = []
    for cx, ox in ((x0, x0 - 1), (x1 - 1, x1)):
        for cy, oy in ((y0, y0 - 1), (y1 - 1, y1)):
            corners += [(cx, cy), (ox, cy), (cx, oy), (ox, oy)]
    corners = np.array(corners, np.float64)
    pts += [corners, corners + 0.37, corners + 0.99]
    pts.append(np.array([(-0.5, -0.5), (c.w - 0.5, c.h - 0.5), (c.w + 3, 5), (5, -2)], np.float64))
    xy = np.concatenate(pts).astype(np.float32)
    assert len(xy) <= 2500
    return xy


def _points_hit(c, xy):
    """How many of the points fall on a pixel of each decision category (from the reference alone)."""
    x, y = np.trunc(xy[:, 0]).astype(int), np.trunc(xy[:, 1]).astype(int)
    ok = (x >= 0) & (x < c.w) & (y >= 0) & (y < c.h)
    return {k: int(c.masks[k][y[ok], x[ok]].sum()) for k in SR.STAT_KEYS}


def _report(what, got, ref, masks):
    """Per decision category: how many of its pixels differ."""
    diff = got != ref
    print(what, "differing pixels", int(diff.sum()), "of", diff.size, "outside the valid rectangle",
          int((diff & ~(masks["texture"] | masks["uniq"] | masks["kept"])).sum()))
    for k in SR.STAT_KEYS:
        print("   %-13s %6d of %6d differ" % (k, int((diff & masks[k]).sum()), int(masks[k].sum())))


def _strided(imgs, pad, seed):
    """imgs (B, H, W) -> flat buffer with row_stride = W + pad, image_stride = row_stride * H + 64, the gaps filled with noise."""
    B, H, W = imgs.shape
    rs = W + pad
    ist = rs * H + 64
    buf = np.random.default_rng(seed).integers(0, 256, B * ist, dtype=np.uint8)
    for b in range(B):
        buf[b * ist:b * ist + rs * H].reshape(H, rs)[:, :W] = imgs[b]
    return buf, rs, ist


def _batched(ctx, c):
    """stereo_bm_batch on (scene, reversed scene), strided inputs, sentinel-filled output -> (2, H, W) int16."""
    import torch
    bl, rs, ist = _strided(np.stack([c.L, c.Lr]), 5, 1)
    br, _, _ = _strided(np.stack([c.R, c.Rr]), 5, 2)
    assert rs == c.w + 5 and ist == rs * c.h + 64
    dl, dr = torch.from_numpy(bl).cuda(), torch.from_numpy(br).cuda()
    out = torch.full((2, c.h, c.w), 12345, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.stereo_bm_batch(dl.data_ptr(), dr.data_ptr(), 2, c.w, c.h, rs, ist, out.data_ptr(), c.nd, c.blk)
    ctx.sync()
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("gid", IDS)
def test_reference_equals_the_oracle(gid):
    """Two restatements of SURVEY A.2 by different routes (per-pixel window loops; cumulative-sum planes) give the same map, the same
    prefiltered image and the same samples."""
    c = _case(gid)
    assert np.array_equal(c.ref, O.stereo_bm(c.L, c.R, c.nd, c.blk))
    assert np.array_equal(c.ref_r, O.stereo_bm(c.Lr, c.Rr, c.nd, c.blk))
    for img in (c.L, c.R):
        assert np.array_equal(SR.prefilter(img), O.stereo_prefilter(img))
    xy = _points(c)
    assert np.array_equal(SR.disparity_at(c.L, c.R, xy, c.nd, c.blk, c.ref).view(np.uint32), O.stereo_disparity_at(c.L, c.R, xy, c.nd, c.blk).view(np.uint32))
    if gid in NARROW:
        n = _case(gid, True)
        assert np.array_equal(n.ref, O.stereo_bm(n.L, n.R, n.nd, n.blk))
        assert np.array_equal(n.ref_r, O.stereo_bm(n.Lr, n.Rr, n.nd, n.blk))


@pytest.mark.parametrize("shape,nd,blk", KRON)
def test_reference_equals_the_oracle_on_shifted_noise(shape, nd, blk):
    """The input of test_hip_stereo_odd_sizes.  Its counts: texture 0, d_max 0, d_zero 0, tie_adj 0 at every shape; uniq 0, 0, 99."""
    L, R = _kron_pair(shape)
    st = {}
    assert np.array_equal(SR.stereo_bm(L, R, nd, blk, st), O.stereo_bm(L, R, nd, blk))
    print(shape, st)
    assert st["kept"] > 3000 and st["texture"] == 0 and st["d_max"] == 0 and st["d_zero"] == 0


@pytest.mark.parametrize("gid", IDS)
def test_scenes_reach_every_decision(gid):
    """Floors on the reference's own counts, over the valid rectangle of each scene (conditions on the reference alone).

    Measured:
          texture t_edge  uniq u_edge   kept d_max d_zero tie_adj   neg   pos   peq | sparse points on texture / uniq / d_max / d_zero
      G1    1367    170  4193   1260  12668  2321   1165     133  5195  3376  4097 |  93 / 292 / 130 /  68
      G2    1256    107  3998   1342  10916  2082   1000     102  4580  2801  3535 |  86 / 243 / 122 /  60
      G3     931    127  2550    744   9446  1580    780     110  3883  2554  3009 |  87 / 250 / 155 /  66
      G4    1906     67  2107   1334   7163  1424   1023     118  2430  2052  2681 | 213 / 228 / 167 / 126
      G5    4124     98  3530   2613  10304  2272   1867      82  2996  2778  4530 | 286 / 247 / 154 / 136
      G6    3408     37  1963   1737   7265  1601   1350      15  1984  1948  3333 | 419 / 278 / 213 / 178
    Every u_edge pixel of the stripes has minimum 0 = threshold: it is rejected by the equality alone (744 to 2,591 pixels per scene
    come out kept if the test is < instead of <=).  What the scenes do NOT decide: a tie between ADJACENT disparities gives the same
    value whichever of the two wins (the sub-pixel term is -128 from the one, +128 from the other), so the choice of the first minimum
    shows only through the uniqueness neighbourhood, and no pixel here is rejected by s[mind - 2] or s[mind + 2] alone.
    The input the suite had before (3 x 3 block noise shifted by 7): texture 0, d_max 0, d_zero 0, tie_adj 0.
    """
    c = _case(gid)
    st = c.stats
    print(gid, st)
    x0, x1, y0, y1 = SR.valid_rect(c.h, c.w, c.nd, c.blk)
    assert sum(st[k] for k in ("texture", "uniq", "kept")) == (x1 - x0) * (y1 - y0)   # the three outcomes partition the rectangle
    assert st["neg"] + st["pos"] + st["peq"] == st["kept"]
    for k, floor in FLOORS.items():
        assert st[k] >= floor, (k, st[k], floor)
    if c.blk >= 7:
        assert st["texture_edge"] >= 10, st["texture_edge"]
    # a band that the reference filters wholesale would pass every equality test: the three noise bands come out with their shift.
    # A winner at d gives a value within 8 of 16 d (|sub-pixel term| <= 128); at the mirrored borders (bands 1, 2) the term is 0.
    # Windows that straddle two noise bands about evenly fail uniqueness (both shifts match half of the window): "mostly" = 80 %.
    for k, d in enumerate((0, c.nd - 1, c.nd // 3)):
        a, b = SR.band_rows(c.h)[k]
        v = c.ref[max(a, y0):b, x0:x1].astype(int)
        exact = ((v == 16 * d) | (v == 16 * d + 1)).mean()
        near = (np.abs(v - 16 * d) <= 8).mean()
        print("   band", k + 1, "d", d, "value 16d or 16d+1: %.3f   winner d: %.3f" % (exact, near))
        assert near >= 0.8, (k, near)
        assert exact >= (0.8 if k < 2 else 0.5), (k, exact)
    hit = _points_hit(c, _points(c))
    print("   sparse points on", {k: hit[k] for k in ("texture", "uniq", "d_max", "d_zero", "tie_adj")})
    for k in ("texture", "uniq", "d_max", "d_zero"):
        assert hit[k] >= SPARSE_FLOOR, (k, hit[k])


def test_single_valid_column_is_kept_by_the_reference():
    for gid in NARROW:
        n = _case(gid, True)
        x0, x1, _, _ = SR.valid_rect(n.h, n.w, n.nd, n.blk)
        assert x1 - x0 == 1
        assert n.stats["kept"] >= 1 and (n.ref[:, x0] != SR.FILTERED).any()
        assert (np.delete(n.ref, x0, 1) == SR.FILTERED).all()


# ------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("gid", IDS)
def test_dense_map_reaches_every_decision(ctx, gid):
    c = _case(gid)
    got = ctx.stereo_bm(c.L, c.R, c.nd, c.blk)
    if not np.array_equal(got, c.ref):
        _report("stereo_bm " + gid, got, c.ref, c.masks)
    assert np.array_equal(got, c.ref)


@gpu
@pytest.mark.parametrize("gid", IDS)
def test_batched_dense_map_reaches_every_decision(ctx, gid):
    c = _case(gid)
    got = _batched(ctx, c)
    for b, (ref, masks, L, R) in enumerate(((c.ref, c.masks, c.L, c.R), (c.ref_r, c.masks_r, c.Lr, c.Rr))):
        if not np.array_equal(got[b], ref):
            _report("stereo_bm_batch %s pair %d" % (gid, b), got[b], ref, masks)
        assert np.array_equal(got[b], ref), b
        assert np.array_equal(got[b], ctx.stereo_bm(L, R, c.nd, c.blk)), b


@gpu
@pytest.mark.parametrize("gid", IDS)
def test_sparse_matcher_all_forms(ctx, gid):
    c = _case(gid)
    xy = _points(c)
    hit = _points_hit(c, xy)
    for k in ("texture", "uniq", "d_max", "d_zero"):
        assert hit[k] >= SPARSE_FLOOR, (k, hit[k])
    want = SR.disparity_at(c.L, c.R, xy, c.nd, c.blk, c.ref)
    got = ctx.stereo_disparity_at(c.L, c.R, xy, c.nd, c.blk)
    bad = got.view(np.uint32) != want.view(np.uint32)
    if bad.any():
        x, y = np.trunc(xy[:, 0]).astype(int), np.trunc(xy[:, 1]).astype(int)
        inside = (x >= 0) & (x < c.w) & (y >= 0) & (y < c.h)
        print("stereo_disparity_at", gid, "differing points", int(bad.sum()), "of", len(xy), "outside the image", int((bad & ~inside).sum()))
        for k in SR.STAT_KEYS:
            on = np.zeros(len(xy), bool)
            on[inside] = c.masks[k][y[inside], x[inside]]
            print("   %-13s %5d of %5d differ" % (k, int((bad & on).sum()), int(on.sum())))
        print("   first", xy[bad][:8].tolist(), got[bad][:8].tolist(), want[bad][:8].tolist())
    assert not bad.any()


@gpu
@pytest.mark.parametrize("gid", list(NARROW))
def test_single_valid_column(ctx, gid):
    n = _case(gid, True)
    x0, x1, y0, y1 = SR.valid_rect(n.h, n.w, n.nd, n.blk)
    assert x1 - x0 == 1 and n.stats["kept"] >= 1
    got = ctx.stereo_bm(n.L, n.R, n.nd, n.blk)
    if not np.array_equal(got, n.ref):
        _report("stereo_bm narrow " + gid, got, n.ref, n.masks)
    assert np.array_equal(got, n.ref)
    gb = _batched(ctx, n)
    assert np.array_equal(gb[0], n.ref) and np.array_equal(gb[1], n.ref_r)
    ys = np.arange(-1, n.h + 1)
    xy = np.concatenate([np.stack([np.full(len(ys), x), ys], 1) for x in (x0 - 1, x0, x0 + 1)]).astype(np.float32) + np.float32(0.37)
    want = SR.disparity_at(n.L, n.R, xy, n.nd, n.blk, n.ref)
    assert (want != -1.0).any()
    got = ctx.stereo_disparity_at(n.L, n.R, xy, n.nd, n.blk)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
