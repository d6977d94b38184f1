"""a2/a3/a4 pyramid, pyrLK and the survivor filter: a plain restatement in Python ints and numpy, independent of the oracle and
of the library.

`oracle/ora_lk.cpp` and `csrc/lk.hip` are by one hand and share one structure (a per-point loop, Scharr derivatives formed on the
fly, a reflecting pixel fetch), so a misreading of SURVEY.md Appendix A.3 common to both cannot show between them.  This file
states the same function again from SURVEY A.3, the arithmetic declared in the header of `oracle/ora_lk.cpp` and the reference's
`FeatureTracker::track_features`, and takes another route wherever bit-exactness leaves one:

  pyramid      whole-array numpy: one gather through an index map, five shifted slices per axis, (s + 128) >> 8
  REFLECT_101  a closed form over the period 2n - 2 (any distance outside; level 3 of an 8 x 8 image is 1 x 1), no loop
  per level    as OpenCV lays it out: ONE image padded by winSize with REFLECT_101 (one more column and row for the bilinear
               neighbour) and ONE whole-level int16 Scharr image, padded with constant 0; windows are slices of the two
  patches      four shifted 21 x 21 slices times the four weights, whole-array int64
  sums         int64 array sums (exact), then int -> float64 -> float32; float64 is exact below 2^53 and that bound is asserted
  f32          every operation is one np.float32 statement in the declared order; nothing is fused
  exits        the reference's double expressions themselves
  bounds       taken on the floored FLOAT before any conversion to int (the declared domain is finite coordinates below 2^20)

The scalar 2 x 2 solve and the exit rules are a handful of f32 statements whose order is declared: they can only be written as
declared, so a misreading of those declarations themselves is not something this file can show.

Every call returns a dictionary of counters (COUNTERS), one per outcome of every decision, plus the largest window sums it met.
`mutation=` selects one deliberate misreading (MUTATIONS); tests/test_lk_paths.py shows that each changes some scene's bytes.
The `stage_*` / `tile_*` counters follow the kernel's 32 x 32 staged region and 24 x 24 source tile only to COUNT which scenes
move them; they never touch a value.
"""
import numpy as np

F = np.float32
WIN, HALF, LEVELS, MAX_ITER = 21, 10, 4, 30
MIN_EIG = F(1e-2)             # the invoker keeps minEigThreshold as a float
EPS = 0.01                    # TermCriteria epsilon, a double
FLT_SCALE = F(2.0 ** -20)
FLT_EPSILON = F(2.0 ** -23)
FB_MAX = 2.0
MAX_PARALLAX = F(200.0)
ONE, W14, HALF_F, TWO = F(1.0), F(16384.0), F(HALF), F(2.0)
STAGE_MARGIN, STAGE_SIZE, TILE = 5, 32, 24  # the kernel's, for the stage_* / tile_* counters only

MUTATIONS = ("round_half_away", "wrap_int32", "parallax_ge", "fb_le", "deriv_reflect", "border_replicate", "no_half_step",
             "skip_sets_status", "mean_over_kept", "pairwise_sum", "no_final_check")
COUNTERS = (
    "tmpl_in", "tmpl_out_coarse", "tmpl_out_l0",
    "eig_ok", "eig_low_l3", "eig_low_l12", "eig_low_l0", "det_small_alone", "tracked_l0_after_l3_skip",
    "iter_in", "iter_out_coarse", "iter_out_l0", "final_ok", "final_out",
    "exit_eps", "exit_osc", "exit_cap", "status1_after_coarse_skip", "status1_after_coarse_break",
    "band_stop", "band_go", "osc_near_below", "osc_near_above",
    "weight_tie", "weight_tie_l0_tmpl",
    "A_over_2p31", "A_over_2p32", "b_over_2p31", "b_over_2p32_pos", "b_over_2p32_neg",
    "stage_restage", "stage_xpos", "stage_xneg", "stage_ypos", "stage_yneg", "stage_in_to_reflect", "stage_reflect_to_in",
    "tile_x_end_at_w", "tile_x_end_w_minus_1", "tile_x_end_w_plus_1", "tile_y_end_at_h", "tile_y_end_h_minus_1", "tile_y_end_h_plus_1",
    "status1_0", "status2_0", "fb_fail", "fb_ok", "fb_is_2", "parallax_drop", "parallax_keep", "parallax_is_200")


def new_record():
    rec = {k: 0 for k in COUNTERS}
    rec["max_abs_sum"] = 0
    rec["max_abs_3rows"] = 0
    return rec


# ---------------------------------------------------------------------------------------------------------------- pyramid
def border_index(i, n, replicate=False):
    """REFLECT_101 of any integer index into [0, n): a closed form over the period 2n - 2 (replicate: the mutation's clamp)."""
    i = np.asarray(i, np.int64)
    if replicate:
        return np.clip(i, 0, n - 1)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    m = np.mod(i, p)
    return np.where(m >= n, p - m, m)


def pyr_down(src):
    h, w = src.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    p = src.astype(np.int64)[:, border_index(np.arange(-2, 2 * dw + 1), w)]
    rows = sum(k[t] * p[:, t:t + 2 * dw:2][:, :dw] for t in range(5))
    p = rows[border_index(np.arange(-2, 2 * dh + 1), h), :]
    s = sum(k[t] * p[t:t + 2 * dh:2, :][:dh, :] for t in range(5))
    return ((s + 128) >> 8).astype(np.uint8)


def build_pyramid(img, levels=LEVELS):
    out = [np.ascontiguousarray(img, np.uint8)]
    assert out[0].ndim == 2
    for _ in range(1, levels):
        out.append(pyr_down(out[-1]))
    return out


# ---------------------------------------------------------------------------------------------------------- level planes
class Plane:
    """One pyramid level as OpenCV holds it: `pad[y + WIN, x + WIN]` is the image at (x, y), REFLECT_101 outside; `dx`, `dy`
    are the int16 Scharr images in the same frame, 0 outside the image."""

    def __init__(self, img, mutation):
        h, w = img.shape
        self.w, self.h = w, h
        rep = mutation == "border_replicate"
        ys, xs = border_index(np.arange(-WIN, h + WIN + 1), h, rep), border_index(np.arange(-WIN, w + WIN + 1), w, rep)
        self.pad = img[np.ix_(ys, xs)].astype(np.int64)
        # Scharr [3 10 3] x [-1 0 1]: its own taps reflect inside the image
        e = img[np.ix_(border_index(np.arange(-1, h + 1), h), border_index(np.arange(-1, w + 1), w))].astype(np.int64)
        smooth_v = 3 * e[:-2, :] + 10 * e[1:-1, :] + 3 * e[2:, :]
        diff_v = e[2:, :] - e[:-2, :]
        dx = (smooth_v[:, 2:] - smooth_v[:, :-2]).astype(np.int16)
        dy = (3 * diff_v[:, :-2] + 10 * diff_v[:, 1:-1] + 3 * diff_v[:, 2:]).astype(np.int16)
        if mutation == "deriv_reflect":
            yr, xr = border_index(np.arange(-WIN, h + WIN + 1), h), border_index(np.arange(-WIN, w + WIN + 1), w)
            self.dx, self.dy = dx[np.ix_(yr, xr)].astype(np.int64), dy[np.ix_(yr, xr)].astype(np.int64)
        else:
            self.dx = np.zeros(self.pad.shape, np.int64)
            self.dy = np.zeros(self.pad.shape, np.int64)
            self.dx[WIN:WIN + h, WIN:WIN + w] = dx
            self.dy[WIN:WIN + h, WIN:WIN + w] = dy

    def window(self, plane, ix, iy):
        """(WIN + 1)^2 samples whose top-left is image position (ix, iy), -WIN <= ix < w."""
        return plane[iy + WIN:iy + 2 * WIN + 1, ix + WIN:ix + 2 * WIN + 1]


def planes(img, mutation=None):
    return [Plane(lv, mutation) for lv in build_pyramid(img)]


# ------------------------------------------------------------------------------------------------------------- one point
def _round(v, mutation):
    """cvRound of a non-negative f32: half to even (the mutation: half away from zero)."""
    if mutation == "round_half_away":
        return int(np.floor(np.float64(v) + 0.5))
    return int(np.rint(v))


def _weights(a, b, rec, mutation, key=None):
    oma = ONE - a
    omb = ONE - b
    v00 = oma * omb
    v00 = v00 * W14
    v01 = a * omb
    v01 = v01 * W14
    v10 = oma * b
    v10 = v10 * W14
    for v in (v00, v01, v10):
        if float(v) - float(np.floor(v)) == 0.5:
            rec["weight_tie"] += 1
            if key:
                rec[key] += 1
    i00, i01, i10 = _round(v00, mutation), _round(v01, mutation), _round(v10, mutation)
    return i00, i01, i10, (1 << 14) - i00 - i01 - i10


def _bilinear(win, wts, shift):
    i00, i01, i10, i11 = wts
    v = win[:-1, :-1] * i00 + win[:-1, 1:] * i01 + win[1:, :-1] * i10 + win[1:, 1:] * i11
    return (v + (1 << (shift - 1))) >> shift


def _sum_f32(prod, rec, mutation, kind):
    """Exact sum of a 21 x 21 int64 array -> double -> float, times 2^-20."""
    rows = prod.sum(axis=1)
    s = int(rows.sum())
    three = int(np.abs(rows[:-2] + rows[1:-1] + rows[2:]).max())
    rec["max_abs_sum"] = max(rec["max_abs_sum"], abs(s))
    rec["max_abs_3rows"] = max(rec["max_abs_3rows"], three)
    if abs(s) >= 1 << 31:
        rec[kind + "_over_2p31"] += 1
    if abs(s) >= 1 << 32:
        rec[kind + "_over_2p32" if kind == "A" else (kind + "_over_2p32_pos" if s > 0 else kind + "_over_2p32_neg")] += 1
    if mutation == "wrap_int32":
        s = (s + (1 << 31)) % (1 << 32) - (1 << 31)
    assert abs(s) < 1 << 53
    v = F(np.float64(s))
    return v * FLT_SCALE


def _outside(fx, fy, w, h):
    """floor(position) outside [-WIN, w) x [-WIN, h), on the floored floats."""
    return bool(fx < -WIN or fx >= w or fy < -WIN or fy >= h)


def _stage_counters(rec, st, inx, iny, w, h):
    """The kernel's staged 32 x 32 region, followed only to count restages (st: [staged, rx0, ry0, inside])."""
    if st[0] and st[1] <= inx <= st[1] + 2 * STAGE_MARGIN and st[2] <= iny <= st[2] + 2 * STAGE_MARGIN:
        return
    rx0, ry0 = inx - STAGE_MARGIN, iny - STAGE_MARGIN
    inside = rx0 >= 0 and ry0 >= 0 and rx0 + STAGE_SIZE <= w and ry0 + STAGE_SIZE <= h
    if st[0]:
        rec["stage_restage"] += 1
        rec["stage_xpos"] += inx > st[1] + 2 * STAGE_MARGIN
        rec["stage_xneg"] += inx < st[1]
        rec["stage_ypos"] += iny > st[2] + 2 * STAGE_MARGIN
        rec["stage_yneg"] += iny < st[2]
        rec["stage_in_to_reflect"] += st[3] and not inside
        rec["stage_reflect_to_in"] += inside and not st[3]
    st[:] = [True, rx0, ry0, inside]


def _tile_counters(rec, ipx, ipy, w, h):
    x0, y0 = ipx - 1, ipy - 1
    if y0 >= 0 and y0 + TILE <= h and x0 >= 0:
        for d, key in ((0, "tile_x_end_at_w"), (-1, "tile_x_end_w_minus_1"), (1, "tile_x_end_w_plus_1")):
            rec[key] += x0 + TILE == w + d
    if x0 >= 0 and x0 + TILE <= w and y0 >= 0:
        for d, key in ((0, "tile_y_end_at_h"), (-1, "tile_y_end_h_minus_1"), (1, "tile_y_end_h_plus_1")):
            rec[key] += y0 + TILE == h + d


def lk_point(PA, PB, px0, py0, rec, mutation=None):
    """One point from the planes PA (template) to PB (target) through all levels: (x, y, status), x and y np.float32."""
    px0, py0 = F(px0), F(py0)
    assert np.isfinite(px0) and np.isfinite(py0) and abs(px0) < 2 ** 20 and abs(py0) < 2 ** 20
    status = 1
    nx = ny = F(0)
    l3_skipped = coarse_skip = coarse_break = False
    for level in range(LEVELS - 1, -1, -1):
        I, J = PA[level], PB[level]
        sc = F(1.0 / (1 << level))
        pxl = px0 * sc
        pyl = py0 * sc
        if level == LEVELS - 1:
            nx, ny = pxl, pyl
        else:
            nx = nx * TWO
            ny = ny * TWO
        pxl = pxl - HALF_F
        pyl = pyl - HALF_F
        fpx, fpy = np.floor(pxl), np.floor(pyl)
        if _outside(fpx, fpy, I.w, I.h):
            rec["tmpl_out_l0" if level == 0 else "tmpl_out_coarse"] += 1
            if level == 0 or mutation == "skip_sets_status":
                status = 0
            continue
        rec["tmpl_in"] += 1
        ipx, ipy = int(fpx), int(fpy)
        _tile_counters(rec, ipx, ipy, I.w, I.h)
        a = pxl - fpx
        b = pyl - fpy
        wts = _weights(a, b, rec, mutation, "weight_tie_l0_tmpl" if level == 0 else None)
        Iw = _bilinear(I.window(I.pad, ipx, ipy), wts, 9).astype(np.int16).astype(np.int64)
        Ix = _bilinear(I.window(I.dx, ipx, ipy), wts, 14).astype(np.int16).astype(np.int64)
        Iy = _bilinear(I.window(I.dy, ipx, ipy), wts, 14).astype(np.int16).astype(np.int64)
        A11 = _sum_f32(Ix * Ix, rec, mutation, "A")
        A12 = _sum_f32(Ix * Iy, rec, mutation, "A")
        A22 = _sum_f32(Iy * Iy, rec, mutation, "A")
        p = A11 * A22
        q = A12 * A12
        D = p - q
        dif = A11 - A22
        t = dif * dif
        u = F(4.0) * A12
        u = u * A12
        t = t + u
        t = np.sqrt(t)
        tr = A22 + A11
        tr = tr - t
        min_eig = tr / F(2 * WIN * WIN)
        if min_eig < MIN_EIG or D < FLT_EPSILON:
            if not min_eig < MIN_EIG:
                rec["det_small_alone"] += 1
            else:
                rec["eig_low_l0" if level == 0 else ("eig_low_l3" if level == LEVELS - 1 else "eig_low_l12")] += 1
            l3_skipped = l3_skipped or level == LEVELS - 1
            coarse_skip = coarse_skip or level > 0
            if level == 0 or mutation == "skip_sets_status":
                status = 0
            continue
        rec["eig_ok"] += 1
        if level == 0 and l3_skipped:
            rec["tracked_l0_after_l3_skip"] += 1
        D = ONE / D
        outx, outy = nx, ny
        nx = nx - HALF_F
        ny = ny - HALF_F
        pdx = pdy = F(0)
        stage = [False, 0, 0, False]
        exit_kind = "exit_cap"
        for j in range(MAX_ITER):
            fnx, fny = np.floor(nx), np.floor(ny)
            if _outside(fnx, fny, J.w, J.h):
                rec["iter_out_l0" if level == 0 else "iter_out_coarse"] += 1
                if level == 0:
                    status = 0
                coarse_break = coarse_break or level > 0
                exit_kind = None
                break
            rec["iter_in"] += 1
            inx, iny = int(fnx), int(fny)
            _stage_counters(rec, stage, inx, iny, J.w, J.h)
            a = nx - fnx
            b = ny - fny
            wts = _weights(a, b, rec, mutation)
            diff = _bilinear(J.window(J.pad, inx, iny), wts, 9) - Iw
            b1 = _sum_f32(diff * Ix, rec, mutation, "b")
            b2 = _sum_f32(diff * Iy, rec, mutation, "b")
            t1 = A12 * b2
            t2 = A22 * b1
            dx = t1 - t2
            dx = dx * D
            t1 = A12 * b1
            t2 = A11 * b2
            dy = t1 - t2
            dy = dy * D
            nx = nx + dx
            ny = ny + dy
            outx = nx + HALF_F
            outy = ny + HALF_F
            step2 = float(dx) * float(dx) + float(dy) * float(dy)
            if abs(step2 - 1e-4) <= 1e-4 * 1e-4:
                rec["band_stop" if step2 <= EPS * EPS else "band_go"] += 1
            if step2 <= EPS * EPS:
                exit_kind = "exit_eps"
                break
            if j > 0:
                sx, sy = abs(float(dx + pdx)), abs(float(dy + pdy))
                for s in (sx, sy):
                    if abs(s - EPS) <= 0.01 * EPS:
                        rec["osc_near_below" if s < EPS else "osc_near_above"] += 1
                if sx < EPS and sy < EPS:
                    if mutation != "no_half_step":
                        hx = dx * F(0.5)
                        hy = dy * F(0.5)
                        outx = outx - hx
                        outy = outy - hy
                    exit_kind = "exit_osc"
                    break
            pdx, pdy = dx, dy
        if exit_kind:
            rec[exit_kind] += 1
        nx, ny = outx, outy
        if status and level == 0 and mutation != "no_final_check":
            fx = nx - HALF_F
            fy = ny - HALF_F
            if _outside(np.floor(fx), np.floor(fy), J.w, J.h):
                rec["final_out"] += 1
                status = 0
            else:
                rec["final_ok"] += 1
    rec["status1_after_coarse_skip"] += bool(status and coarse_skip)
    rec["status1_after_coarse_break"] += bool(status and coarse_break)
    return nx, ny, status


# ------------------------------------------------------------------------------------------------------------------ calls
def lk_track(prev, nxt, xy, mutation=None):
    """calcOpticalFlowPyrLK(prev, next, xy): (out (n, 2) f32, status (n,) u8, counters)."""
    xy = np.ascontiguousarray(xy, F).reshape(-1, 2)
    rec = new_record()
    PA, PB = planes(prev, mutation), planes(nxt, mutation)
    out, st = np.empty((len(xy), 2), F), np.empty(len(xy), np.uint8)
    for i in range(len(xy)):
        out[i, 0], out[i, 1], st[i] = lk_point(PA, PB, xy[i, 0], xy[i, 1], rec, mutation)
    return out, st, rec


def _pairwise(v):
    if len(v) == 0:
        return F(0)
    if len(v) == 1:
        return F(v[0])
    h = len(v) // 2
    return _pairwise(v[:h]) + _pairwise(v[h:])


def track_features(prev, nxt, xy, initial_xy, mutation=None):
    """FeatureTracker::track_features: (kept_xy, kept_index, av_parallax as np.float32, counters).  rec["parallax"] lists the
    f32 parallax of every feature that passed both statuses and the forward-backward test, as (index, value); rec["fwd"] and
    rec["status1"] are the forward pass, i.e. what lk_track returns on the same input."""
    xy = np.ascontiguousarray(xy, F).reshape(-1, 2)
    init = np.ascontiguousarray(initial_xy, F).reshape(-1, 2)
    n = len(xy)
    rec = new_record()
    rec["parallax"] = []
    rec["fwd"], rec["status1"] = np.empty((n, 2), F), np.empty(n, np.uint8)
    PA, PB = planes(prev, mutation), planes(nxt, mutation)
    kept_xy, kept_idx, pars = [], [], []
    for i in range(n):
        fx, fy, s1 = lk_point(PA, PB, xy[i, 0], xy[i, 1], rec, mutation)
        rec["fwd"][i], rec["status1"][i] = (fx, fy), s1
        bx, by, s2 = lk_point(PB, PA, fx, fy, rec, mutation)
        if not s1:
            rec["status1_0"] += 1
        if not s2:
            rec["status2_0"] += 1
        if not (s1 and s2):
            continue
        ex = xy[i, 0] - bx
        ey = xy[i, 1] - by
        d2 = float(ex) * float(ex) + float(ey) * float(ey)
        rec["fb_is_2"] += d2 == FB_MAX * FB_MAX
        if not (d2 <= FB_MAX * FB_MAX if mutation == "fb_le" else d2 < FB_MAX * FB_MAX):
            rec["fb_fail"] += 1
            continue
        rec["fb_ok"] += 1
        dx = fx - init[i, 0]
        dy = fy - init[i, 1]
        p = dx * dx
        q = dy * dy
        p = p + q
        parallax = np.sqrt(p)
        rec["parallax"].append((i, parallax))
        rec["parallax_is_200"] += parallax == MAX_PARALLAX
        if parallax >= MAX_PARALLAX if mutation == "parallax_ge" else parallax > MAX_PARALLAX:
            rec["parallax_drop"] += 1
            continue
        rec["parallax_keep"] += 1
        kept_xy.append((fx, fy))
        kept_idx.append(i)
        pars.append(parallax)
    if mutation == "pairwise_sum":
        total = _pairwise(pars)
    else:
        total = F(0)
        for p in pars:
            total = total + p
    if n == 0:
        av = F(0)
    elif mutation == "mean_over_kept":
        av = total / F(len(pars)) if pars else F(0)
    else:
        av = total / F(n)
    return np.array(kept_xy, F).reshape(-1, 2), np.array(kept_idx, np.int32), F(av), rec
