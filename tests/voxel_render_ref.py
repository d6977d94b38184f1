"""The voxel map's render (include/svo.h, "Voxel map render") restated twice, by two routes that share no code, on the
Tables of tests/voxel_ref.py:

  render_np   whole arrays in numpy, one f64 operation per ufunc (numpy never contracts); the footprints as expanded index lists,
              one per radius that occurs, masked to the image and written by np.maximum.at;
  render_py   voxel by voxel in Python floats and integers; the footprint as a clipped range of rows and columns.

Both return (disp16 (height, width) int16, intensity (height, width) uint8, (n_qualifying, n_drawn, n_splat, n_pixels)).
`variant` of render_np states one deliberate misreading of the contract each; tests/test_voxel_render.py shows that every one of
them changes a render of the main scene.  The scenes are those of tests/voxel_carve_ref.py.  Nothing here is tuned on the library's
output.
"""
import math

import numpy as np

FILTERED = -16
VARIANTS = ("min", "r_floor", "d_trunc", "centre_inside", "no_intensity", "count_gt")


def _resolve(pix, height, width):
    pix = pix.reshape(height, width)
    disp = np.where(pix == 0, FILTERED, pix >> 8).astype(np.int16)
    return disp, (pix & 255).astype(np.uint8), int((pix != 0).sum())


# ------------------------------------------------------------------------------------------------ route (a): numpy
def render_np(table, width, height, cam, m12, voxel_size, min_count=1, max_radius=8, variant=None):
    """cam = (focal, cx, cy, baseline); m12: world->camera, 12 doubles."""
    focal, cx, cy, baseline = (np.float64(v) for v in cam)
    m = np.asarray(m12, np.float64).reshape(3, 4)
    vs = np.float64(np.float32(voxel_size))
    W, H = int(width), int(height)
    count = table.ci >> np.uint64(40)
    mc = np.uint64(min_count)
    qual = (count > mc) if variant == "count_gt" else (count >= mc)
    with np.errstate(all="ignore"):
        c = count.astype(np.float64) * 65536.0
        p = []
        for r, s in enumerate((table.sx, table.sy, table.sz)):
            k = (((table.keys >> np.uint64(21 * r)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20)).astype(np.float64)
            pr = s.astype(np.float64) / c
            pr = k + pr
            p.append(pr * vs)
        q = []
        for r in range(3):
            w = m[r, 0] * p[0]
            w = w + m[r, 1] * p[1]
            w = w + m[r, 2] * p[2]
            q.append(w + m[r, 3])
        front = q[2] > 0.0
        centre = []
        for cr, c0 in ((q[0], cx), (q[1], cy)):
            u = focal * cr
            u = u / q[2]
            u = u + c0
            centre.append(np.floor(u + 0.5))
        dv16 = focal * baseline
        dv16 = dv16 / q[2]
        dv16 = dv16 * 16.0
        d16 = np.floor(dv16) if variant == "d_trunc" else np.floor(dv16 + 0.5)
        seen = (d16 >= 1.0) & (d16 <= 32767.0)
        h = focal * vs
        h = h / q[2]
        h = h * 0.5
        rad = np.floor(h) if variant == "r_floor" else np.floor(h + 0.5)
        rad = np.minimum(np.float64(max_radius), rad)
        edge = np.zeros_like(rad) if variant == "centre_inside" else rad
        inside = (centre[0] >= -edge) & (centre[0] <= (W - 1) + edge) & (centre[1] >= -edge) & (centre[1] <= (H - 1) + edge)
    drawn = qual & front & seen & inside
    idx = np.flatnonzero(drawn)
    px, py = centre[0][idx].astype(np.int64), centre[1][idx].astype(np.int64)
    rr = rad[idx].astype(np.int64)
    isum = table.ci[idx] & np.uint64((1 << 40) - 1)
    mean = (isum // count[idx]).astype(np.int64)
    d = d16[idx].astype(np.int64)
    if variant == "no_intensity":  # the depth alone is compared; among equal depths the voxel first in the table stays
        value = (d << 40) | ((len(table.keys) - 1 - idx.astype(np.int64)) << 8) | mean
    else:
        value = (d << 8) | mean
    if variant == "min":  # the smallest value of a pixel's voxels, i.e. the largest of the complements
        value = (1 << 62) - value
    pix = np.zeros(W * H, np.int64)
    n_splat = 0
    for r in np.unique(rr).tolist():
        sel = rr == r
        oy, ox = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
        x = px[sel][:, None] + ox.reshape(1, -1)
        y = py[sel][:, None] + oy.reshape(1, -1)
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        v = np.broadcast_to(value[sel][:, None], x.shape)
        np.maximum.at(pix, (y[ok] * W + x[ok]), v[ok])
        n_splat += int(ok.sum())
    if variant == "min":
        pix = np.where(pix == 0, 0, (1 << 62) - pix)
    if variant == "no_intensity":
        pix = ((pix >> 40) << 8) | (pix & 255)
    disp, inten, n_pixels = _resolve(pix, H, W)
    return disp, inten, (int(qual.sum()), int(drawn.sum()), n_splat, n_pixels)


# ------------------------------------------------------------------------------------------------ route (b): Python
def render_py(table, width, height, cam, m12, voxel_size, min_count=1, max_radius=8):
    """Leaves the drawn voxels in table order as (px, py, r, d16, mean intensity) under render_py.last."""
    focal, cx, cy, baseline = (float(v) for v in cam)
    m = [float(v) for v in np.asarray(m12, np.float64).reshape(12)]
    vs = float(np.float32(voxel_size))
    W, H = int(width), int(height)
    rows = [[0] * W for _ in range(H)]
    n_qual = n_drawn = n_splat = 0
    render_py.last = []
    for key, ci, sx, sy, sz in zip(*(a.tolist() for a in (table.keys, table.ci, table.sx, table.sy, table.sz))):
        count = ci >> 40
        if count < min_count:
            continue
        n_qual += 1
        pw = []
        for r, s in enumerate((sx, sy, sz)):
            k = ((key >> (21 * r)) & 0x1FFFFF) - (1 << 20)
            pw.append((float(k) + float(s) / (float(count) * 65536.0)) * vs)
        c = []
        for r in range(3):
            w = m[4 * r] * pw[0]
            w = w + m[4 * r + 1] * pw[1]
            w = w + m[4 * r + 2] * pw[2]
            c.append(w + m[4 * r + 3])
        if not c[2] > 0.0:
            continue
        u = focal * c[0] / c[2] + cx + 0.5
        v = focal * c[1] / c[2] + cy + 0.5
        dv = focal * baseline / c[2] * 16.0 + 0.5
        hh = focal * vs / c[2] * 0.5 + 0.5
        if not (math.isfinite(u) and math.isfinite(v) and math.isfinite(dv)):  # floor keeps them, and a comparison below fails
            continue
        d16 = math.floor(dv)
        if not 1 <= d16 <= 32767:
            continue
        r = min(max_radius, math.floor(hh)) if math.isfinite(hh) else max_radius
        px, py = math.floor(u), math.floor(v)
        if not (-r <= px <= W - 1 + r and -r <= py <= H - 1 + r):
            continue
        n_drawn += 1
        value = d16 << 8 | (ci & ((1 << 40) - 1)) // count
        render_py.last.append((px, py, r, d16, value & 255))
        x0, x1, y0, y1 = max(px - r, 0), min(px + r, W - 1), max(py - r, 0), min(py + r, H - 1)
        n_splat += (x1 - x0 + 1) * (y1 - y0 + 1)
        for y in range(y0, y1 + 1):
            row = rows[y]
            for x in range(x0, x1 + 1):
                if value > row[x]:
                    row[x] = value
    disp, inten, n_pixels = _resolve(np.array(rows, np.int64), H, W)
    return disp, inten, (n_qual, n_drawn, n_splat, n_pixels)
