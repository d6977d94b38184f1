"""numpy float64 restatement of the rectification arithmetic declared in include/svo.h / host/rectify.cpp, written from
that declaration (not shared with product code): the table (build_map) and the integer bilinear warp (remap).

Every numpy operation on float64 arrays rounds once (no fused multiply-add), np.rint rounds ties to even: the same bits as
the declared order of operations."""
import numpy as np

SENTINEL = -32768


class DisplacementOverflow(ValueError):
    pass


def build_map(eye, cam, width, height):
    """eye: dict(fx, fy, cx, cy, k1, k2, p1, p2, R (9 row-major)); cam: dict(focal, cx, cy) -> (H, W, 2) int16."""
    f64 = np.float64
    focal, cx, cy = f64(cam["focal"]), f64(cam["cx"]), f64(cam["cy"])
    fx, fy, cxr, cyr = f64(eye["fx"]), f64(eye["fy"]), f64(eye["cx"]), f64(eye["cy"])
    k1, k2, p1, p2 = f64(eye["k1"]), f64(eye["k2"]), f64(eye["p1"]), f64(eye["p2"])
    R = np.asarray(eye["R"], f64).reshape(-1)
    u = np.arange(width, dtype=f64)[None, :].repeat(height, 0)
    v = np.arange(height, dtype=f64)[:, None].repeat(width, 1)
    with np.errstate(all="ignore"):
        xn = (u - cx) / focal
        yn = (v - cy) / focal
        X = (R[0] * xn + R[3] * yn) + R[6]
        Y = (R[1] * xn + R[4] * yn) + R[7]
        W = (R[2] * xn + R[5] * yn) + R[8]
        x = X / W
        y = Y / W
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        t = (f64(2.0) * x) * y
        kr = (k2 * r2 + k1) * r2 + f64(1.0)
        xd = (x * kr + p1 * t) + p2 * (r2 + f64(2.0) * x2)
        yd = (y * kr + p1 * (r2 + f64(2.0) * y2)) + p2 * t
        sx = fx * xd + cxr
        sy = fy * yd + cyr
        ex = f64(32.0) * sx
        ey = f64(32.0) * sy
        ok = (W > 0) & (np.abs(ex) < 2.0 ** 40) & (np.abs(ey) < 2.0 ** 40)  # comparisons with NaN are False
        qx = np.rint(np.where(ok, ex, 0.0)).astype(np.int64)
        qy = np.rint(np.where(ok, ey, 0.0)).astype(np.int64)
    ix, iy = qx >> 5, qy >> 5
    ok &= (ix >= -1) & (ix <= width - 1) & (iy >= -1) & (iy <= height - 1)  # at least one of the four taps is inside
    dx = qx - 32 * u.astype(np.int64)
    dy = qy - 32 * v.astype(np.int64)
    bad = ok & ((np.abs(dx) > 32767) | (np.abs(dy) > 32767))
    if bad.any():
        raise DisplacementOverflow("a displacement does not fit an int16")
    out = np.full((height, width, 2), SENTINEL, np.int16)
    out[..., 0][ok] = dx[ok]
    out[..., 1][ok] = dy[ok]
    return out


def remap(raw, dxdy):
    """raw (H, W) uint8, dxdy (H, W, 2) int16 -> (H, W) uint8: exact-integer bilinear, outside taps and sentinels give 0."""
    raw = np.asarray(raw, np.uint8)
    H, W = raw.shape
    m = np.asarray(dxdy, np.int16).astype(np.int64)
    sent = (m[..., 0] == SENTINEL) & (m[..., 1] == SENTINEL)
    u = np.arange(W, dtype=np.int64)[None, :]
    v = np.arange(H, dtype=np.int64)[:, None]
    qx = 32 * u + m[..., 0]
    qy = 32 * v + m[..., 1]
    ix, iy, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31

    def tap(xx, yy):
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        p = raw[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
        return np.where(inside, p, 0)

    acc = ((32 - ax) * (32 - ay) * tap(ix, iy) + ax * (32 - ay) * tap(ix + 1, iy)
           + (32 - ax) * ay * tap(ix, iy + 1) + ax * ay * tap(ix + 1, iy + 1) + 512) >> 10
    return np.where(sent, 0, acc).astype(np.uint8)


def eye_dict(e):
    """api.RectifyEye -> the dict build_map takes."""
    return dict(fx=e.fx, fy=e.fy, cx=e.cx, cy=e.cy, k1=e.k1, k2=e.k2, p1=e.p1, p2=e.p2, R=list(e.R))


def cam_dict(c):
    return dict(focal=c.focal, cx=c.cx, cy=c.cy)


def rot(rx_deg, ry_deg, rz_deg):
    """Rz Ry Rx, row-major 3x3 (test inputs only)."""
    a, b, c = np.deg2rad([rx_deg, ry_deg, rz_deg])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx
