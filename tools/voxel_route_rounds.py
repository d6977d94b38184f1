"""The CPU trial behind the voxel map route's max_rounds default and its two candidate tile shapes: how many rounds the
tiled relaxation of csrc/voxel_route.hip needs, counted on the host in numpy.  A round relaxes every tile to local convergence (at most
the kernel's 64 sweeps) against a halo frozen at the start of the round - the synchronous reading of a launch, in which no tile sees
what another lowers in the same round; the device can only need fewer.  Reported per case and tile shape: the rounds that changed a
cell (rounds_run's counterpart; a call needs one more to find nothing to do) and the largest number of sweeps a round took.

Cases, at the default volume's proportions scaled down (512 x 128 x 512 -> 128 x 32 x 128): seeded random volumes at densities 0.05,
0.25 and 0.35 with the goal at the centre, an open volume from a corner, and serpentines of slabs across axis 2 every 8 and every 4
layers with one hole row at alternating ends of axis 0 (on 64 x 16 x 64, to keep the trial short).  No GPU, no library: run it with

    python tools/voxel_route_rounds.py [--jobs N]
"""
import argparse
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import voxel_route_ref as V  # noqa: E402  (the moves and the shifted views; not the tiled form)

TILES = ((8, 8, 8), (16, 8, 4))
MAX_SWEEPS = 64
INF = np.int32(0x7FFFFFFF)


def rounds(closed, goal, tile):
    d2, d1, d0 = closed.shape
    free = ~closed
    j2, j1, j0 = np.meshgrid(np.arange(d2), np.arange(d1), np.arange(d0), indexing="ij")
    tid = (j0 // tile[0] + 4096 * (j1 // tile[1] + 4096 * (j2 // tile[2]))).astype(np.int64)
    moves = []
    for k, mv in enumerate(V.MOVES):
        if k == V.SELF:
            continue
        a = free & V._shift(free, mv, False)
        for m in [(x, y, z) for x in {0, mv[0]} for y in {0, mv[1]} for z in {0, mv[2]} if (x, y, z) not in ((0, 0, 0), mv)]:
            a = a & V._shift(free, m, False)
        moves.append((mv, a, V._shift(tid, mv, -1) == tid, np.int32(16 * (3 + 2 * sum(1 for v in mv if v)))))
    cost = np.full(closed.shape, INF, np.int32)
    cost[goal[2], goal[1], goal[0]] = 0
    n_rounds = most = 0
    while True:
        frozen = cost
        sweeps = 0
        while sweeps < MAX_SWEEPS:
            new = cost
            for mv, allowed, same, step in moves:
                cu = np.where(same, V._shift(cost, mv, INF), V._shift(frozen, mv, INF))
                new = np.minimum(new, np.where(allowed & (cu < INF), cu + step, INF))
            if np.array_equal(new, cost):
                break
            cost = new
            sweeps += 1
        if sweeps == 0:
            return n_rounds, most, int((cost < INF).sum())
        n_rounds += 1
        most = max(most, sweeps)


def serpentine(dims, every):
    c = np.zeros((dims[2], dims[1], dims[0]), bool)
    for i, j2 in enumerate(range(every - 1, dims[2] - 1, every)):
        c[j2, :, :] = True
        c[j2, :, dims[0] - 1 if i % 2 == 0 else 0] = False
    return c


def cases():
    big, small = (128, 32, 128), (64, 16, 64)
    out = []
    for density in (0.05, 0.25, 0.35):
        rng = np.random.default_rng([31, int(100 * density)])
        c = rng.random((big[2], big[1], big[0])) < density
        g = (big[0] // 2, big[1] // 2, big[2] // 2)
        c[g[2], g[1], g[0]] = False
        out.append(("random %.2f, goal at the centre, %d x %d x %d" % ((density,) + big), c, g))
    out.append(("open, goal in a corner, %d x %d x %d" % big, np.zeros((big[2], big[1], big[0]), bool), (0, 0, 0)))
    for every in (8, 4):
        out.append(("serpentine, a slab every %d layers, %d x %d x %d" % ((every,) + small), serpentine(small, every), (0, 0, 0)))
    return out


def _one(job):
    name, closed, goal, tile = job
    return name, tile, rounds(closed, goal, tile)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=4)
    a = ap.parse_args()
    jobs = [(name, c, g, t) for name, c, g in cases() for t in TILES]
    with multiprocessing.Pool(a.jobs) as pool:
        for name, tile, (n, most, reached) in pool.imap(_one, jobs):
            print("%-60s tile %2d x %d x %d: %4d rounds, at most %2d sweeps in one, %d cells reached" % ((name,) + tile + (n, most, reached)), flush=True)


if __name__ == "__main__":
    main()
