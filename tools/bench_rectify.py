#!/usr/bin/env python3
"""What rectification costs on the MI355X (a tool: bench.py is untouched and measures no rectification).

One process, two measurements:
  1. the remap launch alone at the bench shape (1241 x 376, 16 frames x 96 lanes x 2 eyes = 3072 images, one shared camera),
     timed with HIP events around the launch (svo_profile_select("rectify_remap")), as bytes/s over the pass's algorithmic
     bytes (1 B read + 4 B table + 1 B written per pixel), beside svo_measure_peak("hbm_copy") taken in the same run;
  2. bench.py's headline load (96 lanes in 3 pipeline groups of 16-frame steps, its group settings) without and with
     rectification on the same frames, alternating, as frames/s and their ratio.
Prints one JSON line; --out also writes the text report.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (its module level sets the hardware-queue count bench.py measures with, before HIP starts)
import numpy as np  # noqa: E402

W, H = bench.W, bench.H
BYTES_PER_PIXEL = 6  # 1 read + 4 table + 1 written


def model(S, p):
    """A mild stereo camera: barrel distortion, tangential terms, a fraction of a degree about each axis, per eye."""
    from stereo_vo_amd import api

    def rot(rx, ry, rz):  # Rz Ry Rx, degrees
        a, b, c = np.deg2rad([rx, ry, rz])
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
        return Rz @ Ry @ Rx
    return (api.rectify_eye(p.focal * 1.004, p.focal * 0.997, p.cx + 1.3, p.cy - 0.8, -0.03, 0.008, 2e-4, -1e-4, rot(0.15, -0.2, 0.1)),
            api.rectify_eye(p.focal * 0.998, p.focal * 1.003, p.cx - 0.9, p.cy + 0.6, -0.025, 0.006, -1e-4, 2e-4, rot(-0.1, 0.15, -0.12)))


def standalone(S, torch, lanes, frames, warmup, reps):
    images = lanes * frames * 2
    ctx = S.Context(W, H, max_batch=1, max_corners=64, max_candidates=1 << 12, max_features=64)
    p = S.synth_default(W, H)
    cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
    eye = model(S, p)[0]
    left = S.synth_render(p, 0)[0]
    src = torch.from_numpy(left).cuda().repeat(images, 1, 1).contiguous()  # 3072 frames in HBM: far beyond the Infinity Cache
    dst = torch.empty_like(src)
    torch.cuda.synchronize()
    copy = ctx.measure_peak("hbm_copy")
    for _ in range(warmup):
        ctx.rectify_remap_batch_dev(src.data_ptr(), images, W, H, W, W * H, eye, cam, dst.data_ptr())
    ctx.profile_select("rectify_remap")
    for _ in range(reps):
        ctx.rectify_remap_batch_dev(src.data_ptr(), images, W, H, W, W * H, eye, cam, dst.data_ptr())
    ms, n = ctx.profile_read()
    ctx.profile_select("")
    assert n == reps, (n, reps)
    per = ms / n * 1e-3
    nbytes = images * W * H * BYTES_PER_PIXEL
    ctx.close()
    return {"images": images, "launch_ms": 1e3 * per, "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / per,
            "hbm_copy_bytes_per_s": copy, "share_of_copy_rate": nbytes / per / copy, "launches_timed": n}


def grouped(S, torch, lanes, n_groups, frames, warmup, steps, rounds):
    bench.group_lines(n_groups)
    seeds = [0x5EED0001 + i for i in range(lanes)]
    groups = [bench._Group(S, torch, 0, seeds[gi::n_groups], frames) for gi in range(n_groups)]
    torch.cuda.synchronize()
    m = model(S, groups[0].p)

    def run(k):
        def work(g):
            for _ in range(k):
                g.step()
        bench.run_threads([lambda g=g: work(g) for g in groups])

    def timed(rect):
        for g in groups:
            g.pipe.set_rectification(-1, *(m if rect else (None, None)))
            g.clear_counters()
        run(warmup)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return lanes * frames * steps / dt, 1e3 * dt / steps

    plain, rect = [], []
    for _ in range(rounds):  # alternating: other people's work shares the host
        plain.append(timed(False))
        rect.append(timed(True))
    for g in groups:
        g.close()
    med = lambda xs: float(np.median(xs))
    fp, fr = med([x[0] for x in plain]), med([x[0] for x in rect])
    return {"lanes": lanes, "groups": n_groups, "frames_per_step_per_lane": frames, "steps": steps, "rounds": rounds,
            "frames_per_s_plain": fp, "frames_per_s_rectified": fr, "ratio": fr / fp,
            "step_ms_plain": med([x[1] for x in plain]), "step_ms_rectified": med([x[1] for x in rect]),
            "all_plain": [x[0] for x in plain], "all_rectified": [x[0] for x in rect]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=96)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-groups", action="store_true")
    ap.add_argument("--out", help="write the text report here as well")
    a = ap.parse_args()
    import torch
    import stereo_vo_amd as S
    if not torch.cuda.is_available():
        sys.exit("bench_rectify: needs the GPU (nothing is measured without it)")
    res = {"standalone": standalone(S, torch, a.lanes, a.frames, 3, 20)}
    if not a.skip_groups:
        res["pipeline_groups"] = grouped(S, torch, a.lanes, a.groups, a.frames, a.warmup, a.steps, a.rounds)
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    print(json.dumps(res))
    if a.out:
        s, g = res["standalone"], res.get("pipeline_groups")
        with open(a.out, "w") as f:
            f.write(f"rectify_remap_kernel, {s['images']} images of {W} x {H} in one launch: {s['launch_ms']:.3f} ms "
                    f"(mean of {s['launches_timed']} launches, HIP events)\n")
            f.write(f"  algorithmic bytes (6 B / pixel): {s['algorithmic_bytes'] / 1e9:.2f} GB -> {s['bytes_per_s'] / 1e12:.3f} TB/s; "
                    f"svo_measure_peak(hbm_copy) in the same run: {s['hbm_copy_bytes_per_s'] / 1e12:.3f} TB/s ({100 * s['share_of_copy_rate']:.1f} %)\n")
            if g:
                f.write(f"{g['lanes']} lanes in {g['groups']} groups, {g['frames_per_step_per_lane']}-frame steps, median of {g['rounds']} alternating rounds of "
                        f"{g['steps']} steps:\n  without rectification {g['frames_per_s_plain']:.0f} frames/s ({g['step_ms_plain']:.1f} ms / step), "
                        f"with {g['frames_per_s_rectified']:.0f} frames/s ({g['step_ms_rectified']:.1f} ms / step): ratio {g['ratio']:.3f}\n"
                        f"  rounds without: {[round(x) for x in g['all_plain']]}, with: {[round(x) for x in g['all_rectified']]}\n")


if __name__ == "__main__":
    main()
