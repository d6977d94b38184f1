"""bench.py --workload ba50k: BASELINE.json configs[3] — synthetic 50k-landmark / 20-keyframe bundle
adjustment, landmarks sharded across the ranks (landmark j on rank j mod N, poses replicated), the reduced
camera system summed over the ranks by RCCL called from the library on the adjuster's own stream
(svo_ba_set_comm).  A step = one LM iteration (strong scaling: the problem is fixed, per-rank
work shrinks with N).  The timed solve follows an untimed warm-up solve of the same problem (code objects
loaded, workspaces sized, communicator warmed)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, CX, CY, W, H = 718.856, 607.1928, 185.2157, 1241, 376
FP64_PUBLIC_PEAK_TFLOPS = 78.6  # AMD's public MI355X figure for the FP64 vector and matrix pipes (not in the local guide)


def make_problem(seed=0xBA000004, K=20, N=50000, dense=False, noise=0.5):
    """Vectorised SURVEY §8d config-4 generator: poses on a gently curving trajectory 1 m apart, landmarks in the
    union of frusta, visibility windows L_j ~ U{2..20}, 0.5 px noise, perturbed initial values, pose 0 fixed."""
    rng = np.random.default_rng(seed)
    yaw = 0.01 * np.arange(K)
    C = np.stack([0.005 * np.arange(K) ** 2, np.zeros(K), 1.0 * np.arange(K)], 1)
    q = np.stack([np.cos(-yaw / 2), np.zeros(K), np.sin(-yaw / 2), np.zeros(K)], 1)

    def rot(qq):
        w, x, y, z = qq.T
        return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                         np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                         np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    R = rot(q)
    t = -np.einsum("kij,kj->ki", R, C)
    poses = np.concatenate([q, t], 1)
    pts = np.stack([rng.uniform(-14, 14, N), rng.uniform(-2.5, 2.0, N), rng.uniform(4, 60 + K, N)], 1)
    Lj = np.full(N, K) if dense else rng.integers(2, K + 1, N)
    sj = np.zeros(N, int) if dense else (rng.random(N) * (K - Lj + 1)).astype(int)
    Xc = np.einsum("kij,nj->nki", R, pts) + t[None]
    u = F * Xc[..., 0] / Xc[..., 2] + CX
    v = F * Xc[..., 1] / Xc[..., 2] + CY
    kk = np.arange(K)[None]
    vis = (Xc[..., 2] > 1.0) & (u >= 0) & (u < W) & (v >= 0) & (v < H) & (kk >= sj[:, None]) & (kk < (sj + Lj)[:, None])
    vis &= vis.sum(1, keepdims=True) >= 2
    keep = vis.any(1)
    pts, vis, u, v = pts[keep], vis[keep], u[keep], v[keep]
    oj, op = np.nonzero(vis)  # landmark-major, pose ascending
    uv = np.stack([u[oj, op], v[oj, op]], 1) + rng.normal(0, noise, (len(oj), 2))
    pts0 = pts + rng.normal(0, 0.10, pts.shape)
    poses0 = poses.copy()
    poses0[1:, 4:] += rng.normal(0, 0.05, (K - 1, 3))
    dq = np.concatenate([np.ones((K - 1, 1)), rng.normal(0, 0.004, (K - 1, 3))], 1)
    w1, x1, y1, z1 = dq.T
    w2, x2, y2, z2 = poses0[1:, :4].T
    poses0[1:, :4] = np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                               w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], 1)
    return dict(poses0=poses0, points0=pts0, op=op.astype(np.int32), oj=oj.astype(np.int32), uv=uv, poses_gt=poses)


def flops_per_iteration(op, oj, n_points):
    """466 per observation + per landmark 50 + 144 L + 216 L(L+1)/2 (f64)."""
    L = np.bincount(oj, minlength=n_points).astype(np.float64)
    return 466.0 * len(op) + float(np.sum(50 + 144 * L + 216 * L * (L + 1) / 2))


def bytes_per_iteration(n_obs, n_points, K):
    """24 B per observation (uv + two indices), 48 B per landmark (read + write), 56 B per pose."""
    return 24.0 * n_obs + 48.0 * n_points + 56.0 * K


def rccl_comm(S, dist, torch, dev, rank, world, local):
    """The rank's ncclComm_t for the library's own all-reduce: the unique id is created on rank 0 by the librccl the
    library binds and broadcast through the process group (whatever its backend is)."""
    from stereo_vo_amd import api
    if dist.get_backend() == "nccl":
        idt = torch.zeros(128, dtype=torch.uint8, device=dev)
        if rank == 0:
            idt.copy_(torch.frombuffer(bytearray(api.rccl_unique_id()), dtype=torch.uint8))
        dist.broadcast(idt, 0)
        uid = bytes(idt.cpu().numpy().tobytes())
    else:
        box = [api.rccl_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, 0)
        uid = box[0]
    return api.rccl_comm_create(world, rank, uid, local)


def cpu_baseline(p, K, seconds=12.0):
    """The CPU oracle (restatement of ceres::Solve DENSE_SCHUR, kind "port") on a bounded sample of the SAME problem:
    the first half of the landmarks, 3-iteration solves repeated for about 12 s, host cores."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    cores = min(os.cpu_count() or 1, 16)
    n_lm = len(p["points0"]) // 2
    m = p["oj"] < n_lm
    op, oj, uv, pts = p["op"][m], p["oj"][m], p["uv"][m], p["points0"][:n_lm]
    t0 = time.perf_counter()
    its = 0
    while time.perf_counter() - t0 < seconds and its < 600:
        _, _, so = O.ba_solve(p["poses0"], pts, op, oj, uv, F, CX, CY, max_iterations=3, num_threads=cores)
        its += max(so["iterations"], 1)
    dt = time.perf_counter() - t0
    frac = len(op) / len(p["op"])
    # iterations/s of the FULL problem: work is linear in the observations, so the sample's rate scales by its share
    cb = dict(value=its / dt * frac, unit="iterations/s", cores=cores, kind="port",
              sample=f"oracle ba_solve on the first {n_lm} landmarks ({len(op)} of {len(p['op'])} observations, {its} LM "
                     f"iterations in {dt:.1f} s), rate scaled by the observation share {frac:.3f}")
    return cb, dict(pts=pts, op=op, oj=oj, uv=uv, oracle=so)


def parity_vs_cpu(S, ctx, p, K, sub, acc_mode):
    """The SAME 3-iteration solve of the cpu_baseline sample on the GPU: in the deterministic accumulation mode (declared summation
    order: the oracle's numbers) and in the mode the bench line was measured in (hardware-order sums: tolerance level)."""
    out = {"sample": f"3 LM iterations on the cpu_baseline sample ({len(sub['pts'])} landmarks, {len(sub['op'])} observations)"}
    so = sub["oracle"]
    for mode in dict.fromkeys(("deterministic", acc_mode)):
        ba = S.BA(ctx, K, F, CX, CY, max_landmarks=len(sub["pts"]) + 8, max_observations=len(sub["op"]) + 8, max_iterations=3, max_time_s=0.0,
                  accumulation=mode)
        try:
            ba.load_problem(p["poses0"], sub["pts"], sub["op"], sub["oj"], sub["uv"])
            s = ba.solve_problem()
        except S.api.SvoError as e:  # the dense variant's contribution slots (210 pose pairs per landmark) exceed the deterministic mode's store
            out[mode] = {"not_run": str(e)[-120:]}
            continue
        finally:
            ba.close()
        out[mode] = {"iterations_identical": bool(s.iterations == so["iterations"]),
                     "initial_cost_rel_diff": abs(s.initial_cost - so["initial_cost"]) / so["initial_cost"],
                     "final_cost_rel_diff": abs(s.final_cost - so["final_cost"]) / so["final_cost"],
                     "final_cost_bits_identical": bool(s.final_cost == so["final_cost"])}
    det, acc = out.get("deterministic", {}), out.get(acc_mode, {})
    if "final_cost_rel_diff" in det:
        out["identical"] = bool(det["iterations_identical"] and det["final_cost_rel_diff"] <= 1e-12)
    else:  # tolerance level only (hardware-order sums): the bound tests/test_ba_config4.py uses for the first iterations
        out["identical"] = None
        out["within_tolerance"] = bool(acc.get("iterations_identical") and acc.get("final_cost_rel_diff", 1.0) <= 1e-9)
    return out


def run(args, cpu_seconds=12.0):
    sys.path.insert(0, ROOT)
    import stereo_vo_amd as S
    from stereo_vo_amd import sharding
    import bench
    torch, dist, rank, local, world = bench.dist_setup(args.gpus)
    dev = torch.device("cuda", local)
    p = make_problem(dense=os.environ.get("SVO_BA_DENSE") == "1")
    # developer aid: SVO_BA_SHARD_OF=N times the per-rank load of an N-rank run on one GPU (no collective)
    emu = int(os.environ.get("SVO_BA_SHARD_OF", "0"))
    pts, op, oj, uv, mine = sharding.shard_problem(p["points0"], p["op"], p["oj"], p["uv"], rank if not emu else 0, world if not emu else emu)
    ctx = S.Context(64, 64, device=local)
    K = p["poses0"].shape[0]
    iters = args.steps
    acc_mode = os.environ.get("SVO_BA_ACC", "mfma")
    ba = S.BA(ctx, K, F, CX, CY, max_landmarks=len(pts) + 8, max_observations=len(op) + 8, max_iterations=iters, max_time_s=0.0,
              accumulation=acc_mode)
    comm = None
    if dist is not None:
        if os.environ.get("SVO_BA_COLLECTIVE", "rccl") == "rccl" and dist.get_backend() == "nccl":
            comm = rccl_comm(S, dist, torch, dev, rank, world, local)
            ba.set_comm(comm)  # ncclAllReduce from the library, on the adjuster's stream: no Python in the LM loop
        else:
            ba.set_allreduce(sharding.allreduce_device_fn(dist, dev))  # rehearsal on one GPU (gloo): callback
    # warm-up solve, then the timed solve of exactly `iters` LM iterations from the same start
    warm = max(1, min(args.warmup, iters))
    wb = S.BA(ctx, K, F, CX, CY, max_landmarks=len(pts) + 8, max_observations=len(op) + 8, max_iterations=warm, max_time_s=0.0,
              accumulation=acc_mode)
    if comm is not None:
        wb.set_comm(comm)
    elif dist is not None:
        wb.set_allreduce(sharding.allreduce_device_fn(dist, dev))
    wb.load_problem(p["poses0"], pts, op, oj, uv)
    ws = wb.solve_problem()
    wb.close()
    ba.load_problem(p["poses0"], pts, op, oj, uv)
    if args.full:
        ctx.profile_select("ba_linearize")
    bench.barrier_sync(torch, dist, ctx)
    t0 = time.perf_counter()
    s = ba.solve_problem()
    bench.barrier_sync(torch, dist, ctx)
    dt = time.perf_counter() - t0
    k_ms, k_n = ctx.profile_read() if args.full else (0.0, 0)
    st = ba.last_stats()
    if args.dump_outputs and rank == 0:
        poses, points = ba.read_problem()  # this rank's landmarks
        bench.dump_outputs(args.dump_outputs, {"poses": poses, "points": points, "final_cost": np.array([s.final_cost])})
    if dist is not None:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    n_it = max(s.iterations, 1)
    fl_local = flops_per_iteration(op, oj, len(pts))
    n = 6 * (K - 1)
    out = {"metric": "BA LM iterations/sec (50k landmarks x 20 keyframes)", "value": n_it / dt, "unit": "iterations/s",
           "n_gpus": (dist.get_world_size() if dist is not None else 1), "steps": n_it, "warmup": ws.iterations, "ms_per_step": 1e3 * dt / n_it, "higher_is_better": True,
           "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "ba_50k_landmarks_20_keyframes (BASELINE configs[3])", "observations": int(len(p["op"])),
                      "landmarks": int(len(p["points0"])), "poses": K, "final_cost": s.final_cost,
                      "initial_cost": s.initial_cost, "accumulation": acc_mode, "variant": "dense (every landmark in all 20 poses)" if os.environ.get("SVO_BA_DENSE") == "1" else "sparse (L_j ~ U{2..20})",
                      "sharding": "landmark j on rank j mod N, poses replicated",
                      "collective": ("ncclAllReduce(sum, f64) from libsvo_hip.so on the adjuster's stream" if comm is not None else
                                     "callback" if dist is not None else "none (single rank)"),
                      "doubles_per_exchange": {"payload2": 8, "payload1": n * n + 3 * n + 2},
                      "lm_stats": {"stand_alone_pass_A": st.linearize_calls, "steps": st.step_calls,
                                   "next_linearisation_with_the_step": st.speculations, "usable": st.speculation_hits,
                                   "payloads_in_one_collective": st.single_exchange},
                      # all-reduces the LM loop issued (or would issue on N ranks): a stand-alone pass A = 1, a same-sweep step = 1
                      # (both payloads in one buffer), a chained step = 2 (payload2, decision, payload1), a plain step = 1
                      "collectives_per_iteration": st.collectives / n_it,
                      # round 5: where the step control ran (1: ba_bulk_control_kernel on the device, the host only enqueues) and what the
                      # host spent inside the LM loop per iteration — launch calls; with the device-side control it is overlapped by the
                      # run-ahead (the GPU never waits for it)
                      "step_control_on_device": bool(st.device_control),
                      "host_us_per_iteration": st.host_us / n_it}}
    if k_n:
        # roofline of the dominant kernel.  achieved = SURVEY 8d algorithmic f64 flops of one linearisation / launch time,
        # HIP events on the adjuster's stream.  peak = the f64 MFMA rate MEASURED on this card (svo_measure_peak).
        avg_us = 1e3 * k_ms / k_n
        tf = fl_local / (avg_us * 1e-6) / 1e12
        peaks = {k: ctx.measure_peak(k) / 1e12 for k in ("f64_mfma", "f64_fma", "f64_muladd")}
        hbm = ctx.measure_peak("hbm_copy") / 1e9
        out["roofline"] = {"kernel": "ba_linearize_mfma_kernel" if acc_mode == "mfma" else "ba_linearize_kernel",
                           "bound": "mfma", "achieved": tf, "peak": peaks["f64_mfma"],
                           "unit": "TFLOP/s", "frac": tf / peaks["f64_mfma"], "traffic": None, "avg_launch_us": avg_us,
                           "launches": k_n, "accumulation": acc_mode,
                           "measured_peaks_tflops": peaks, "public_peak_tflops": FP64_PUBLIC_PEAK_TFLOPS,
                           "measured_hbm_copy_gbs": hbm,
                           "algorithmic_bytes_per_launch": bytes_per_iteration(len(op), len(pts), K),
                           "note": "per-rank algorithmic flops (466/observation + 50 + 144 L + 108 L(L+1) per landmark) over the "
                                   "launch time; peaks measured on this card by svo_measure_peak; the kernel's parity-exact "
                                   "residual/Jacobian part issues separate f64 multiply and add (f64_muladd row), only the "
                                   "Schur products run on the matrix pipe"}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not emu:
        out["cpu_baseline"], sub = cpu_baseline(p, K, cpu_seconds)
        out["parity_vs_cpu"] = parity_vs_cpu(S, ctx, p, K, sub, acc_mode)
    ba.close()
    if comm is not None:
        from stereo_vo_amd import api
        api.rccl_comm_destroy(comm)
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()
    return out if rank == 0 else None
