"""bench.py's launcher contract: `--gpus N` without a launcher starts N ranks itself and must REFUSE (non-zero exit, clear
message) when fewer GPUs are visible — never print a line measured on fewer ranks than asked."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300, env=e)


def test_bench_refuses_more_ranks_than_gpus():
    import torch
    want = torch.cuda.device_count() + 1
    if want < 2:
        want = 2
    r = _run(["--gpus", str(want), "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "refusing" in r.stderr and '"metric"' not in r.stdout


def test_bench_refuses_a_world_size_that_is_not_gpus():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], env={"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE" in r.stderr and '"metric"' not in r.stdout


def test_bench_spawner_counts_gpus_without_hip_and_starts_the_ranks():
    """`bench.py --gpus N` without a launcher: the parent counts GPUs WITHOUT the HIP runtime (here: the stub
    SVO_BENCH_GPU_COUNT, on a box: *_VISIBLE_DEVICES / the KFD topology in sysfs), refuses to fork + exec from a process that
    has libamdhip64 mapped, and starts the ranks with torch.distributed.run.  The two ranks come up, rendezvous over gloo and
    then fail at svo_create: they are forced onto device 64, which no machine has (with device 0 they would run on a GPU box):
    what is checked is that the spawner got that far and relayed the failure, never a line measured on fewer ranks."""
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "ba50k"],
             env={"SVO_BENCH_GPU_COUNT": "2", "SVO_BENCH_BACKEND": "gloo", "SVO_BENCH_FORCE_DEVICE": "64"})
    assert r.returncode != 0
    assert "2-rank run failed" in r.stderr and '"metric"' not in r.stdout
    assert "HIP runtime mapped" not in r.stderr


def test_bench_gpu_count_reads_the_environment_not_the_runtime():
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    old = {k: os.environ.pop(k, None) for k in ("SVO_BENCH_GPU_COUNT", "ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")}
    try:
        os.environ["SVO_BENCH_GPU_COUNT"] = "5"
        assert bench.visible_gpu_count() == 5
        del os.environ["SVO_BENCH_GPU_COUNT"]
        base = bench.visible_gpu_count()      # the KFD topology of this machine (0 in the build container)
        os.environ["HIP_VISIBLE_DEVICES"] = "0,1"
        assert bench.visible_gpu_count() == (min(base, 2) if base else 2)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def test_bench_fails_when_a_group_thread_dies_and_when_groups_ran_different_step_counts():
    """Round 5: a pipeline group's thread that raised used to end silently while the bench went on and divided the frames of ALL groups
    by the elapsed time (figures up to 2.5x too high, retracted in profiles/).  run_threads must re-raise; group_self_parity must refuse
    groups whose recorded step counts differ."""
    sys.path.insert(0, ROOT)
    import importlib
    import pytest
    bench = importlib.import_module("bench")
    done = []
    with pytest.raises(RuntimeError, match="store"):
        bench.run_threads([lambda: done.append(1), lambda: (_ for _ in ()).throw(RuntimeError("landmark store belongs to another id")), lambda: done.append(2)])
    assert sorted(done) == [1, 2]  # the others ran to their end first
    bench.run_threads([lambda: done.append(3)])

    class G:
        def __init__(self, n, raws):
            self.n, self.raws = n, raws
    rec = bytes(range(16))
    ok = bench.group_self_parity([G(2, [rec * 2 * 4] * 3), G(2, [rec * 2 * 4] * 3)], 4)
    assert ok["lanes_checked"] == 4 and ok["steps_checked"] == 3 and ok["lane_steps_that_differ_from_step_0"] == 0
    with pytest.raises(RuntimeError, match="fewer steps"):
        bench.group_self_parity([G(2, [rec * 2 * 4] * 3), G(2, [rec * 2 * 4] * 1)], 4)
