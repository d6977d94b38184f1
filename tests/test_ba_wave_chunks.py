"""The wide device-resident solve with several chunks per wavefront (ba_lm_multi_kernel, SVO_BA_WAVE_CHUNKS=k): every chunk still
publishes its own partials and level 2 sums them in the declared order, so the bits are those of the host-driven loop for every k.
The knob is read once per process: one child process per setting."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, poses, landmarks): windows of 2..14 poses, from one chunk to ~120 (C < 2k and C mod 2k != 0 among them)
_PROBLEMS = [(61, 2, 12), (62, 2, 40), (63, 3, 50), (64, 4, 90), (65, 5, 120), (66, 6, 200), (67, 7, 400), (68, 8, 700),
             (69, 9, 1000), (70, 10, 1300), (75, 5, 2300), (76, 3, 1800), (77, 11, 700), (78, 12, 600), (79, 13, 500), (80, 14, 450)]

_SOLVES = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import stereo_vo_amd as S
import ba_problem as BP
ctx = S.Context(64, 64)
fb = 0
for seed, K, N in %(problems)r:
    p = BP.make_problem(seed, K, N)
    res = []
    for dev in (False, True):
        ba = S.api.BA(ctx, max(K, 2), BP.F, BP.CX, BP.CY, max_landmarks=len(p["points0"]) + 8, max_observations=len(p["op"]) + 8, max_time_s=0.0,
                      device_lm=dev, solve_form="wide" if dev else None, accumulation="deterministic")
        for rep in range(%(reps)d):
            ba.load_problem(p["poses0"], p["points0"], p["op"], p["oj"], p["uv"])
            s = ba.solve_problem()
            if dev:
                fb += ba.last_stats().fallbacks
        poses, pts = ba.read_problem()
        res.append((s.iterations, s.termination, s.initial_cost, s.final_cost, poses.tobytes(), pts.tobytes()))
        ba.close()
    assert res[0] == res[1], (seed, K, N, len(p["op"]), res[0][:4], res[1][:4])
print("solves ok", fb)
'''


def _run(env, reps, problems=_PROBLEMS, timeout=600):
    code = _SOLVES % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), problems=problems, reps=reps)
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_hip_wide_solve_with_k_chunks_per_wavefront_equals_the_host_driven_loop(k):
    """Bit for bit against the host-driven loop for windows of 2..14 poses and 1..~120 chunks, for k = 1..4 chunks per wavefront."""
    out = _run({"SVO_BA_WAVE_CHUNKS": str(k)}, reps=1)
    assert out.returncode == 0 and "solves ok 0" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


@pytest.mark.gpu
def test_hip_wide_solve_with_contiguous_chunk_turns_equals_the_host_driven_loop():
    """The other chunk -> wavefront assignment (SVO_BA_WAVE_ORDER=contiguous) changes no bit either."""
    out = _run({"SVO_BA_WAVE_CHUNKS": "3", "SVO_BA_WAVE_ORDER": "contiguous"}, reps=1, problems=_PROBLEMS[::2])
    assert out.returncode == 0 and "solves ok 0" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


@pytest.mark.gpu
def test_hip_wide_solve_with_two_chunks_per_wavefront_that_gives_up_loses_nothing():
    """SVO_BA_TEST_GIVEUP=2: every second wide launch reports "gave up"; the re-run must return the host-driven loop's bits."""
    problems = [(51, 5, 500), (52, 6, 900), (53, 3, 100), (54, 5, 1200)]
    out = _run({"SVO_BA_WAVE_CHUNKS": "2", "SVO_BA_TEST_GIVEUP": "2"}, reps=2, problems=problems)
    assert out.returncode == 0 and "solves ok 4" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("k", ["1", None])
def test_hip_group_of_eight_lanes_equals_its_oracles_at_k_and_at_one(k):
    """A pipeline group of 8 lanes, frame for frame against the oracle, at one chunk per wavefront and at the default."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_group import _child_code
    e = dict(os.environ)
    e.pop("SVO_BA_WAVE_CHUNKS", None)
    if k is not None:
        e["SVO_BA_WAVE_CHUNKS"] = k
    out = subprocess.run([sys.executable, "-c", _child_code(n=16, lanes=8, batch=8, seed=0x5EED0E00, reps=1)], env=e, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "child ok" in out.stdout, out.stderr[-3000:]
