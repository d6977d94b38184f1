"""Pipelined turns of the device-resident solves (ba_lm_multi_kernel for k = 1..4 chunks per wavefront, ba_lm_compact_kernel):
a turn's record, landmark and Jacobi scales are requested while the previous turn computes.  Only loads move, so every form must
still return the host-driven loop's bits — here on the cases where an early load could read the wrong thing: steps the decision
rejects (pass A then reads the current landmarks, not the candidates pass B just wrote), the first pass A (which writes the scales
instead of reading them), a wavefront whose last turn is empty (C not a multiple of 2k) and compact windows of more than 128
chunks (groups of G > 1 chunks in the running sums).  The knob is read once per process: one child process per setting."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (seed, poses, landmarks, noisy): windows of 2..12 poses and 1..~150 chunks; the noisy ones start far from the optimum, so
# the LM loop rejects steps
_PROBLEMS = [(81, 2, 30, False), (82, 3, 70, False), (83, 4, 150, True), (84, 5, 260, False), (85, 6, 380, True), (86, 7, 520, False),
             (87, 8, 800, True), (88, 9, 1100, False), (89, 10, 1400, True), (90, 5, 2100, True), (91, 12, 600, True), (92, 3, 1700, False)]
_BEYOND_128 = [(93, 8, 2600, True), (94, 11, 2300, False)]

_SOLVES = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import stereo_vo_amd as S
import ba_problem as BP
ctx = S.Context(64, 64)
rejected = 0
big = 0
for seed, K, N, noisy in %(problems)r:
    p = BP.make_problem(seed, K, N, noise=2.0, pose_sigma=(0.2, 0.03)) if noisy else BP.make_problem(seed, K, N)
    big += len(p["op"]) > 128 * 64
    res = []
    for dev in (False, True):
        ba = S.api.BA(ctx, max(K, 2), BP.F, BP.CX, BP.CY, max_landmarks=len(p["points0"]) + 8, max_observations=len(p["op"]) + 8, max_time_s=0.0,
                      device_lm=dev, solve_form=%(form)r if dev else None, accumulation="deterministic")
        for rep in range(2):  # the second solve of an adjuster: its first pass A writes the scales again
            ba.load_problem(p["poses0"], p["points0"], p["op"], p["oj"], p["uv"])
            s = ba.solve_problem()
        poses, pts = ba.read_problem()
        res.append((s.iterations, s.successful_steps, s.termination, s.initial_cost, s.final_cost, poses.tobytes(), pts.tobytes()))
        ba.close()
    assert res[0] == res[1], (seed, K, N, len(p["op"]), res[0][:5], res[1][:5])
    rejected += res[0][0] - res[0][1]
print("solves ok rejected", rejected, "beyond128", big)
'''


def _run(env, form, problems):
    code = _SOLVES % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), problems=problems, form=form)
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=900)


def _counts(stdout):
    words = stdout.split("solves ok rejected", 1)[1].split()
    return int(words[0]), int(words[2])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_hip_pipelined_wide_solve_with_k_chunks_per_wavefront_equals_the_host_driven_loop(k):
    """The wide form, bit for bit against the host-driven loop, with rejected steps among the iterations."""
    out = _run({"SVO_BA_WAVE_CHUNKS": str(k)}, "wide", _PROBLEMS)
    assert out.returncode == 0 and "solves ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
    rejected, _ = _counts(out.stdout)
    assert rejected > 0, out.stdout[-500:]


@pytest.mark.gpu
def test_hip_pipelined_compact_solve_equals_the_host_driven_loop():
    """The compact form, bit for bit against the host-driven loop, up to and beyond 128 chunks."""
    out = _run({}, "compact", _PROBLEMS + _BEYOND_128)
    assert out.returncode == 0 and "solves ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
    rejected, big = _counts(out.stdout)
    assert rejected > 0 and big == len(_BEYOND_128), out.stdout[-500:]
