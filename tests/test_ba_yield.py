"""A wide window solve (ba_lm_multi_kernel) that steps aside after N LM iterations of one launch and continues in a later one
(svo_ba_set_yield_iterations, SVO_BA_YIELD_ITERS): the step-control scalars, the Jacobi scales of the pose columns and the current poses
travel in a small device record, the linearisation is formed again at the current point with the current radius — the totals the
yielding launch held — so every yield keeps every bit.  CPU part: the order in which a pipeline group offers its solves to the
admission (host/group_lines.h), with solves that stepped aside."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_solves_that_stepped_aside_are_offered_before_fresh_ones(tmp_path):
    """host/group_lines.h — the text host/group.cpp compiles — walked on the host under ASan + UBSan: a lane whose keyframe waits comes
    first, a solve that has run before comes before a fresh one, first come, first served within each class; without solves that
    stepped aside the order is the plain one."""
    exe = str(tmp_path / "solve_order_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "stereo_vo_amd", "host"), os.path.join(ROOT, "tests", "sanitize", "solve_order_test.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "solve order ok" in r.stdout


# (seed, poses, landmarks) -> chunks, LM iterations, rejected steps of the CPU oracle: 4 / 45 / 5, 7 / 29 / 1, 26 / 24 / 2, 74 / 48 / 11,
# 66 / 50 (the iteration cap) / 6
_PROBLEMS = [(64, 4, 90), (65, 5, 120), (51, 5, 500), (41, 5, 1500), (76, 3, 1800)]
_ITERATIONS = [45, 29, 24, 48, 50]
_BUDGETS = [1, 2, 3, 7, 10, 25, 64]  # 64 never yields; 10 and 25 put a yield point on the cap's iteration of the last problem

_HEAD = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import stereo_vo_amd as S
import ba_problem as BP
ctx = S.Context(64, 64)
LIMIT = S.lib().svo_ba_wave_chunks_limit()
def make(p, K, dev, k=0, budget=None):
    ba = S.api.BA(ctx, max(K, 2), BP.F, BP.CX, BP.CY, max_landmarks=len(p["points0"]) + 8, max_observations=len(p["op"]) + 8, max_time_s=0.0,
                  device_lm=dev, solve_form="wide" if dev else None, accumulation="deterministic")
    if k:
        ba.set_wave_chunks(k)
    if budget is not None:
        ba.set_yield_iterations(budget)
    ba.load_problem(p["poses0"], p["points0"], p["op"], p["oj"], p["uv"])
    return ba
def bits(ba, s):
    poses, pts = ba.read_problem()
    return (s.iterations, s.termination, s.initial_cost, s.final_cost, poses.tobytes(), pts.tobytes())
def calls(ba, s):
    st = ba.last_stats()
    return (st.linearize_calls, st.step_calls, s.successful_steps)
# A solve of I LM iterations passes the top of the LM loop with m = 0 .. I - 1 iterations behind it (and once more with m = I only where
# a cap ends it there: the caps are tested in front of the yield).  A launch that began at m0 steps aside at the first m with
# m - m0 >= N, so the yields fall on m = N, 2 N, ... <= I - 1: floor((I - 1) / N) of them = ceil(I / N) - 1 — a solve that ends on a
# boundary (I a multiple of N, the cap's iteration included) has finished before it would yield again.
def resumes_expected(I, N):
    return 0 if N <= 0 or I <= 0 else (I - 1) // N
'''

_EVERY_BUDGET = _HEAD + r'''
problems, expect_iters, budgets = %(problems)r, %(iterations)r, %(budgets)r
total = 0
for (seed, K, N), I in zip(problems, expect_iters):
    p = BP.make_problem(seed, K, N)
    ba = make(p, K, False)
    ref = bits(ba, ba.solve_problem())
    ba.close()
    assert ref[0] == I, (seed, K, N, ref[0], I)
    for k in (2, 3, LIMIT):
        ba = make(p, K, True, k, 0)
        s0 = ba.solve_problem()
        assert bits(ba, s0) == ref and ba.solve_resumes() == 0, (seed, K, N, k)
        calls0 = calls(ba, s0)
        ba.close()
        for budget in budgets:
            ba = make(p, K, True, k, budget)
            s = ba.solve_problem()
            got, c, r = bits(ba, s), calls(ba, s), ba.solve_resumes()
            forms, gave_up = ba.solve_forms()
            fb = ba.last_stats().fallbacks
            ba.close()
            print(seed, K, N, "k", k, "budget", budget, "iterations", got[0], "resumes", r, "calls", c, flush=True)
            assert fb == 0 and gave_up == 0 and forms[0] == 0 and forms[k] == 1 and sum(forms) == 1, (seed, K, N, k, budget, forms, gave_up, fb)
            assert got == ref, (seed, K, N, k, budget, got[:4], ref[:4])
            assert c == calls0, (seed, K, N, k, budget, c, calls0)
            assert r == resumes_expected(I, budget) and r == -(-I // budget) - 1, (seed, K, N, k, budget, r, I)
            total += r
print("resumes", total, flush=True)
assert total > 0
print("every budget ok", flush=True)
'''

_NEVER = _HEAD + r'''
for seed, K, N in %(problems)r:
    p = BP.make_problem(seed, K, N)
    ba = make(p, K, False)
    ref = bits(ba, ba.solve_problem())
    ba.close()
    for budget in (1, 3):
        ba = make(p, K, True, 0, budget)
        s = ba.solve_problem()
        forms, gave_up = ba.solve_forms()
        print(seed, K, N, "budget", budget, "iterations", s.iterations, "forms", forms, "resumes", ba.solve_resumes(), flush=True)
        assert s.iterations > budget, (seed, s.iterations)
        assert forms[1] == 1 and sum(forms) == 1 and gave_up == 0 and ba.solve_resumes() == 0, (seed, K, N, forms, gave_up)
        assert bits(ba, s) == ref, (seed, K, N, budget)
        ba.close()
print("never ok", flush=True)
'''

_SHARED = _HEAD + r'''
problems, budgets = %(problems)r, %(budgets)r
ps = [BP.make_problem(seed, K, N) for seed, K, N in problems]
alone = []
for p, (seed, K, N) in zip(ps, problems):
    ba = make(p, K, False)
    alone.append(bits(ba, ba.solve_problem()))
    ba.close()
bas = [make(p, K, True, 0, b) for p, (seed, K, N), b in zip(ps, problems, budgets)]
shared, sums = S.api.BA.solve_problems(bas)
print("shared", shared, flush=True)
assert shared == len(bas), shared
for i, (ba, s) in enumerate(zip(bas, sums)):
    forms, gave_up = ba.solve_forms()
    r = ba.solve_resumes()
    print(problems[i], "budget", budgets[i], "iterations", s.iterations, "resumes", r, flush=True)
    assert gave_up == 0 and forms[0] == 0 and sum(forms) == 1, (i, forms, gave_up)
    assert r == resumes_expected(s.iterations, budgets[i]), (i, r, s.iterations, budgets[i])
    assert bits(ba, s) == alone[i], (i, problems[i], budgets[i])
    ba.close()
print("shared ok", flush=True)
'''

_GIVEUP = _HEAD + r'''
seed, K, N = %(problem)r
p = BP.make_problem(seed, K, N)
ba = make(p, K, False)
ref = bits(ba, ba.solve_problem())
ba.close()
ba = make(p, K, True, 0, 3)
s = ba.solve_problem()   # wide launch 1 steps aside after 3 iterations, wide launch 2 — the continuation — reports "gave up": run again
forms, gave_up = ba.solve_forms()
print("forms", forms, "gave up", gave_up, "fallbacks", ba.last_stats().fallbacks, "iterations", s.iterations, flush=True)
assert ref[0] > 3
assert bits(ba, s) == ref
assert ba.last_stats().fallbacks == 1 and gave_up == 1, (ba.last_stats().fallbacks, gave_up)
ba.close()
print("giveup ok", flush=True)
'''

_GROUP = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import stereo_vo_amd as S
from test_pipeline import _seq
from test_group import _group, KEY
n, lanes, batch, seed0 = 16, 8, 8, 0x5EED0F00
seqs = [_seq(n, seed=seed0 + 11 * i) for i in range(lanes)]
p0 = seqs[0][0]
Ls = np.stack([s[1] for s in seqs]); Rs = np.stack([s[2] for s in seqs])
ctx = S.Context(p0.width, p0.height, max_batch=lanes * batch, max_corners=600, max_candidates=1 << 16, max_features=600)
g = _group(S, ctx, p0, 600, 10.0, 600, lanes)
got = [[] for _ in range(lanes)]
for b0 in range(0, n, batch):
    dl, dr = torch.from_numpy(Ls[:, b0:b0 + batch].copy()).cuda(), torch.from_numpy(Rs[:, b0:b0 + batch].copy()).cuda()
    res = g.process_batch_dev(dl.data_ptr(), dr.data_ptr(), batch * p0.width * p0.height, batch)
    torch.cuda.synchronize()
    for l in range(lanes):
        got[l] += res[l]
forms, gave_up = g.solve_forms()
resumes = g.solve_resumes()
print("forms", forms, "gave up", gave_up, "resumes", resumes, flush=True)
pp = S.pipeline_default_params()
pp.cam.focal, pp.cam.cx, pp.cam.cy, pp.cam.baseline = p0.focal, p0.cx, p0.cy, p0.baseline
pp.width, pp.height = p0.width, p0.height
pp.max_corners, pp.min_feature_distance, pp.max_features, pp.window_size = 600, 10.0, 600, 5
pp.ba_max_time_s = 0.0
for l in range(lanes):
    single = S.Pipeline(ctx, pp)
    ref = single.process_batch(seqs[l][1], seqs[l][2])
    single.close()
    assert [KEY(r) for r in got[l]] == [KEY(r) for r in ref], l
assert gave_up == 0, gave_up
assert resumes > 0, resumes
print("group ok", flush=True)
'''


def _run(code, env=None, timeout=600, **kw):
    e = dict(os.environ)
    for name in ("SVO_BA_WAVE_CHUNKS", "SVO_BA_WAVE_ORDER", "SVO_BA_FORM", "SVO_BA_OVERFLOW", "SVO_BA_BUDGET_PERCENT", "SVO_BA_TEST_GIVEUP", "SVO_BA_YIELD_ITERS"):
        e.pop(name, None)
    e.update(env or {})
    return subprocess.run([sys.executable, "-c", code % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), **kw)], env=e, capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
def test_hip_wide_solve_that_yields_equals_the_host_driven_loop_at_every_budget():
    """Five windows (4 to 74 chunks, 24 to 50 LM iterations, 1 to 11 rejected steps, one that stops at the iteration cap), yield budgets
    1, 2, 3, 7, 10, 25 and 64 at k = 2, 3 and the limit: iterations, termination, both costs, poses and landmarks are the host-driven
    loop's bit for bit; linearize_calls, step_calls and successful steps are those of the solve that never yields; the continuation
    launches number ceil(iterations / N) - 1 (the rule is derived at resumes_expected); no solve gives up."""
    out = _run(_EVERY_BUDGET, problems=_PROBLEMS, iterations=_ITERATIONS, budgets=_BUDGETS)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "every budget ok" in out.stdout, (out.stdout[-800:], out.stderr[-3000:])


@pytest.mark.gpu
def test_hip_forms_that_never_yield_keep_their_bits_with_a_budget_set():
    """Windows of one and two chunks run ba_lm_kernel (one chunk per wavefront) whatever the budget: no continuation launch, the
    host-driven loop's bits, although they run more LM iterations than the budget."""
    out = _run(_NEVER, problems=[(61, 2, 12), (62, 2, 40)])
    print(out.stdout[-1000:])
    assert out.returncode == 0 and "never ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


@pytest.mark.gpu
def test_hip_one_launch_of_solves_with_different_budgets_gives_each_its_own_bits():
    """Six adjusters with budgets 0, 1, 3, 3, 7 and 64 leave as ONE ba_lm_multi_kernel launch (svo_ba_solve_problems); those that step
    aside are launched again until they are done.  Each ends with the bits it has alone on the host-driven loop."""
    out = _run(_SHARED, problems=[(64, 4, 90), (65, 5, 120), (51, 5, 500), (41, 5, 1500), (76, 3, 1800), (66, 6, 200)], budgets=[0, 1, 3, 3, 7, 64])
    print(out.stdout[-1000:])
    assert out.returncode == 0 and "shared ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


@pytest.mark.gpu
def test_hip_continuation_that_gives_up_is_run_again_from_the_image():
    """Budget 3 with SVO_BA_TEST_GIVEUP=2: the adjuster's second wide launch — the continuation of a solve that stepped aside — reports
    "gave up".  The solve is run again from its problem image, ends with the host-driven loop's bits and counts one fallback."""
    out = _run(_GIVEUP, env={"SVO_BA_TEST_GIVEUP": "2"}, problem=(65, 5, 120))
    print(out.stdout[-600:])
    assert out.returncode == 0 and "giveup ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


@pytest.mark.gpu
def test_hip_group_whose_solves_yield_keeps_parity_with_single_pipelines():
    """8 lanes, 16 frames, SVO_BA_YIELD_ITERS=2: the lanes' window solves step aside every two LM iterations and ride the group's later
    wide launches.  Every lane == its own svo_pipeline frame for frame, solves were continued, none gave up."""
    out = _run(_GROUP, env={"SVO_BA_YIELD_ITERS": "2"})
    print(out.stdout[-600:])
    assert out.returncode == 0 and "group ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
