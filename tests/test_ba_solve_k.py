"""k (chunks per wavefront of the wide window solve, ba_lm_multi_kernel) chosen per solve where the solve is admitted: a solve the
admission budget refuses at the default k rides the launch at a larger one instead of leaving in the one-workgroup form.  Every chunk
still posts its own partials and level 2 sums them in the declared order, so no k changes a bit; solves of different k share a launch.
CPU part: the turn arithmetic (csrc/lm_turns.h) compiled for the host."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_turns_cover_every_chunk_once_for_every_k(tmp_path):
    """csrc/lm_turns.h — the text ba_lm_multi_kernel compiles — walked on the host under ASan + UBSan: for 1..300 chunks, every k up to
    the limit and both chunk -> wavefront orders every chunk is taken exactly once, no wavefront takes more than k turns, and the
    workgroup count falls monotonically with k."""
    exe = str(tmp_path / "lm_turns_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "stereo_vo_amd", "csrc"), os.path.join(ROOT, "tests", "sanitize", "lm_turns_test.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "lm turns ok" in r.stdout


def test_wave_chunks_limit_is_what_the_header_says():
    """The library reports the limit of lm_turns.h (the tests below walk every k up to it) and refuses a k beyond it."""
    import re
    import stereo_vo_amd as S
    txt = open(os.path.join(ROOT, "stereo_vo_amd", "csrc", "lm_turns.h")).read()
    limit = int(re.search(r"constexpr int LM_MAX_WAVE_CHUNKS = (\d+);", txt).group(1))
    assert S.lib().svo_ba_wave_chunks_limit() == limit and limit >= 4
    assert S.lib().svo_ba_set_wave_chunks(None, 1) != 0


# (seed, poses, landmarks): windows of 2..14 poses, from one chunk to ~250 (C < 2k and C mod 2k != 0 among them; beyond 128 chunks the
# grouped kernel keeps one chunk per wavefront whatever k is asked for)
_PROBLEMS = [(61, 2, 12), (62, 2, 40), (63, 3, 50), (64, 4, 90), (65, 5, 120), (66, 6, 200), (67, 7, 400), (68, 8, 700),
             (69, 9, 1000), (70, 10, 1300), (75, 5, 2300), (76, 3, 1800), (77, 11, 700), (78, 12, 600), (79, 13, 500), (80, 14, 450),
             (41, 5, 1500), (42, 8, 2600)]

_HEAD = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np
import stereo_vo_amd as S
import ba_problem as BP
ctx = S.Context(64, 64)
LIMIT = S.lib().svo_ba_wave_chunks_limit()
def make(p, K, dev, k=0):
    ba = S.api.BA(ctx, max(K, 2), BP.F, BP.CX, BP.CY, max_landmarks=len(p["points0"]) + 8, max_observations=len(p["op"]) + 8, max_time_s=0.0,
                  device_lm=dev, solve_form="wide" if dev else None, accumulation="deterministic")
    if k:
        ba.set_wave_chunks(k)
    ba.load_problem(p["poses0"], p["points0"], p["op"], p["oj"], p["uv"])
    return ba
def bits(ba, s):
    poses, pts = ba.read_problem()
    return (s.iterations, s.termination, s.initial_cost, s.final_cost, poses.tobytes(), pts.tobytes())
'''

_EVERY_K = _HEAD + r'''
ran = [0] * (LIMIT + 1)
for seed, K, N in %(problems)r:
    p = BP.make_problem(seed, K, N)
    ba = make(p, K, False)
    ref = bits(ba, ba.solve_problem())
    ba.close()
    for k in range(1, LIMIT + 1):
        ba = make(p, K, True, k)
        got = bits(ba, ba.solve_problem())
        forms, gave_up = ba.solve_forms()
        assert ba.last_stats().fallbacks == 0 and gave_up == 0 and forms[0] == 0, (seed, K, N, k, forms, gave_up)
        assert sum(forms) <= 1 and all(f == 0 for i, f in enumerate(forms) if i not in (1, k)), (seed, K, N, k, forms)
        ran[k] += forms[k]
        ba.close()
        assert got == ref, (seed, K, N, k, len(p["op"]), got[:4], ref[:4])
print("ran", ran, flush=True)
assert all(r >= 6 for r in ran[1:]), ran
print("every k ok", flush=True)
'''

_MIXED = _HEAD + r'''
problems = %(problems)r
ks = [2, 3, 5, LIMIT, 4, 6, 7, 3, 2, LIMIT][:len(problems)]
ps = [BP.make_problem(seed, K, N) for seed, K, N in problems]
alone = []
for p, (seed, K, N) in zip(ps, problems):
    ba = make(p, K, False)
    alone.append(bits(ba, ba.solve_problem()))
    ba.close()
bas = [make(p, K, True, k) for p, (seed, K, N), k in zip(ps, problems, ks)]
shared, sums = S.api.BA.solve_problems(bas)
print("shared", shared, flush=True)
assert shared == len(bas), shared
for i, (ba, s) in enumerate(zip(bas, sums)):
    forms, gave_up = ba.solve_forms()
    assert gave_up == 0 and forms[ks[i]] == 1 and sum(forms) == 1, (i, ks[i], forms, gave_up)
    assert bits(ba, s) == alone[i], (i, problems[i], ks[i])
    ba.close()
print("mixed ok", flush=True)
'''

_GROUP = r'''
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import stereo_vo_amd as S
from test_pipeline import _seq
from test_group import _group, KEY
n, lanes, batch, seed0 = 16, %(lanes)d, 8, 0x5EED0F00
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
print("forms", forms, "gave up", gave_up, flush=True)
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
assert sum(forms[%(default_k)d + 1:]) > 0, forms
print("group ok", flush=True)
'''


def _run(code, env=None, timeout=600, **kw):
    e = dict(os.environ)
    for name in ("SVO_BA_WAVE_CHUNKS", "SVO_BA_WAVE_ORDER", "SVO_BA_FORM", "SVO_BA_OVERFLOW", "SVO_BA_BUDGET_PERCENT", "SVO_BA_TEST_GIVEUP"):
        e.pop(name, None)
    e.update(env or {})
    return subprocess.run([sys.executable, "-c", code % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), **kw)], env=e, capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
def test_hip_wide_solve_equals_the_host_driven_loop_at_every_k_the_admission_can_choose():
    """Windows of 2..14 poses, one chunk to ~250: poses, landmarks, costs and iteration counts of the wide solve at k = 1 .. the limit
    (svo_ba_set_wave_chunks) are the host-driven loop's, bit for bit; no solve gives up; the solves did run at the k asked for."""
    out = _run(_EVERY_K, problems=_PROBLEMS)
    print(out.stdout[-600:])
    assert out.returncode == 0 and "every k ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


@pytest.mark.gpu
def test_hip_one_launch_of_solves_with_different_k_gives_each_its_own_bits():
    """Ten adjusters with different windows and k = 2 .. the limit leave as ONE ba_lm_multi_kernel launch (svo_ba_solve_problems: the
    grid as wide as the widest solve, the dynamic LDS that of the largest): each ends with the bits it has alone on the host-driven loop."""
    out = _run(_MIXED, problems=[(64, 4, 90), (65, 5, 120), (66, 6, 200), (67, 7, 400), (68, 8, 700), (69, 9, 1000), (70, 10, 1300), (75, 5, 2300), (76, 3, 1800), (51, 5, 500)])
    print(out.stdout[-600:])
    assert out.returncode == 0 and "mixed ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])


@pytest.mark.gpu
def test_hip_group_with_a_squeezed_budget_rides_at_larger_k_and_keeps_parity():
    """24 lanes with windows of up to ~45 chunks and a tenth of the admission budget (44 workgroups for the process), one compact line:
    refused solves ride the group's wide launches at k above the default.  Every lane == its own svo_pipeline frame for frame, no
    solve gave up, and the group's solve-form counts show solves above the default k."""
    out = _run(_GROUP, env={"SVO_GROUP_COMPACT_LINES": "1", "SVO_BA_BUDGET_PERCENT": "10"}, lanes=24, default_k=3)
    print(out.stdout[-600:])
    assert out.returncode == 0 and "group ok" in out.stdout, (out.stdout[-500:], out.stderr[-3000:])
