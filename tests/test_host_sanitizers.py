"""AddressSanitizer + UndefinedBehaviorSanitizer over the GPU-free host code of the product (the step control
host/lm.cpp, the dense Cholesky, the KITTI-layout decoders, the track rasteriser, the synthetic renderer, and the three
GPU-free pieces of the bundle adjuster: the sliding-window graph host/ba_graph.h, the problem layout host/ba_layout.h, the
admission ledger host/ba_admission.h, the launch planning of its device-resident solve host/ba_plan.h with the kernels' LDS sizes
csrc/lm_lds.h (tests/sanitize/ba_plan_test.cpp), and the argument rules, sizes and launch geometry of the dense keyframe chain
host/dense_args.h), and the pose conversions host/det_trig.h at their branches (tests/sanitize/det_trig_test.cpp), on the CPU: GPU sanitizers are not available on the target pool, and these are the
pieces that parse files and index host arrays.  Every program is stand-alone (its own main); nothing is loaded into Python."""
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunk(t, data):
    return struct.pack(">I", len(data)) + t + data + struct.pack(">I", zlib.crc32(t + data) & 0xFFFFFFFF)


def _write_inputs(d):
    from PIL import Image
    rng = np.random.default_rng(5)
    g = rng.integers(0, 256, (37, 53)).astype(np.uint8)
    Image.fromarray(g).save(os.path.join(d, "ok_gray.png"))
    Image.fromarray(rng.integers(0, 256, (20, 31, 3)).astype(np.uint8)).save(os.path.join(d, "ok_rgb.png"))
    Image.fromarray((g.astype(np.uint32) * 257).astype(np.uint16)).save(os.path.join(d, "ok_gray16.png"))
    open(os.path.join(d, "ok_p5.pgm"), "wb").write(b"P5\n# c\n53 37\n255\n" + g.tobytes())
    sig = b"\x89PNG\r\n\x1a\n"
    ihdr = struct.pack(">IIBBBBB", 4, 4, 8, 0, 0, 0, 0)
    idat = zlib.compress(b"".join(b"\x00" + bytes([10 * r] * 4) for r in range(4)))
    bad = {
        "bad_short_ihdr.png": sig + _chunk(b"IHDR", ihdr[:5]) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"") + b"\0" * 16,
        "bad_no_ihdr.png": sig + _chunk(b"IDAT", idat) + _chunk(b"IEND", b"") + b"\0" * 32,
        "bad_two_ihdr.png": sig + _chunk(b"IHDR", ihdr) + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b""),
        "bad_zero.png": sig + _chunk(b"IHDR", struct.pack(">IIBBBBB", 0, 4, 8, 0, 0, 0, 0)) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b""),
        "bad_huge.png": sig + _chunk(b"IHDR", struct.pack(">IIBBBBB", 70000, 4, 8, 0, 0, 0, 0)) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b""),
        "bad_len.png": sig + struct.pack(">I", 0xFFFFFFF0) + b"IHDR" + ihdr + b"\0" * 8,
        "bad_short_idat.png": sig + _chunk(b"IHDR", struct.pack(">IIBBBBB", 64, 64, 8, 0, 0, 0, 0)) + _chunk(b"IDAT", idat) + _chunk(b"IEND", b""),
        "bad_filter.png": sig + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(b"".join(b"\x09" + bytes(4) for _ in range(4)))) + _chunk(b"IEND", b""),
        "bad_truncated.png": (sig + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", idat))[:40],
        "bad_neg.pgm": b"P5\n-1 -1\n255\n" + b"\0" * 4,
        "bad_overflow.pgm": b"P5\n99999999999999999999 2\n255\n" + b"\0" * 4,
        "bad_zero.pgm": b"P5\n0 7\n255\n",
        "bad_truncated.pgm": b"P5\n8 8\n255\n" + b"\0" * 10,
        "bad_empty.png": b"",
    }
    for name, blob in bad.items():
        open(os.path.join(d, name), "wb").write(blob)
    rows = ["%e " * 11 % tuple(range(11)) + "1.0" for _ in range(3)] + ["1 2 3"]
    open(os.path.join(d, "poses.txt"), "w").write("\n".join(rows) + "\n")


def test_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    host = os.path.join(ROOT, "stereo_vo_amd", "host")
    exe = str(tmp_path / "host_sanitize")
    srcs = [os.path.join(ROOT, "tests", "sanitize", "host_sanitize.cpp")] + \
           [os.path.join(host, f) for f in ("lm.cpp", "linalg.cpp", "kitti_io.cpp", "draw.cpp", "synth.cpp")]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", host, "-I", os.path.join(ROOT, "stereo_vo_amd", "csrc")] + \
          srcs + ["-o", exe, "-lz", "-lpthread"]
    subprocess.run(cmd, check=True, timeout=600)
    d = tmp_path / "inputs"
    d.mkdir()
    _write_inputs(str(d))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "host sanitize ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_xcd_aware_block_map_serves_every_slot_exactly_once(tmp_path):
    """The item -> workgroup map of the grouped tracking / sparse-stereo launches (csrc/xcd_map.h): the device function's own text
    compiled for the host walks whole grids — every (lane, item) slot once, max(n, 1) workgroups per lane (what the lanes'
    arrival targets count), contiguous runs per XCD label — under ASan + UBSan."""
    exe = str(tmp_path / "xcd_map_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "stereo_vo_amd", "csrc"), os.path.join(ROOT, "tests", "sanitize", "xcd_map_test.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "xcd map ok" in r.stdout


def test_group_line_policy_partitions_gathers_and_orders_solves(tmp_path):
    """The line policy of a pipeline group (host/group_lines.h: which queued lanes ride which line, the gather rule, the order in
    which assembled solves are offered to the admission), the functions host/group.cpp calls, walked on the CPU under ASan + UBSan:
    the lines partition the queue in queue order, gather off is always ripe, gather on holds a line back in exactly one case, the
    solve order is a strict weak ordering that never puts a waiting lane behind a non-waiting one."""
    exe = str(tmp_path / "group_lines_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "stereo_vo_amd", "host"), os.path.join(ROOT, "tests", "sanitize", "group_lines_test.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "group lines ok" in r.stdout


def _run_sanitized(tmp_path, name, ok, *args):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "stereo_vo_amd", "host"),
           "-I", os.path.join(ROOT, "stereo_vo_amd", "csrc"), os.path.join(ROOT, "tests", "sanitize", name + ".cpp"), "-o", exe, "-lpthread"]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert ok in r.stdout
    return r.stdout


def test_ba_graph_ids_truncation_window_gather_and_write_back(tmp_path):
    """The sliding-window graph of the bundle adjuster (host/ba_graph.h), walked on the CPU under ASan + UBSan: sequential ids,
    truncation at max_features, the window pop, an unknown id rejected with nothing committed, gather() against a sort-based
    restatement on the merge path and on the stable-sort path (and the two on the same observations), write_back, reset."""
    _run_sanitized(tmp_path, "ba_graph_test", "ba graph ok")


def test_ba_layout_tables_match_a_brute_force_restatement(tmp_path):
    """The host half of the declared summation order (host/ba_layout.h), walked on the CPU under ASan + UBSan: chunks, dimensions
    and the per-chunk destination tables against a brute-force restatement, entry for entry and in order, for K = 1, 2, 3, 5, 9;
    chunk boundaries; more than 128 and more than 2,048 chunks; the staging image; every rejection at its boundary."""
    _run_sanitized(tmp_path, "ba_layout_test", "ba layout ok")


def test_ba_admission_ledger_within_and_across_processes(tmp_path):
    """The admission ledger (host/ba_admission.h), walked on the CPU under ASan + UBSan with its table file in a temporary
    directory: the budget within a process, a forked child's workgroups counted against the parent's budget, the slot of a
    process that died without releasing, and the per-process admission without a file."""
    d = tmp_path / "table"
    d.mkdir()
    _run_sanitized(tmp_path, "ba_admission_test", "ba admission ok", str(d))


def test_dense_args_rules_sizes_and_launch_geometry_at_their_boundaries(tmp_path):
    """The dense keyframe chain's host logic (host/dense_args.h), walked on the CPU under ASan + UBSan: the StereoBM shape and batch
    rules, the cloud, speckle, left-right and SGM rules, each accepted at its limit and refused one step beyond with its entry's
    message; chunk, seam and path-grid counts against brute-force counts; the SGM workspace's regions aligned and disjoint, up to
    2^30 pixels; the keyframe clouds' resolved parameters, buffer sizes and sub-batch split."""
    _run_sanitized(tmp_path, "dense_args_test", "dense args ok")


def test_ba_plan_sizes_forms_budget_and_raised_k_match_a_restatement(tmp_path):
    """The launch planning of the device-resident window solve (host/ba_plan.h, csrc/lm_lds.h), walked on the CPU under ASan + UBSan
    against restatements written from the rules: the LDS sizes of the wide and the compact form (monotone in k and in the waves, the
    union, the tail, n = 36 pinned), form / k / eligibility for every C up to 300 with every boundary at its limit and one beyond, the
    compact form's waves against a linear search and the shape of a mixed launch, budget and cost, the raise of k against a fake
    occupancy and a fake ledger (nothing admissible skipped, nothing offered behind the occupancy drop, no offer that saves no
    workgroup, an adjuster's own k never raised), and every knob parsed from unset, empty, in-range, out-of-range and non-numeric
    strings."""
    _run_sanitized(tmp_path, "ba_plan_test", "ba plan ok")


def test_host_call_order_rule_and_parts_carver_match_a_restatement(tmp_path):
    """What every synchronous entry shares (host/host_call.h), walked on the CPU under ASan + UBSan with a fake error type: all 16
    combinations of {the copies up fail, the _dev entry refuses, the copies back fail, the drain fails} against a restatement of the
    rule (which callables ran and in what order, the drain exactly once and last, the returned code, the reported error), a refusal's
    way into the context, and the parts carver (offsets multiples of 256, parts disjoint and in order, empty parts take no room, the
    total at least the parts' sum, sizes up to 2^40)."""
    _run_sanitized(tmp_path, "host_call_test", "host call ok")


def _det_trig_inputs():
    """rvecs (n, 3) f64 and matrices (m, 9) f32 at every branch of host/det_trig.h."""
    F, eps = np.float32, np.float32(2.0 ** -52)                         # cv::Rodrigues' small-angle threshold DBL_EPSILON is a float, too
    axes = [np.array(a, float) for a in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, 0, -1), (0.48, -0.6, 0.64), (0.6, 0.64, 0.48), (-0.64, 0.48, 0.6))]
    mags = [0.0, float(np.nextafter(eps, F(0))), float(eps), float(np.nextafter(eps, F(1))), 1e-20, 1e-300,
            float(np.nextafter(1e-12, 0)), 1e-12, float(np.nextafter(1e-12, 1)), 1e-7, 0.3, 0.5, float(np.nextafter(0.5, 1)), 1.0,
            np.pi - 1e-3, np.pi - 1e-7, float(np.nextafter(F(np.pi), F(0))), np.pi, float(F(np.pi)), np.pi + 1e-7, np.pi + 1e-3, 4.0, 6.0]
    mags += list(np.deg2rad(np.arange(118.0, 181.0, 1.0)))             # 120 ... 180 degrees: the trace turns negative on the way
    rv = np.array([a * m for a in axes for m in mags])
    mats = []
    rng = np.random.default_rng(7)
    vals = (-1.0, -0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0)
    for a in vals:
        for b in vals:
            for c in vals:
                big = max(a, b, c)
                if a + b + c > 0.5 or 1.0 + 2.0 * big - (a + b + c) <= 0:    # a few with a positive trace; the root stays real
                    continue
                m = rng.uniform(-1, 1, (3, 3))
                m[0, 0], m[1, 1], m[2, 2] = a, b, c
                mats.append(m.ravel())
    return rv, np.array(mats, F)


def test_pose_conversions_at_their_branches_match_the_restatements(tmp_path):
    """host/det_trig.h: svo_det_rodrigues_f, svo_det_quat_from_R, svo_det_quat_from_rvec and svo_det_rvec_from_quat, compiled for the
    host under ASan + UBSan and run on rvecs of length 0, either side of 2^-52 and of 1e-12, near pi and from 118 to 180 degrees about
    x, y, z and skew axes, and on matrices with a positive, a zero and a negative trace, each diagonal entry largest, with ties on the
    diagonal.  Every result equals, bit for bit, the restatements in tests/pipeline_ref.py (cv::Rodrigues, Eigen::Quaternionf(Matrix3f))
    and tests/pnp_ref.py (rvec <-> quaternion); the restatement's counters show that all four quaternion branches and the small-angle
    branches ran."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pipeline_ref as PR
    import pnp_ref
    rv, mats = _det_trig_inputs()
    path = tmp_path / "det_trig_inputs.bin"
    path.write_bytes(np.array([len(rv), len(mats)], "<i4").tobytes() + rv.astype("<f8").tobytes() + mats.astype("<f4").tobytes())
    lines = _run_sanitized(tmp_path, "det_trig_test", "det trig ok", str(path)).splitlines()
    assert len(lines) == len(rv) + len(mats) + 1

    def f32(words):
        return np.array([int(w, 16) for w in words], np.uint32)

    def f64(words):
        return np.array([int(w, 16) for w in words], np.uint64)
    rec = dict.fromkeys(PR.COUNTERS, 0)
    flips = {"quat_flip": 0}
    tie01 = tie2 = small_q = small_v = 0
    for r, line in zip(rv, lines):
        w = line.split()
        assert w[0] == "v" and len(w) == 1 + 9 + 4 + 4 + 3 + 3
        R = PR.rodrigues_f(r.astype(np.float32), rec)
        q = pnp_ref.quat_from_rvec([float(v) for v in r])
        small_q += np.linalg.norm(r) < 1e-12
        small_v += np.linalg.norm(q[1:]) < 1e-12
        want = [R.view(np.uint32).ravel(), PR.quat_from_R(R, rec).view(np.uint32), np.array(q).view(np.uint64),
                np.array(pnp_ref.rvec_from_quat(q, flips)).view(np.uint64), np.array(pnp_ref.rvec_from_quat([-v for v in q], flips)).view(np.uint64)]
        got = [f32(w[1:10]), f32(w[10:14]), f64(w[14:18]), f64(w[18:21]), f64(w[21:24])]
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (r.tolist(), k, a, b)
    for m, line in zip(mats, lines[len(rv):]):
        w = line.split()
        assert w[0] == "m" and len(w) == 5
        assert np.array_equal(f32(w[1:]), PR.quat_from_R(m.reshape(3, 3), rec).view(np.uint32)), m.tolist()
        if m[0] + m[4] + m[8] <= 0:
            tie01 += m[4] == m[0]
            tie2 += m[8] == max(m[0], m[4])
    assert min(rec[k] for k in ("quat_trace_pos", "quat_x", "quat_y", "quat_z", "rodrigues_small")) > 0, rec
    assert flips["quat_flip"] > 0 and tie01 > 0 and tie2 > 0 and small_q > 0 and small_v > 0
    assert any(m[0] + m[4] + m[8] == 0 for m in mats)
