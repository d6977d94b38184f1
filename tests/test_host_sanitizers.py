"""AddressSanitizer + UndefinedBehaviorSanitizer over the GPU-free host code of the product (the step control
host/lm.cpp, the dense Cholesky, the KITTI-layout decoders, the track rasteriser, the synthetic renderer, and the three
GPU-free pieces of the bundle adjuster: the sliding-window graph host/ba_graph.h, the problem layout host/ba_layout.h, the
admission ledger host/ba_admission.h, the launch planning of its device-resident solve host/ba_plan.h with the kernels' LDS sizes
csrc/lm_lds.h (tests/sanitize/ba_plan_test.cpp), and the argument rules, sizes and launch geometry of the dense keyframe chain
host/dense_args.h), on the CPU: GPU sanitizers are not available on the target pool, and these are the
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
