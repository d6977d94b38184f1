"""Semi-global matching (include/svo.h, "semi-global matching"): the restatement tests/sgm_ref.py against itself and
against the two StereoBM restatements (CPU), then the device entries against it with `==` (GPU).

Figures the CPU tests pin (all reproduced by route (a); scene = stereo_bm_ref.scene(96, 192, 32, 2) at (32, 9), p1 = 81, p2 = 324):
  mutations, pixels of the map that change: d +- 2 2,202; one neighbour 6,175; no "- m" 7,065; three paths (right->left missing) 924;
      both directions of each axis run forward 2,421.  (Other readings of the last two: top->bottom / bottom->top / left->right
      missing 1,270 / 2,034 / 799; the horizontal axis alone forward twice 925, the vertical alone 2,284.)
  winners of the min per (step, d), same-d first, then adjacent, then far, and same-d == far:
      the scene 291,717 / 148,937 / 1,267,314 / 73,430;  lr_check_ref.occlusion_pair() 58,168 / 112,634 / 1,537,166 / 23
  valid pixels 10,446 against StereoBM's 8,870, 2,991 pixels different.
  weak texture (sgm_ref.planes_pair, 96 x 192, two half-planes, texture 100 +- 3, noise +- 3 per eye, defaults): StereoBM keeps
      6,302 (5,835 within 1 px of truth), semi-global matching 12,838 (11,887)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lr_check_ref as LR
import sgm_ref as SG
import speckle_ref as SP
import stereo_bm_ref as BM
from test_stereo_paths import GRID, NARROW

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _scene():
    if "scene" not in _CACHE:
        L, R = BM.scene(96, 192, 32, 2)
        counts = {}
        m, c = SG.sgm(L, R, 32, 9, 81, 324, counts=counts)
        for a in (L, R, m, c):
            a.setflags(write=False)
        _CACHE["scene"] = (L, R, m, c, counts)
    return _CACHE["scene"]


# ------------------------------------------------------------------------------------------------ CPU
def test_abi_symbols_argtypes_header_and_python_names():
    import stereo_vo_amd as S
    from stereo_vo_amd import api
    L = S.lib()
    names = ["svo_sgm_default_params", "svo_sgm_workspace_bytes", "svo_stereo_sgm_batch_dev", "svo_stereo_sgm",
             "svo_pipeline_set_keyframe_sgm", "svo_pipeline_group_set_keyframe_sgm"]
    hdr = open(os.path.join(ROOT, "include", "svo.h")).read()
    for n in names:
        assert hasattr(L, n) and n in api.SYMBOLS and re.search(r"\b%s\s*\(" % n, hdr), n
    assert len(L.svo_stereo_sgm_batch_dev.argtypes) == 15 and L.svo_stereo_sgm_batch_dev.argtypes[7] is C.c_size_t
    assert L.svo_stereo_sgm_batch_dev.argtypes[12] is C.c_size_t and len(L.svo_stereo_sgm.argtypes) == 11
    assert L.svo_sgm_workspace_bytes.restype is C.c_size_t and len(L.svo_sgm_workspace_bytes.argtypes) == 5
    assert re.search(r"#define\s+SVO_SGM_MAX_P2\s+32767\b", hdr) and api.SGM_MAX_P2 == 32767 == SG.MAX_P2
    sub = re.search(r"#define\s+SVO_SGM_KEYFRAME_SUB_BATCH\s+(\d+)", hdr)
    assert sub and int(sub.group(1)) == api.SGM_KEYFRAME_SUB_BATCH >= 1
    assert re.search(r"typedef struct svo_sgm_params \{\s*int p1;.*?int p2;", hdr, re.S)
    assert [f[0] for f in api.SgmParams._fields_] == ["p1", "p2"] and C.sizeof(api.SgmParams) == 8
    assert '"stereo_sgm"' in hdr and "NOT tuned on real imagery" in hdr and "parity with OpenCV's SGBM is NOT" in hdr
    for cls, meths in ((api.Context, ("stereo_sgm", "stereo_sgm_batch", "sgm_workspace_bytes")), (api.Pipeline, ("set_keyframe_sgm",)),
                       (api.PipelineGroup, ("set_keyframe_sgm",))):
        for m in meths:
            assert callable(getattr(cls, m)), (cls, m)
    for block in (5, 9, 21):
        p = api.sgm_default_params(block)
        assert (p.p1, p.p2) == (2 * block * block, 8 * block * block) == SG.default_params(block)
    for bad in (4, 3, 23, 0):
        assert L.svo_sgm_default_params(C.byref(api.SgmParams()), bad) == -1
    assert L.svo_sgm_default_params(None, 9) == -1


def test_workspace_bytes_is_pure_and_zero_for_a_refused_shape():
    from stereo_vo_amd import api
    up = lambda v: (v + 255) & ~255
    for w, h, nd, bl, b in [(1241, 376, 48, 21, 1), (192, 96, 32, 9, 3), (131, 61, 16, 5, 3), (200, 64, 64, 7, 2)]:
        px = (w - bl - nd + 2) * (h - bl + 1) * b
        assert api.sgm_workspace_bytes(w, h, nd, bl, b) == up(2 * px * nd) + up(4 * px * nd) + up(2 * px), (w, h, nd, bl, b)
    assert 119e6 < api.sgm_workspace_bytes(1241, 376, 48, 21, 1) < 123e6
    assert api.sgm_workspace_bytes(39, 64, 32, 9, 3) == 256 == api.sgm_workspace_bytes(192, 8, 32, 9, 1)   # an empty rectangle
    assert api.sgm_workspace_bytes(40, 9, 32, 9, 1) == 3 * 256                                           # one pixel
    for w, h, nd, bl, b in [(2, 96, 32, 9, 1), (192, 2, 32, 9, 1), (192, 96, 24, 9, 1), (192, 96, 80, 9, 1), (192, 96, 0, 9, 1),
                            (192, 96, 32, 8, 1), (192, 96, 32, 23, 1), (192, 96, 32, 3, 1), (192, 96, 32, 9, 0), (192, 96, 32, 9, 65536),
                            (-5, 96, 32, 9, 1), (40000, 40000, 32, 9, 1)]:
        assert api.sgm_workspace_bytes(w, h, nd, bl, b) == 0, (w, h, nd, bl, b)


@pytest.mark.parametrize("h,w,nd,bl,p1,p2", [(40, 56, 16, 5, 50, 200), (40, 56, 16, 5, 60, 60), (40, 56, 16, 5, 0, 90), (40, 56, 16, 5, 0, 0),
                                             (30, 48, 16, 7, 98, 392), (33, 20, 16, 5, 50, 200), (5, 56, 16, 5, 50, 200), (30, 19, 16, 5, 1, 2)],
                         ids=["defaults", "p1_eq_p2", "p1_zero", "zero", "block7_odd_height", "one_column", "one_row", "empty"])
def test_the_two_routes_agree(h, w, nd, bl, p1, p2):
    L, R = BM.scene(h, w, nd, 3)
    a = SG.sgm(L, R, nd, bl, p1, p2)
    b = SG.sgm_pixels(L, R, nd, bl, p1, p2)
    valid = int((a[0] != SG.FILTERED).sum())
    print("valid", valid, "of", max(w - bl - nd + 2, 0) * max(h - bl + 1, 0))
    assert np.array_equal(a[0], np.array(b[0], np.int16)) and np.array_equal(a[1], np.array(b[1], np.uint16))
    assert ((a[1] == SG.NO_COST) == (a[0] == SG.FILTERED)).all()
    if w >= 48:
        assert valid >= (10 if h > 5 else 3)
    if w == 19:
        assert valid == 0


IDENTITY = [(k, False) for k in GRID] + [(k, True) for k in NARROW] + [("row", None), ("empty", None)]


@pytest.mark.parametrize("gid,narrow", IDENTITY, ids=[f"{k}{'_narrow' if n else ''}" for k, n in IDENTITY])
def test_zero_penalties_are_block_matching(gid, narrow):
    if gid == "row":
        nd, bl, h, w, seed = 32, 9, 9, 150, 4       # a single valid row: H = block
    elif gid == "empty":
        nd, bl, h, w, seed = 32, 9, 40, 39, 4       # W = ndisp - 1 + block - 1
    else:
        nd, bl, h, w, seed = (NARROW if narrow else GRID)[gid]
    L, R = BM.scene(h, w, nd, seed)
    m, c = SG.sgm(L, R, nd, bl, 0, 0)
    want = BM.stereo_bm(L, R, nd, bl)
    assert np.array_equal(m, want) and np.array_equal(c, LR.min_sad(L, R, nd, bl))
    x0, x1, y0, y1 = BM.valid_rect(h, w, nd, bl)
    if gid == "empty":
        assert x1 <= x0 and (m == SG.FILTERED).all()
    else:
        assert (want != SG.FILTERED).sum() >= (5 if narrow or gid == "row" else 500)
        assert (x1 - x0 == 1) == bool(narrow) and (y1 - y0 == 1) == (gid == "row")


@pytest.mark.parametrize("mutation,changed", zip(SG.MUTATIONS, (2202, 6175, 7065, 924, 2421)))
def test_every_mutation_changes_the_scene(mutation, changed):
    L, R, m, c, _ = _scene()
    got = SG.sgm(L, R, 32, 9, 81, 324, mutation=mutation)[0]
    assert int((got != m).sum()) == changed
    Lo, Ro = LR.occlusion_pair()
    assert (SG.sgm(Lo, Ro, 32, 9, 81, 324, mutation=mutation)[0] != SG.sgm(Lo, Ro, 32, 9, 81, 324)[0]).sum() >= 50


def test_recorded_branch_counts():
    L, R, m, c, counts = _scene()
    assert counts == dict(same=291717, adjacent=148937, far=1267314, same_ties_far=73430)
    assert sum(counts[k] for k in ("same", "adjacent", "far")) == 32 * (2 * 88 * 152 + 2 * 153 * 87)
    oc = {}
    SG.sgm(*LR.occlusion_pair(), 32, 9, 81, 324, counts=oc)
    assert oc == dict(same=58168, adjacent=112634, far=1537166, same_ties_far=23)
    bm = BM.stereo_bm(L, R, 32, 9)
    assert (int((m != SG.FILTERED).sum()), int((bm != SG.FILTERED).sum()), int((m != bm).sum())) == (10446, 8870, 2991)


def test_weak_texture_is_filled():
    L, R = SG.planes_pair()
    truth = np.where(np.arange(192)[None, :] < 96, 6, 18) * 16
    near = lambda d: int(((d != SG.FILTERED) & (np.abs(d.astype(np.int64) - truth) <= 16)).sum())
    bm, sg = BM.stereo_bm(L, R, 32, 9), SG.sgm(L, R, 32, 9)[0]
    print("kept / within 1 px: block matching", int((bm != -16).sum()), near(bm), "semi-global", int((sg != -16).sum()), near(sg))
    assert near(sg) >= 2 * near(bm) and near(sg) >= 0.85 * 13464


def test_parameter_corners():
    L, R = BM.scene(96, 192, 32, 2)
    base = SG.sgm(L, R, 32, 9, 81, 324)[0]
    for p1, p2 in ((200, 200), (0, 324)):
        got = SG.sgm(L, R, 32, 9, p1, p2)[0]
        assert (got != base).sum() >= 100 and (got != BM.stereo_bm(L, R, 32, 9)).sum() >= 100, (p1, p2)
    info = {}
    Lb, Rb = BM.scene(80, 160, 48, 4)
    m = SG.sgm(Lb, Rb, 48, 21, 0, SG.MAX_P2, info=info)[0]
    print(info)
    assert 32767 < info["l_max"] < 65536 and info["l_max"] <= 27342 + SG.MAX_P2 and info["s_max"] > 65535 and (m != SG.FILTERED).sum() >= 100


# ------------------------------------------------------------------------------------------------ GPU
GUARD = 4096  # bytes behind every output and behind the work space that must stay as they were


def _pairs(w, h, nd):
    """Three distinct pairs: a band scene, its left-right mirror (another image), another seed."""
    key = ("pairs", w, h, nd)
    if key not in _CACHE:
        a, b = BM.scene(h, w, nd, 2), BM.scene(h, w, nd, 3)
        _CACHE[key] = [a, (np.ascontiguousarray(a[0][:, ::-1]), np.ascontiguousarray(a[1][:, ::-1])), b]
    return _CACHE[key]


def _want(w, h, nd, bl, p1, p2):
    key = ("want", w, h, nd, bl, p1, p2)
    if key not in _CACHE:
        _CACHE[key] = [SG.sgm(L, R, nd, bl, p1, p2) for L, R in _pairs(w, h, nd)]
    return _CACHE[key]


def _device_sgm(ctx, torch, pairs, nd, bl, p1, p2, cost=True, pad=0):
    """svo_stereo_sgm_batch_dev -> (maps, costs or None), (B, H, W); guard bands behind map, cost and work space; inputs unchanged."""
    from stereo_vo_amd import api
    B = len(pairs)
    h, w = pairs[0][0].shape
    n = B * h * w
    rs = w + pad
    ist = rs * h + (64 if pad else 0)
    host = []
    for eye in (0, 1):
        buf = np.random.default_rng(7 + eye).integers(0, 256, B * ist, dtype=np.uint8)
        for b in range(B):
            buf[b * ist:b * ist + rs * h].reshape(h, rs)[:, :w] = pairs[b][eye]
        host.append(buf)
    dl, dr = torch.from_numpy(host[0]).cuda(), torch.from_numpy(host[1]).cuda()
    need = api.sgm_workspace_bytes(w, h, nd, bl, B)
    assert need >= 256
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    dm = torch.from_numpy(np.full(n + GUARD // 2, 0x5A5A, np.uint16).view(np.int16)).cuda()
    dc = torch.from_numpy(np.full(n + GUARD // 2, 0x3C3C, np.uint16).view(np.int16)).cuda()
    torch.cuda.synchronize()
    ctx.stereo_sgm_batch(dl.data_ptr(), dr.data_ptr(), B, w, h, rs, ist, api.SgmParams(p1, p2), ws.data_ptr(), need, dm.data_ptr(),
                         dc.data_ptr() if cost else None, nd, bl)
    ctx.sync()
    m, c = dm.cpu().numpy(), dc.cpu().numpy().view(np.uint16)
    assert (m[n:].view(np.uint16) == 0x5A5A).all() and (c[n:] == 0x3C3C).all(), "bytes behind an output changed"
    assert (ws[need:].cpu().numpy() == 0xA5).all(), "bytes behind the work space changed"
    assert np.array_equal(dl.cpu().numpy(), host[0]) and np.array_equal(dr.cpu().numpy(), host[1]), "the images changed"
    if not cost:
        assert (c == 0x3C3C).all()
    return m[:n].reshape(B, h, w), (c[:n].reshape(B, h, w) if cost else None)


def _device_bm_cost(ctx, torch, pairs, nd, bl):
    B = len(pairs)
    h, w = pairs[0][0].shape
    dl = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    dr = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    dm = torch.zeros(B * h * w, dtype=torch.int16, device="cuda")
    dc = torch.zeros(B * h * w, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.stereo_bm_cost_batch(dl.data_ptr(), dr.data_ptr(), B, w, h, w, w * h, dm.data_ptr(), dc.data_ptr(), nd, bl)
    ctx.sync()
    return dm.cpu().numpy().reshape(B, h, w), dc.cpu().numpy().view(np.uint16).reshape(B, h, w)


SHAPES = [(192, 96, 32, 9), (131, 61, 16, 5), (160, 80, 48, 21), (200, 64, 64, 7)]
EDGES = [(40, 61, 32, 9), (150, 9, 32, 9), (39, 40, 32, 9), (68, 50, 48, 21)]   # one column, one row, empty, one column at (48, 21)
EDGE_IDS = ["one_column", "one_row", "empty", "one_column_48_21"]


@gpu
@pytest.mark.parametrize("w,h,nd,bl", SHAPES + EDGES, ids=[f"{s[0]}x{s[1]}_{s[2]}_{s[3]}" for s in SHAPES] + EDGE_IDS)
def test_zero_penalties_equal_the_cost_form_of_block_matching_on_the_device(ctx, w, h, nd, bl):
    import torch
    pairs = _pairs(w, h, nd)
    maps, costs = _device_sgm(ctx, torch, pairs, nd, bl, 0, 0)
    bm, bc = _device_bm_cost(ctx, torch, pairs, nd, bl)
    print((w, h, nd, bl), "map differs at", int((maps != bm).sum()), "cost differs at", int((costs != bc).sum()), "valid", int((bm != -16).sum()))
    assert np.array_equal(maps, bm) and np.array_equal(costs, bc)
    if w - bl - nd + 2 <= 0:
        assert (maps == SG.FILTERED).all() and (costs == SG.NO_COST).all()
    else:
        assert (bm != SG.FILTERED).sum() >= 3


@gpu
@pytest.mark.parametrize("w,h,nd,bl", SHAPES + EDGES, ids=[f"{s[0]}x{s[1]}_{s[2]}_{s[3]}" for s in SHAPES] + EDGE_IDS)
def test_defaults_equal_the_restatement(ctx, w, h, nd, bl):
    import torch
    p1, p2 = SG.default_params(bl)
    maps, costs = _device_sgm(ctx, torch, _pairs(w, h, nd), nd, bl, p1, p2)
    for v, (m, c) in enumerate(_want(w, h, nd, bl, p1, p2)):
        print((w, h, nd, bl), v, "map differs at", int((maps[v] != m).sum()), "cost differs at", int((costs[v] != c).sum()), "valid", int((m != -16).sum()))
        assert np.array_equal(maps[v], m) and np.array_equal(costs[v], c), v


@gpu
@pytest.mark.parametrize("w,h,nd,bl,p1,p2", [(192, 96, 32, 9, 200, 200), (192, 96, 32, 9, 0, 324), (131, 61, 16, 5, 7, 7), (200, 64, 64, 7, 0, 500),
                                             (160, 80, 48, 21, 0, 32767), (160, 80, 48, 21, 32767, 32767)],
                         ids=["p1_eq_p2", "p1_zero", "p1_eq_p2_16", "p1_zero_64", "p2_max_block21", "both_max_block21"])
def test_parameter_corners_equal_the_restatement(ctx, w, h, nd, bl, p1, p2):
    import torch
    maps, costs = _device_sgm(ctx, torch, _pairs(w, h, nd), nd, bl, p1, p2)
    for v, (m, c) in enumerate(_want(w, h, nd, bl, p1, p2)):
        assert np.array_equal(maps[v], m) and np.array_equal(costs[v], c), (v, int((maps[v] != m).sum()), int((costs[v] != c).sum()))
        assert (m != SG.FILTERED).sum() >= 100


@gpu
def test_strided_input_and_null_cost(ctx):
    """row_stride = W + 5, a padded image_stride, noise in the gaps; cost16 NULL writes no cost."""
    import torch
    w, h, nd, bl = 131, 61, 16, 5
    p1, p2 = SG.default_params(bl)
    maps, costs = _device_sgm(ctx, torch, _pairs(w, h, nd), nd, bl, p1, p2, cost=False, pad=5)
    assert costs is None
    for v, (m, _) in enumerate(_want(w, h, nd, bl, p1, p2)):
        assert np.array_equal(maps[v], m), v
    maps, costs = _device_sgm(ctx, torch, _pairs(w, h, nd)[:1], nd, bl, p1, p2, pad=5)   # batch 1, with the cost
    assert np.array_equal(maps[0], _want(w, h, nd, bl, p1, p2)[0][0]) and np.array_equal(costs[0], _want(w, h, nd, bl, p1, p2)[0][1])


@gpu
@pytest.mark.parametrize("w,h,nd,bl", [(192, 96, 32, 9), (68, 50, 48, 21), (39, 40, 32, 9)], ids=["192x96", "one_column", "empty"])
def test_host_form_leaves_its_input(ctx, w, h, nd, bl):
    L, R = _pairs(w, h, nd)[2]
    p1, p2 = SG.default_params(bl)
    want = _want(w, h, nd, bl, p1, p2)[2]
    l0, r0 = L.copy(), R.copy()
    ctx.profile_select("stereo_sgm")
    m, c = ctx.stereo_sgm(l0, r0, nd, bl, cost=True)
    only = ctx.stereo_sgm(l0, r0, nd, bl, p1, p2)
    launches = ctx.profile_read()[1]
    ctx.profile_select(None)
    assert launches == 2 and np.array_equal(l0, L) and np.array_equal(r0, R)
    assert np.array_equal(m, want[0]) and np.array_equal(c, want[1]) and np.array_equal(only, want[0])


@gpu
def test_bad_arguments_are_refused_without_a_launch(ctx):
    import torch
    from stereo_vo_amd import api
    w, h, nd, bl = 131, 61, 16, 5
    L, R = _pairs(w, h, nd)[0]
    dl, dr = torch.from_numpy(np.stack([L, L])).cuda(), torch.from_numpy(np.stack([R, R])).cuda()
    need = api.sgm_workspace_bytes(w, h, nd, bl, 2)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    dm = torch.full((2 * h * w,), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    Lb, l, r, wp, m = ctx.L, dl.data_ptr(), dr.data_ptr(), ws.data_ptr(), dm.data_ptr()
    P = lambda a, b: C.byref(api.SgmParams(a, b))
    ok = P(50, 200)
    dev = lambda **k: Lb.svo_stereo_sgm_batch_dev(ctx.h, k.get("l", l), k.get("r", r), k.get("batch", 1), k.get("w", w), k.get("h", h),
                                                  k.get("rs", w), k.get("ist", w * h), k.get("nd", nd), k.get("bl", bl), k.get("prm", ok),
                                                  k.get("ws", wp), k.get("wb", need), k.get("m", m), None)
    hd = np.zeros((h, w), np.int16)
    hp = hd.ctypes.data_as(C.c_void_p)
    lp, rp = L.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p)
    hst = lambda **k: Lb.svo_stereo_sgm(ctx.h, k.get("l", lp), k.get("r", rp), k.get("w", w), h, w, k.get("nd", nd), k.get("bl", bl),
                                        k.get("prm", ok), k.get("m", hp), None)
    cases = {
        "null image": lambda: dev(l=None), "null image ": lambda: dev(r=None), "disp16": lambda: dev(m=None),
        "null workspace": lambda: dev(ws=None), "workspace_bytes": lambda: dev(wb=need // 2, batch=2), "workspace_bytes ": lambda: dev(wb=0),
        "params": lambda: dev(prm=None), "p1": lambda: dev(prm=P(-1, 5)), "p2": lambda: dev(prm=P(9, 8)), "p1 ": lambda: dev(prm=P(-3, -2)),
        "SVO_SGM_MAX_P2": lambda: dev(prm=P(5, 32768)), "numDisparities": lambda: dev(nd=24), "numDisparities ": lambda: dev(nd=80),
        "blockSize": lambda: dev(bl=6), "blockSize ": lambda: dev(bl=23), "batch": lambda: dev(batch=0), "batch ": lambda: dev(batch=5),
        "image size": lambda: dev(w=2), "image size ": lambda: dev(h=0), "image size  ": lambda: dev(rs=w - 1),
        "image_stride": lambda: dev(batch=2, ist=w * h - 1),
        "null image  ": lambda: hst(l=None), "disp16 ": lambda: hst(m=None), "params ": lambda: hst(prm=None), "p2 ": lambda: hst(prm=P(2, 1)),
        "SVO_SGM_MAX_P2 ": lambda: hst(prm=P(0, 40000)), "numDisparities  ": lambda: hst(nd=17), "blockSize  ": lambda: hst(bl=4),
        "image size   ": lambda: hst(w=1),
    }
    ctx.profile_select("stereo_sgm")
    for word, call in cases.items():
        assert call() == -1, word
        assert word.strip() in Lb.svo_last_error(ctx.h).decode(), (word, Lb.svo_last_error(ctx.h))
    launches = ctx.profile_read()[1]
    ctx.profile_select(None)
    assert launches == 0
    assert (dm.cpu().numpy().view(np.uint16) == 0x5A5A).all() and (ws.cpu().numpy() == 0xA5).all() and (hd == 0).all()
    # the context works afterwards
    p1, p2 = SG.default_params(bl)
    assert np.array_equal(ctx.stereo_sgm(L, R, nd, bl), _want(w, h, nd, bl, p1, p2)[0][0])


@gpu
def test_chain_sgm_cost_then_left_right_check_then_speckle(ctx):
    """The device's own (map, cost) through svo_disparity_lr_check_batch_dev and the speckle filter equals the restatements composed."""
    import torch
    from stereo_vo_amd import api
    w, h, nd, bl = 192, 96, 32, 9
    p1, p2 = SG.default_params(bl)
    pairs = _pairs(w, h, nd)[:2] + [LR.occlusion_pair()]
    maps, costs = _device_sgm(ctx, torch, pairs, nd, bl, p1, p2)
    B = len(pairs)
    dm = torch.from_numpy(maps.reshape(-1).copy()).cuda()
    dc = torch.from_numpy(costs.view(np.int16).reshape(-1).copy()).cuda()
    dn = torch.zeros(B, dtype=torch.int32, device="cuda")
    sw = api.speckle_workspace_bytes(w, h, B)
    ws = torch.zeros(sw, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.lr_check_dev(dm.data_ptr(), dc.data_ptr(), B, w, h, api.LrCheckParams(16), dn.data_ptr())
    ctx.sync()
    checked, removed = dm.cpu().numpy().reshape(B, h, w).copy(), dn.cpu().numpy().copy()
    ctx.speckle_filter_dev(dm.data_ptr(), B, w, h, api.SpeckleParams(100, 32), ws.data_ptr(), sw, None)
    ctx.sync()
    final = dm.cpu().numpy().reshape(B, h, w)
    total = speck = 0
    for v, (L, R) in enumerate(pairs):
        m, c = SG.sgm(L, R, nd, bl, p1, p2)
        assert np.array_equal(maps[v], m) and np.array_equal(costs[v], c), v
        want, n = LR.check_arrays(m, c, 16)
        assert np.array_equal(checked[v], want) and removed[v] == n, (v, n, int(removed[v]))
        sp = SP.filter_propagate(want, 100, 32)[0]
        assert np.array_equal(final[v], sp), v
        print("pair", v, "valid", int((m != -16).sum()), "removed by the check", n, "by the speckle filter", int((sp != want).sum()))
        total += n
        speck += int((sp != want).sum())
    assert total >= 100 and speck >= 100
