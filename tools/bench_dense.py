#!/usr/bin/env python3
"""What dense keyframe depth costs on the MI355X (a tool: bench.py is untouched and measures no clouds).

One process, one GPU, HIP events (svo_profile_select) around the launches:
  1. dense map: the fused batched launch (stereo_dense_batch_kernel, raw images in, 16 pairs per launch) per pair, beside
     the three-launch sequence inside svo_stereo_bm (two prefilter launches + stereo_dense_kernel, one pair per call) timed
     in the same run, both at 1241 x 376, StereoBM(48, 21);
  2. cloud: the count + scan + write launches per pair at steps 1 and 4, with the bytes they move and
     svo_measure_peak("hbm_copy") of the same run;
  3. speckle filter: the four launches of svo_disparity_speckle_filter_batch_dev per pair on the fused launch's own maps,
     max_size 100 and 400, max_diff16 32, beside the fused launch and the copy rate of the same run;
  4. left-right check: the cost form of the fused launch (svo_stereo_bm_cost_batch_dev, which also writes the winner's SAD) per
     pair beside the plain form, and the one launch of svo_disparity_lr_check_batch_dev per pair on that map and cost,
     max_diff16 16, beside the copy rate of the same run;
  5. semi-global matching: the launch sequence of svo_stereo_sgm_batch_dev (fill, cost volume, four paths; defaults, with the cost
     form) per pair beside the plain fused launch in alternating blocks, its bytes counted from the code against the
     copy rate of the same run;
  6. cost to the VO: bench.py's headline load (96 lanes in 3 pipeline groups of 16-frame steps) without keyframe clouds, with
     clouds at step 4, with clouds and the speckle filter, with clouds and the left-right check, and with clouds from semi-global
     matching, alternating, as frames/s, their ratios and the spread over the rounds;
  7. voxel map: one svo_voxel_map_insert_dev per cloud ("voxel_insert" bracket) for the 16 clouds of the batch at steps 1 and 4
     into a map of the default capacity, voxel sizes 0.05 and 0.2 m in three alternating blocks, into the cleared map and again
     into the filled one, beside the time hbm_copy needs for the records' 16 bytes per point and the run heads per point from
     tests/voxel_ref.py; the extraction of the resulting table ("voxel_extract") beside its 40 bytes per slot; and the 96-lane
     load with clouds at step 4 with and without inserting every keyframe's cloud into a map per lane after each call;
  8. carving and the copy of the live voxels: one svo_voxel_map_copy_live_dev of each filled map of section 7 into a cleared map of
     the same capacity ("voxel_copy") and one svo_voxel_map_carve_dev of it with the batch's last disparity map under its pose
     ("voxel_carve": first with keep_count 1, which walks, projects and reads the windows but protects every voxel, then the real
     one), each beside the time hbm_copy needs for 8 bytes per slot + 32 per live slot (+ 40 per copied voxel); and the 96-lane
     load with every keyframe inserted against every keyframe's map carving its lane's map before its cloud is inserted;
  9. render: one svo_voxel_map_render_dev of each filled map of section 7 (before section 8 carves it) at 1241 x 376 under the last
     cloud's pose ("voxel_render" bracket: two memsets and both launches, mean of 5), at the defaults and with max_radius 0, with the
     four counts, n_splat as the number of atomic requests, and the time hbm_copy needs for 8 bytes per slot + 32 per qualifying
     slot + 11 per pixel (memset, resolve read, two writes); and the default render again in the splat launch's other three drawing
     modes (svo_voxel_render_set_mode).  No 96-lane figure: a render is per published view, not per keyframe.
 10. removal and move: on each filled map of section 7 (before sections 8 and 9), one svo_voxel_map_remove_dev of the last inserted
     cloud ("voxel_remove") and one svo_voxel_map_move_dev of it to a pose 1 cm and 0.1 degrees away ("voxel_move"), mean of 5 each,
     beside one more svo_voxel_map_insert_dev of the same cloud in the same run and the time hbm_copy needs for its 16 bytes per
     record; and the 96-lane load with clouds at step 4 with every lane's ledger holding four keyframes and moving all of them after
     each call, beside clouds alone (--ledger-only runs just these two).
 11. grid: one svo_voxel_map_grid_dev of each filled map of section 7 (before section 8 carves it) at the defaults for its voxel size
     (0.5 m cells, 256 x 256 of them, the band -3 .. 2.5), the origin shifted so that the last cloud's pose is at the start of the a
     axis and the middle of the b axis ("voxel_grid" bracket: two memsets and both launches, mean of 5), with the five counts, the
     binned voxels per occupied cell, and the time hbm_copy needs for 16 bytes per slot + 8 per qualifying slot + 64 per cell + the
     26 per cell of the outputs, and the same grid in both modes of the walk (svo_voxel_grid_set_mode); its yardsticks are the carve with every voxel protected and the render of the same run and map.
 12. clearance: one svo_grid_clearance_dev (all four outputs and the counts; "grid_clearance" bracket: the counts' memset and both
     launches, mean of 5) of section 11's grid of each filled map at the defaults (OBSTACLE cells are the sources, max_dist 64) and
     with UNKNOWN cells as sources too, and of a synthetic 2048 x 2048 grid at source densities 0 (every cell searches its whole
     window), 0.001 and 0.1 with max_dist 64 and at 0.001 with max_dist 512; each beside the time hbm_copy needs for 22 bytes per
     cell (cls read, the offsets written and read, 13 bytes of outputs) and, for the 256 x 256 grids, the loop steps of both passes
     summed over the cells, counted on the host from cls.
 13. route: one svo_grid_route_dev ("grid_route" bracket: its memsets and every launch, mean of 5; cost, next, four paths of up to 4096
     cells and the counts) over the clearance (inflate_radius two cells) of section 11's grid of each filled map, near_r2 64,
     near_weight 4, the goal at the grid's centre cell, the starts at its four corners, at the default 64 rounds (raised fourfold
     until the call converges); and of a synthetic 2048 x 2048 grid at blocked densities 0, 0.1 and 0.3 (goal and starts kept passable) without dist2.  Per case the
     time, rounds_run, the counts and the longest path; the cost of an enqueued round that finds nothing to do (the same case at
     max_rounds = rounds_run and at 64 more, the difference per launch); the path launch alone (the call with the starts minus the
     call without, per step of the longest path); and, as context, the device-to-host copies of blocked and dist2 plus this tool's
     host Dijkstra in Python (256 x 256 only): the detour the entry replaces.
 14. frontiers: one svo_grid_frontiers_dev ("grid_frontier" bracket: the counts' memset and every launch, mean of 5; records, goal_cells,
     label and the counts at the defaults: min_size 3, max_frontiers 1024) of section 11's grid of each filled map off section 12's
     clearance at an inflation of two cells, with the cost of a route from the grid's centre cell; of seeded 2048 x 2048 grids at
     (unknown, obstacle) densities (0.05, 0.05), (0.3, 0.1) and (0.6, 0.2); and of a 2048 x 2048 serpentine, one frontier of about two
     million cells.  Per case the time, the counts, the time without the combining of runs along a wavefront
     (svo_grid_frontier_set_mode; the same bytes), the time hbm_copy needs for cls, blocked and 8 bytes of labels per cell and, as
     context, the device-to-host copies of the inputs plus the restatement's numpy route on the host (256 x 256 only).
 15. view: one svo_grid_view_dev ("grid_view" bracket: two memsets and both launches, mean of 5; records, order, best, seen and the
     counts at the defaults) over section 14's goal_cells (all 1024 entries) and cost field of section 11's grid of each filled map,
     and over a seeded 2048 x 2048 grid with 1024 and 4096 views at max_range 64 and 255.  Per case the time staged in LDS and the
     time with every step reading cls (svo_grid_view_set_mode; the same bytes), the counts, the steps walked per target in range
     from the restatement's counter (the synthetic cases: over the first 8 views), the time hbm_copy needs for the windows once per
     used view, the records and seen and, as context, the device-to-host copies of the inputs plus the restatement's numpy route on
     the host (256 x 256 only): the detour the entry replaces.
 16. surface: one svo_grid_surface_dev ("grid_surface" bracket: the counts' memset and the launch, mean of 5; cls_out, step, relief,
     support and the counts) of section 11's grid of each filled map at the defaults (r2 = 2), and of seeded 2048 x 2048 and
     8192 x 2048 grids at r2 = 0, 2, 25 and 225 (max_step 0.3, max_relief 0.6, min_support_256 200).  Per case the time, the counts,
     the time hbm_copy needs for 5 bytes read and 11 written per cell, the time per cell and footprint cell and, as context, the
     device-to-host copies of cls and top plus the restatement's numpy route on the host (the ground plans, and 2048 x 2048 up to
     r2 = 25): the detour the entry replaces.  --surface-only runs just the seeded grids (a library built with another tile shape,
     -DSVO_EXP_SURFACE_TILE_A / _B, is measured with it).
 17. waypoints: one svo_grid_waypoints_dev ("grid_waypoints" bracket: the counts' memset and the launch, mean of 5; all five outputs
     and the counts) over the paths of a route to the centre cell: on section 12's clearance (inflation two cells) of section 11's
     grid of each filled map from one start, the corner with the longest path, and on a seeded 2048 x 2048 grid (blocked density
     0.1) from one start (a corner) and from 4,096 seeded starts; max_look 16, 64 and 255.  Per case the counts and, as context for one path up to max_look 64, the device-to-host copies of path, path_len and blocked plus the
     restatement's Python walk on the host: the detour the entry replaces.  --waypoints-only runs just the seeded grid.
 18. align: on each filled map of section 7 (before sections 8 and 9), one svo_voxel_map_align_sums_dev of the batch's last cloud
     under its own pose ("voxel_align" bracket: the sums' memset and the launch, mean of 5 after the warm-up) at reach 0 and 1, with
     the four counts, beside section 10's insert of the same cloud in the same run (one probe per record against 27 look-ups); and
     svo_voxel_map_align of that cloud from its pose displaced by half a voxel and 0.01 rad at the defaults: wall clock (mean of 5),
     the iterations taken, the status, and the share of the wall clock that is not inside the "voxel_align" brackets of one more run
 19. normals and the plane form of the align: on the same maps and clouds, in the same run as section 18, one
     svo_voxel_map_normals_dev at the defaults ("voxel_normals" bracket: the counts' memset and the launch, mean of 5 after the warm-up)
     beside the map's load factor and live voxel count; svo_voxel_map_align_plane_sums_dev at reach 0 and 1 ("voxel_align_plane"
     bracket) with its five counts, beside section 18's point sums and section 10's insert of the same cloud; and
     svo_voxel_map_align_plane from section 18's displaced pose: wall clock (mean of 5), iterations, status, beside section 18's
     svo_voxel_map_align.  --align-only runs section 7's fill and sections 10, 18 and 19 alone.
 20. locate: on the same maps and clouds, in the same run as sections 7, 18 and 19, one svo_voxel_map_occupancy_dev at the default
     dims around the last cloud's pose ("voxel_occupancy" bracket, mean of 5) beside section 7's extraction walk of the same table;
     one svo_voxel_map_locate_scores_dev of the last inserted cloud over the nine default candidates at box (8, 4, 8) and at
     (16, 4, 16) ("voxel_locate" bracket, mean of 5), as us and as occupancy tests per second (n * K * |box| per call), beside
     section 18's reach-1 sums of the same cloud as look-ups per second (27 n per call); and svo_voxel_map_locate (point and plane
     form) from the cloud's pose moved by (5.3, -1.7, 4.2) voxels and turned by 0.11 rad about the world's y: wall clock (mean of 5),
     status, chosen candidate and the shift left.  A library built with -DSVO_EXP_LOCATE_BASELINE (SVO_EXTRA_HIPFLAGS) runs the same
     section with the baseline form of the score kernel.  --align-only runs this section too.
 21. sight lines: on the same maps, in the same run as section 20 and from the same volume (the default dims around the last cloud's
     pose), one svo_voxel_occupancy_coarse_dev ("voxel_coarse" bracket: the memset and the launch, mean of 5); the camera form at
     the image size from the map's own pose and 262,144 random rays (range 30 m, directions normal) from the volume's centre
     ("voxel_rays" bracket: the counts' memset and the launch, mean of 5), each with the plain and with the block-skipping walk,
     whose outputs are compared byte for byte; steps per ray from the counts, and the share of the visited cells the skipping
     walk jumps from the restatement over the first 4,096 of the random rays (the two walks' counts are equal by contract, so
     they cannot say); beside them, for context only, the same run's splat render at the defaults and section 20's occupancy.
     --align-only runs this section too.
 22. distance field: on the same maps, in the same run as sections 20 and 21 and over the same volume, svo_voxel_occupancy_distance_dev
     ("voxel_distance" bracket: the counts' memset and the three launches, mean of 5) at max_dist 8, 32 and 128 with dist2 alone and
     with all four outputs (inflate_radius 3 voxels), and svo_voxel_distance_query_dev of 262,144 random spheres in and around the
     volume ("voxel_distance_query" bracket, mean of 5).  Beside each: section 20's occupancy launch, the time hbm_copy needs for the
     bytes the workspace layout moves per cell (8.125 for dist2 alone, 22.25 for all four outputs) and the steps per cell, counted
     on the host by the search's stop rule: the words each wavefront reads from the volume's words (axis 0), and the outward steps
     from the downloaded partial and final squares (axes 1 and 2).  --align-only runs this section too.
 23. route through the volume: on the same maps and over the same volume, svo_voxel_occupancy_route_dev ("voxel_route" bracket: its
     memsets and every launch, mean of 5) over the distance field's `inflated` at inflate_radius 0 (the occupancy itself) and 0.3 m
     (max_dist 8), without dist2 and with it (near_r2 16, near_weight 4), the goal at the free cell nearest the volume's centre: the
     rounds a call of 1,024 needs (rounds_run), cost alone at rounds_run + 1 and the time per round, the same with 64 more rounds
     (what an enqueued round with no active tile costs), at the default max_rounds, and with next and 64 paths from random free cells;
     beside each the time hbm_copy (measured in the same run) needs for one pass over the arrays (12.125 B per cell for cost alone,
     + 2 with dist2; 18.25 with next, + 4 with dist2).  The tile shape is the library's: a library built with
     -DSVO_EXP_VOXEL_ROUTE_CUBE (SVO_EXTRA_HIPFLAGS) runs the same section with 8 x 8 x 8 tiles.  --align-only runs this section too;
     --route-only runs section 7's fill and this section alone.
Prints one JSON line; --out also writes the text report.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # voxel_ref: the restatement counts the run heads

import bench  # noqa: E402  (its module level sets the hardware-queue count bench.py measures with, before HIP starts)
import numpy as np  # noqa: E402

W, H = bench.W, bench.H
NDISP, BLOCK = 48, 21
SPECKLE_SIZES, SPECKLE_DIFF = (100, 400), 32
LR_DIFF = 16
VOXEL_SIZES = (0.05, 0.2)
VOXEL_LANE_LOG2 = 20  # the 96 per-lane maps of the group load: 42 MB each


def standalone(S, torch, batch, warmup, reps):
    from stereo_vo_amd import api
    ctx = S.Context(W, H, max_batch=batch, max_corners=64, max_candidates=1 << 12, max_features=64)
    p = S.synth_default(W, H)
    cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
    pairs = [S.synth_render(p, i) for i in range(batch)]
    dl = torch.from_numpy(np.stack([x[0] for x in pairs])).cuda()
    dr = torch.from_numpy(np.stack([x[1] for x in pairs])).cuda()
    dm = torch.empty((batch, H, W), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    copy = ctx.measure_peak("hbm_copy")
    out = {"batch": batch, "hbm_copy_bytes_per_s": copy}

    def fused():
        ctx.stereo_bm_batch(dl.data_ptr(), dr.data_ptr(), batch, W, H, W, W * H, dm.data_ptr(), NDISP, BLOCK)

    def timed(tag, fn, n):
        for _ in range(warmup):
            fn()
        ctx.profile_select(tag)
        for _ in range(n):
            fn()
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        return ms, k

    ms, k = timed("stereo_dense_batch", fused, reps)
    out["fused_ms_per_pair"] = ms / k / batch
    out["fused_launches_timed"] = k
    # the baseline: svo_stereo_bm's own three launches, one pair per call (its host copies are outside the bracket)
    ms, k = timed("stereo_bm", lambda: [ctx.stereo_bm(x[0], x[1], NDISP, BLOCK) for x in pairs], max(reps // 4, 2))
    out["three_launch_ms_per_pair"] = ms / k
    out["three_launch_calls_timed"] = k
    same = all(np.array_equal(dm[i].cpu().numpy(), ctx.stereo_bm(pairs[i][0], pairs[i][1], NDISP, BLOCK)) for i in (0, batch - 1))
    out["fused_equals_three_launch"] = bool(same)
    # clouds of those maps
    out["cloud"] = []
    for step in (1, 4):
        mp = ((W + step - 1) // step) * ((H + step - 1) // step)
        pts = torch.empty((batch, mp, 4), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((batch, 2), dtype=torch.int32, device="cuda")
        prm = api.CloudParams(step, 0.0, mp)
        ms, k = timed("cloud", lambda: ctx.disparity_cloud(dm.data_ptr(), dl.data_ptr(), batch, W, H, W, W * H, cam, None, prm, pts.data_ptr(),
                                                          cnt.data_ptr()), reps)
        kept = float(cnt.cpu().numpy()[:, 0].mean())
        # per pair: the map's sampled values read twice (count + write: 2 B each, a whole 64-B sector per sample once step > 1 is
        # NOT counted), the left pixel of every kept point, 16 B written per point
        nbytes = 2 * 2 * mp + kept * (1 + 16)
        per = ms / k / batch * 1e-3
        out["cloud"].append({"step": step, "ms_per_pair": 1e3 * per, "kept_per_pair": kept, "algorithmic_bytes_per_pair": nbytes,
                             "bytes_per_s": nbytes / per, "share_of_copy_rate": nbytes / per / copy, "sequences_timed": k})
    # speckle filter of those maps (in place: every call gets a fresh copy, made outside the timed bracket)
    out["speckle"] = []
    work = torch.empty_like(dm)
    need = api.speckle_workspace_bytes(W, H, batch)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    nrem = torch.zeros(batch, dtype=torch.int32, device="cuda")
    for max_size in SPECKLE_SIZES:
        sp = api.SpeckleParams(max_size, SPECKLE_DIFF)

        def filt():  # the copy runs on torch's stream, the filter on the context's: neither may overlap the other's use of `work`
            work.copy_(dm)
            torch.cuda.synchronize()
            ctx.speckle_filter_dev(work.data_ptr(), batch, W, H, sp, ws.data_ptr(), need, nrem.data_ptr())
            ctx.sync()

        ms, k = timed("speckle", filt, reps)
        removed = float(nrem.cpu().numpy().mean())
        nbytes = 19 * W * H  # map read, labels and counts written once and read once, the seams
        per = ms / k / batch * 1e-3
        out["speckle"].append({"max_size": max_size, "max_diff16": SPECKLE_DIFF, "ms_per_pair": 1e3 * per, "removed_per_pair": removed,
                               "valid_per_pair": float((dm != -16).sum().item()) / batch, "budget_bytes_per_pair": nbytes,
                               "bytes_per_s": nbytes / per, "share_of_copy_rate": nbytes / per / copy,
                               "ratio_to_fused_dense": 1e3 * per / out["fused_ms_per_pair"], "sequences_timed": k})
    # left-right check: the cost form of the fused launch beside the plain form (alternating blocks, the same bracket), then the
    # check on that map and cost (in place: every call gets a fresh copy of the map, made outside the timed bracket)
    dc = torch.empty((batch, H, W), dtype=torch.int16, device="cuda")  # uint16 costs
    dm2 = torch.empty_like(dm)

    def fused_cost():
        ctx.stereo_bm_cost_batch(dl.data_ptr(), dr.data_ptr(), batch, W, H, W, W * H, dm2.data_ptr(), dc.data_ptr(), NDISP, BLOCK)

    plain_ms, cost_ms = [], []
    for _ in range(3):
        ms, k = timed("stereo_dense_batch", fused, reps)
        plain_ms.append(ms / k / batch)
        ms, k = timed("stereo_dense_batch", fused_cost, reps)
        cost_ms.append(ms / k / batch)
    ctx.sync()
    lr = {"max_diff16": LR_DIFF, "plain_ms_per_pair": float(np.median(plain_ms)), "cost_ms_per_pair": float(np.median(cost_ms)),
          "all_plain_ms": plain_ms, "all_cost_ms": cost_ms, "launches_per_block": reps,
          "cost_map_equals_plain_map": bool(torch.equal(dm, dm2))}
    lr["ratio_cost_to_plain"] = lr["cost_ms_per_pair"] / lr["plain_ms_per_pair"]
    prm = api.LrCheckParams(LR_DIFF)

    def check():
        work.copy_(dm2)
        torch.cuda.synchronize()
        ctx.lr_check_dev(work.data_ptr(), dc.data_ptr(), batch, W, H, prm, nrem.data_ptr())
        ctx.sync()

    ms, k = timed("lr_check", check, reps)
    per = ms / k / batch * 1e-3
    nbytes = 4 * W * H  # map and cost read once, 2 B each; the few FILTERED stores are not counted
    lr.update({"check_ms_per_pair": 1e3 * per, "removed_per_pair": float(nrem.cpu().numpy().mean()),
               "valid_per_pair": float((dm2 != -16).sum().item()) / batch, "budget_bytes_per_pair": nbytes, "bytes_per_s": nbytes / per,
               "share_of_copy_rate": nbytes / per / copy, "ratio_to_fused_dense": 1e3 * per / lr["plain_ms_per_pair"], "calls_timed": k})
    out["lr_check"] = lr
    # semi-global matching: the whole sequence as one bracket, alternating with the plain fused launch
    sp = api.sgm_default_params(BLOCK)
    need = api.sgm_workspace_bytes(W, H, NDISP, BLOCK, batch)
    del ws
    sws = torch.empty(need, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def sgm():
        ctx.stereo_sgm_batch(dl.data_ptr(), dr.data_ptr(), batch, W, H, W, W * H, sp, sws.data_ptr(), need, dm2.data_ptr(), dc.data_ptr(), NDISP, BLOCK)

    plain_ms, sgm_ms = [], []
    for _ in range(3):
        ms, k = timed("stereo_dense_batch", fused, reps)
        plain_ms.append(ms / k / batch)
        ms, k = timed("stereo_sgm", sgm, reps)
        sgm_ms.append(ms / k / batch)
    ctx.sync()
    rect = (W - BLOCK - NDISP + 2) * (H - BLOCK + 1)
    # the volume written once (2 B) and read by each path (4 x 2 B), the sums written by three paths and read by three
    # (6 x 4 B) per (pixel, disparity); the texture sum written and read; both images read; map and cost filled and written
    nbytes = 34 * rect * NDISP + 4 * rect + 2 * W * H + 4 * W * H + 4 * rect
    per = float(np.median(sgm_ms)) * 1e-3
    out["sgm"] = {"p1": sp.p1, "p2": sp.p2, "plain_ms_per_pair": float(np.median(plain_ms)), "sgm_ms_per_pair": 1e3 * per,
                  "all_plain_ms": plain_ms, "all_sgm_ms": sgm_ms, "sequences_per_block": reps, "ratio_to_fused_dense": 1e3 * per / float(np.median(plain_ms)),
                  "workspace_bytes_per_pair": need / batch, "bytes_per_pair": nbytes, "bound_ms_per_pair": 1e3 * nbytes / copy,
                  "bytes_per_s": nbytes / per, "share_of_copy_rate": nbytes / per / copy,
                  "valid_per_pair_sgm": float((dm2 != -16).sum().item()) / batch, "valid_per_pair_bm": float((dm != -16).sum().item()) / batch}
    out["voxel"] = voxel(S, torch, ctx, cam, dm, dl, batch, warmup, copy)
    out["clearance_synthetic"] = [clearance_case(S, torch, ctx, clearance_random(torch, 2048, 2048, density), 4, md, 0.5, warmup, copy, density=density)
                                  for density, md in ((0.0, 64), (0.001, 64), (0.1, 64), (0.001, 512))]
    out["route_synthetic"] = [route_case(S, torch, ctx, route_random(torch, 2048, 2048, density), None, 0, 0, warmup, copy, density=density)
                              for density in (0.0, 0.1, 0.3)]
    out["frontier_synthetic"] = [frontier_case(S, torch, ctx, *frontier_random(torch, 2048, 2048, pu, po), warmup, copy, densities=[pu, po])
                                 for pu, po in ((0.05, 0.05), (0.3, 0.1), (0.6, 0.2))]
    out["frontier_synthetic"].append(frontier_case(S, torch, ctx, *frontier_serpentine(torch, 2048), warmup, copy, densities="serpentine"))
    out["view_synthetic"] = view_synthetic(S, torch, ctx, warmup, copy)
    out["surface_synthetic"] = surface_synthetic(S, torch, ctx, warmup, copy)
    out["waypoint_synthetic"] = waypoint_synthetic(S, torch, ctx, warmup)
    ctx.close()
    return out


def voxel(S, torch, ctx, cam, dm, dl, batch, warmup, copy, only_align=False, only_route=False):
    """Section 7: the batch's clouds into one map.  Cloud i goes in under a small rotation and 0.8 m of forward motion per frame
    (the synthetic stream's step), so consecutive clouds see almost the same surfaces, as consecutive keyframes do."""
    import voxel_ref as V
    from stereo_vo_amd import api
    out = []
    m12 = [V.rot_y(0.004 * i, (0.0, 0.0, 0.8 * i)) for i in range(batch)]
    for step in (1, 4):
        mp = ((W + step - 1) // step) * ((H + step - 1) // step)
        pts = torch.empty((batch, mp, 4), dtype=torch.int32, device="cuda")
        cnt = torch.zeros((batch, 2), dtype=torch.int32, device="cuda")
        ctx.disparity_cloud(dm.data_ptr(), dl.data_ptr(), batch, W, H, W, W * H, cam, None, api.CloudParams(step, 0.0, mp), pts.data_ptr(), cnt.data_ptr())
        ctx.sync()
        n = [int(v) for v in cnt.cpu().numpy()[:, 1]]
        host0 = pts[0, :n[0]].cpu().numpy().view(np.uint32).copy().view(V.POINT).reshape(-1)
        rows = {vs: {"fresh": [], "again": []} for vs in VOXEL_SIZES}
        maps = {vs: S.VoxelMap(ctx, voxel_size=vs) for vs in VOXEL_SIZES}
        stats = {}

        def insert_all(vm):
            for i in range(batch):
                vm.insert(pts[i].data_ptr(), n[i], m12=m12[i])

        for _ in range(3):  # alternating blocks
            for vs in VOXEL_SIZES:
                vm = maps[vs]
                for _ in range(warmup):
                    vm.clear()
                    insert_all(vm)
                vm.clear()
                ctx.profile_select("voxel_insert")
                insert_all(vm)
                ms, k = ctx.profile_read()
                rows[vs]["fresh"].append(ms / k)
                stats[vs] = vm.stats()
                ctx.profile_select("voxel_insert")
                insert_all(vm)
                ms, k = ctx.profile_read()
                rows[vs]["again"].append(ms / k)
                ctx.profile_select("")
        mean_n = float(np.mean(n))
        for vs in VOXEL_SIZES:
            vm = maps[vs]
            buf = torch.empty((min(vm.capacity, 2 * stats[vs]["n_voxels"] + 1), 4), dtype=torch.int32, device="cuda")
            c2 = torch.zeros(2, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            for _ in range(warmup):
                vm.extract_dev(1, buf.data_ptr(), buf.shape[0], c2.data_ptr())
            ctx.profile_select("voxel_extract")
            for _ in range(5):
                vm.extract_dev(1, buf.data_ptr(), buf.shape[0], c2.data_ptr())
            ms, k = ctx.profile_read()
            ctx.profile_select("")
            fresh, again = float(np.median(rows[vs]["fresh"])), float(np.median(rows[vs]["again"]))
            bound = 1e3 * 16 * mean_n / copy
            out.append({"cloud_step": step, "voxel_size": vs, "capacity_log2": vm.params.capacity_log2, "points_per_cloud": mean_n,
                        "fresh_ms_per_cloud": fresh, "again_ms_per_cloud": again, "all_fresh_ms": rows[vs]["fresh"], "all_again_ms": rows[vs]["again"],
                        "record_bytes_bound_ms": bound, "fresh_share_of_bound": bound / fresh, "again_share_of_bound": bound / again,
                        "run_heads_per_point_cloud0": V.run_heads(host0, m12[0], vs) / max(n[0], 1),
                        "stats_after_fresh": stats[vs], "load": stats[vs]["n_voxels"] / vm.capacity,
                        "extract_ms": ms / k, "extract_n_total": int(c2.cpu()[0]), "table_bytes_bound_ms": 1e3 * 40 * vm.capacity / copy,
                        "extract_share_of_bound": (1e3 * 40 * vm.capacity / copy) / (ms / k)})
            if only_route:
                out[-1].update(voxel_route_view(torch, ctx, vm, 0.004 * (batch - 1), 0.8 * (batch - 1), warmup, copy))
                vm.close()
                continue
            out[-1].update(remove_and_move(torch, ctx, vm, pts[batch - 1], n[batch - 1], 0.004 * (batch - 1), 0.8 * (batch - 1), warmup, copy))
            out[-1].update(align_view(torch, ctx, vm, pts[batch - 1], n[batch - 1], 0.004 * (batch - 1), 0.8 * (batch - 1), warmup))
            out[-1].update(normals_view(torch, ctx, vm, pts[batch - 1], n[batch - 1], 0.004 * (batch - 1), 0.8 * (batch - 1), warmup, out[-1]["align"]))
            out[-1].update(locate_view(torch, ctx, vm, pts[batch - 1], n[batch - 1], 0.004 * (batch - 1), 0.8 * (batch - 1), warmup, out[-1]["align"], out[-1]["extract_ms"]))
            out[-1].update(rays_view(torch, ctx, cam, vm, 0.004 * (batch - 1), 0.8 * (batch - 1), warmup, out[-1]["locate"]))
            out[-1].update(distance_view(torch, ctx, vm, 0.004 * (batch - 1), 0.8 * (batch - 1), warmup, out[-1]["locate"], copy))
            out[-1].update(voxel_route_view(torch, ctx, vm, 0.004 * (batch - 1), 0.8 * (batch - 1), warmup, copy))
            if only_align:
                vm.close()
                continue
            out[-1].update(grid_view(S, torch, ctx, vm, np.asarray(m12[batch - 1]), warmup, copy))  # before the carve changes the map, as the render
            out[-1].update(clearance_view(S, torch, ctx, vm, np.asarray(m12[batch - 1]), warmup, copy))  # of the same grid, before the carve too
            out[-1].update(route_view(S, torch, ctx, vm, np.asarray(m12[batch - 1]), warmup, copy))  # over that grid's clearance
            out[-1].update(frontier_view(S, torch, ctx, vm, np.asarray(m12[batch - 1]), warmup, copy))  # of that grid, off that clearance
            out[-1].update(surface_view(S, torch, ctx, vm, np.asarray(m12[batch - 1]), warmup, copy))  # of that grid's cls and top
            out[-1].update(waypoint_view(S, torch, ctx, vm, np.asarray(m12[batch - 1]), warmup, copy))  # of a route over that grid's clearance
            out[-1].update(render_view(S, torch, ctx, cam, vm, np.asarray(m12[batch - 1]), warmup, copy))
            out[-1].update(carve_and_copy(S, torch, ctx, cam, dm, vm, np.asarray(m12[batch - 1]), warmup, copy))
            vm.close()
            print(f"bench_dense: voxel map at cloud step {step}, voxel {vs} m done", file=sys.stderr, flush=True)
    return out


def remove_and_move(torch, ctx, vm, cloud, n, angle, forward, warmup, copy):
    """Section 10 for one filled map: the last inserted cloud taken out ("voxel_remove"), moved to a pose 1 cm and 0.1 degrees away
    ("voxel_move": the removal and the insert) and, as the yardstick of the same run, inserted once more ("voxel_insert"); mean of 5
    each.  Every timed call is undone by its untimed inverse, so the map is afterwards what it was."""
    import voxel_ref as V
    here, there = V.rot_y(angle, (0.0, 0.0, forward)), V.rot_y(angle + np.deg2rad(0.1), (0.01, 0.0, forward))
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p, c = cloud.data_ptr(), cnt.data_ptr()
    calls = {"remove": (lambda: vm.remove(p, n, m12=here, counts_ptr=c), lambda: vm.insert(p, n, m12=here), "voxel_remove"),
             "move": (lambda: vm.move(p, n, from_m12=here, to_m12=there, counts_ptr=c), lambda: vm.move(p, n, from_m12=there, to_m12=here), "voxel_move"),
             "insert": (lambda: vm.insert(p, n, m12=here), lambda: vm.remove(p, n, m12=here), "voxel_insert")}
    out, before = {}, vm.stats()
    for name, (do, undo, bracket) in calls.items():
        for _ in range(warmup):
            do()
            undo()
        total = 0.0
        for _ in range(5):
            ctx.profile_select(bracket)
            do()
            ms, k = ctx.profile_read()
            assert k == 1, (bracket, k)
            total += ms
            ctx.profile_select("")
            if name != "insert":
                counts = [int(v) for v in cnt.cpu()]
            undo()
        out[name + "_ms"] = total / 5
        if name != "insert":
            out[name + "_counts"] = counts
            assert counts[2] == 0 and counts[3] == 0, (name, counts)  # nothing missing, nothing short: the exact inverse
    after = vm.stats()
    assert after["n_dropped"] == before["n_dropped"], (before, after)
    out["remove_move_bound_ms"] = 1e3 * 16 * n / copy
    out["remove_move_points"] = n
    return out


def align_view(torch, ctx, vm, cloud, n, angle, forward, warmup):
    """Section 18 for one filled map: the sums of the last inserted cloud under its own pose at reach 0 and 1, and the loop from the
    pose displaced by half a voxel and 0.01 rad.  Nothing in the map changes."""
    import voxel_ref as V
    here = V.rot_y(angle, (0.0, 0.0, forward))
    vs = float(vm.params.voxel_size)
    sums = torch.zeros(32, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p, out = cloud.data_ptr(), {"points": n}
    for reach in (0, 1):
        for _ in range(warmup):
            vm.align_sums(p, n, c2w12=here, sums_ptr=sums.data_ptr(), reach=reach)
        ctx.profile_select("voxel_align")
        for _ in range(5):
            vm.align_sums(p, n, c2w12=here, sums_ptr=sums.data_ptr(), reach=reach)
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        assert k == 5, k
        out[f"sums_reach{reach}_ms"] = ms / k
        out[f"sums_reach{reach}_counts"] = [int(v) for v in sums.cpu()[17:21]]
    # the cloud's pose7 (X_cam = R(q) X_world + t) from its camera->world rot_y(angle), shift (0, 0, forward), then displaced
    c, sn = np.cos(angle / 2), np.sin(angle / 2)
    R = np.asarray(here).reshape(3, 4)[:, :3]
    pose = np.concatenate([[c, 0.0, -sn, 0.0], -R.T @ np.array([0.0, 0.0, forward])])
    from stereo_vo_amd import api
    assert np.allclose(api.pose7_to_cam_to_world(pose).reshape(12), here, rtol=0, atol=1e-12)
    import voxel_align_ref as A  # the tests' maker of a displaced pose: the shift in the world frame, the turn on the camera side
    start = np.array(A.displaced(pose, [0.5 * vs * c for c in (0.6, -0.5, 0.62)], [0.01 * c for c in (0.5, 0.7, -0.5)]))
    for _ in range(warmup):
        vm.align(p, n, start)
    t0 = time.perf_counter()
    for _ in range(5):
        pose_out, res = vm.align(p, n, start)
    out["loop_wall_ms"] = 1e3 * (time.perf_counter() - t0) / 5
    ctx.profile_select("voxel_align")
    t0 = time.perf_counter()
    vm.align(p, n, start)
    wall = 1e3 * (time.perf_counter() - t0)
    ms, k = ctx.profile_read()
    ctx.profile_select("")
    assert k == res["iterations"], (k, res)
    out.update({"loop_iterations": res["iterations"], "loop_status": res["status"], "loop_first_matched": res["first_matched"],
                "loop_last_matched": res["last_matched"], "loop_first_cost": res["first_cost"], "loop_last_cost": res["last_cost"],
                "loop_brackets_ms": ms, "loop_profiled_wall_ms": wall, "loop_share_outside_brackets": 1.0 - ms / wall,
                "loop_start_shift": float(0.5 * vs * np.linalg.norm([0.6, -0.5, 0.62])), "loop_start_pose7": [float(v) for v in start],
                "loop_shift_left": float(np.linalg.norm(api.pose7_to_cam_to_world(pose_out)[:, 3] - np.array([0.0, 0.0, forward])))})
    return {"align": out}


def align_line(k, insert_ms):
    """Section 18's lines of the text report for one align_view."""
    return (f"sums of the last inserted cloud ({k['points']} points) under its own pose (memset + one launch, mean of 5): reach 0 "
            f"{1e3 * k['sums_reach0_ms']:.1f} us, counts {k['sums_reach0_counts']}; reach 1 {1e3 * k['sums_reach1_ms']:.1f} us, counts {k['sums_reach1_counts']} "
            f"(matched, rejected, unmatched, far); the same run's insert of the same cloud {1e3 * insert_ms:.1f} us -> reach 0 / insert "
            f"{k['sums_reach0_ms'] / insert_ms:.2f}, reach 1 / insert {k['sums_reach1_ms'] / insert_ms:.2f}\n"
            f"  align from that pose displaced by half a voxel ({k['loop_start_shift']:.4f}) and 0.01 rad, defaults: {k['loop_wall_ms']:.3f} ms wall clock (mean of 5), "
            f"{k['loop_iterations']} iterations, status {k['loop_status']}, matched {k['loop_first_matched']} -> {k['loop_last_matched']}, cost word "
            f"{k['loop_first_cost']} -> {k['loop_last_cost']}, shift left {k['loop_shift_left']:.4f}; one more run with the brackets on: {k['loop_profiled_wall_ms']:.3f} ms, "
            f"of which {k['loop_brackets_ms']:.3f} ms inside the brackets -> {100 * k['loop_share_outside_brackets']:.1f} % is the 256-byte copies, the waits and the host solves\n")


def normals_view(torch, ctx, vm, cloud, n, angle, forward, warmup, align):
    """Section 19 for one filled map: the normals launch at the defaults, the plane sums of the last inserted cloud under its own pose
    at reach 0 and 1, and the plane loop from section 18's displaced pose (`align`: section 18's figures of this map).  Nothing in
    the map changes."""
    import voxel_ref as V
    from stereo_vo_amd import api
    here = V.rot_y(angle, (0.0, 0.0, forward))
    nbuf = torch.empty(vm.capacity * 4, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(api.VOXEL_NORMALS_COUNTS, dtype=torch.int64, device="cuda")
    sums = torch.zeros(api.VOXEL_ALIGN_PLANE_WORDS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p, out = cloud.data_ptr(), {"points": n, "capacity": vm.capacity}
    for _ in range(warmup):
        vm.normals(nbuf.data_ptr(), counts_ptr=cnt.data_ptr())
    ctx.profile_select("voxel_normals")
    for _ in range(5):
        vm.normals(nbuf.data_ptr(), counts_ptr=cnt.data_ptr())
    ms, k = ctx.profile_read()
    ctx.profile_select("")
    assert k == 5, k
    out["normals_ms"] = ms / k
    out["normals_counts"] = [int(v) for v in cnt.cpu()[:5]]
    out["load"] = vm.stats()["n_voxels"] / vm.capacity
    for reach in (0, 1):
        for _ in range(warmup):
            vm.align_plane_sums(nbuf.data_ptr(), p, n, c2w12=here, sums_ptr=sums.data_ptr(), reach=reach)
        ctx.profile_select("voxel_align_plane")
        for _ in range(5):
            vm.align_plane_sums(nbuf.data_ptr(), p, n, c2w12=here, sums_ptr=sums.data_ptr(), reach=reach)
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        assert k == 5, k
        out[f"sums_reach{reach}_ms"] = ms / k
        out[f"sums_reach{reach}_counts"] = [int(v) for v in sums.cpu()[29:34]]
    start = np.array(align["loop_start_pose7"])
    for _ in range(warmup):
        vm.align_plane(nbuf.data_ptr(), p, n, start)
    t0 = time.perf_counter()
    for _ in range(5):
        pose_out, res = vm.align_plane(nbuf.data_ptr(), p, n, start)
    out["loop_wall_ms"] = 1e3 * (time.perf_counter() - t0) / 5
    out.update({"loop_iterations": res["iterations"], "loop_status": res["status"], "loop_first_matched": res["first_matched"],
                "loop_last_matched": res["last_matched"], "loop_first_cost": res["first_cost"], "loop_last_cost": res["last_cost"],
                "loop_shift_left": float(np.linalg.norm(api.pose7_to_cam_to_world(pose_out)[:, 3] - np.array([0.0, 0.0, forward])))})
    return {"normals": out}


def locate_view(torch, ctx, vm, cloud, n, angle, forward, warmup, align, extract_ms):
    """Section 20 for one filled map (`align`: section 18's figures of this map).  Nothing in the map changes."""
    import voxel_locate_ref as L
    import voxel_ref as V
    from stereo_vo_amd import api
    vs = float(vm.params.voxel_size)
    c, sn = np.cos(angle / 2), np.sin(angle / 2)
    R = np.asarray(V.rot_y(angle, (0.0, 0.0, forward))).reshape(3, 4)[:, :3]
    pose = np.concatenate([[c, 0.0, -sn, 0.0], -R.T @ np.array([0.0, 0.0, forward])])
    prm = api.voxel_locate_default_params(vs)
    ref = L.default_params()
    T, _, mats = L.candidates(pose, ref)
    origin = L.origin_of(T, vs, ref.dims)
    ws = torch.empty(api.voxel_locate_workspace_bytes(prm) + 256, dtype=torch.uint8, device="cuda")
    bits = torch.empty(api.voxel_occupancy_bytes(ref.dims) // 8, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    best = torch.zeros(9 * 8, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p, out = cloud.data_ptr(), {"points": n, "capacity": vm.capacity, "extract_ms": extract_ms, "dims": list(ref.dims), "K": len(mats)}
    for _ in range(warmup):
        vm.occupancy(bits.data_ptr(), origin, ref.dims, counts_ptr=cnt.data_ptr())
    ctx.profile_select("voxel_occupancy")
    for _ in range(5):
        vm.occupancy(bits.data_ptr(), origin, ref.dims, counts_ptr=cnt.data_ptr())
    ms, k = ctx.profile_read()
    ctx.profile_select("")
    assert k == 5, k
    out["occupancy_ms"] = ms / k
    out["occupancy_counts"] = [int(v) for v in cnt.cpu()]
    for box in ((8, 4, 8), (16, 4, 16)):
        shifts = (2 * box[0] + 1) * (2 * box[1] + 1) * (2 * box[2] + 1)
        hits = torch.zeros(len(mats) * shifts, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        call = lambda: vm.locate_scores(bits.data_ptr(), origin, ref.dims, p, n, np.array(mats), box, hits_ptr=hits.data_ptr(), best_ptr=best.data_ptr())
        for _ in range(warmup):
            call()
        ctx.profile_select("voxel_locate")
        for _ in range(5):
            call()
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        assert k == 5, k
        b = best.cpu().numpy().view(L.BEST)
        tag = "x".join(str(v) for v in box)
        out[f"scores_{tag}_ms"] = ms / k
        out[f"scores_{tag}_tests_per_s"] = n * len(mats) * shifts / (1e-3 * ms / k)
        out[f"scores_{tag}_best"] = [int(b["hits_max"][4]), int(b["s0"][4]), int(b["s1"][4]), int(b["s2"][4]), int(b["n_used"][4]), int(b["n_inside"][4])]
    out["align_lookups_per_s"] = 27 * n / (1e-3 * align["sums_reach1_ms"])
    start = np.array(L.start_pose(pose, [5.3 * vs, -1.7 * vs, 4.2 * vs], 0.11))
    wptr = (ws.data_ptr() + 255) & ~255
    nbuf = torch.empty(vm.capacity * 4, dtype=torch.float32, device="cuda")
    vm.normals(nbuf.data_ptr())
    ctx.sync()
    for name, nptr in (("point", None), ("plane", nbuf.data_ptr())):
        for _ in range(warmup):
            vm.locate(p, n, start, normals_ptr=nptr, workspace_ptr=wptr)
        t0 = time.perf_counter()
        for _ in range(5):
            pose_out, res = vm.locate(p, n, start, normals_ptr=nptr, workspace_ptr=wptr)
        out[f"locate_{name}_wall_ms"] = 1e3 * (time.perf_counter() - t0) / 5
        out[f"locate_{name}"] = {"status": res["status"], "k": res["k"], "shift": list(res["shift"]), "hits": res["hits"], "rank": res["rank"],
                                 "align_status": res["align"]["status"], "align_iterations": res["align"]["iterations"],
                                 "shift_left": float(np.linalg.norm(api.pose7_to_cam_to_world(pose_out)[:, 3] - np.array([0.0, 0.0, forward])))}
    out["locate_start_shift"] = float(vs * np.linalg.norm([5.3, -1.7, 4.2]))
    return {"locate": out}


def rays_view(torch, ctx, cam, vm, angle, forward, warmup, locate):
    """Section 21 for one filled map (`locate`: section 20's figures of this map).  Nothing in the map changes."""
    import voxel_locate_ref as L
    import voxel_rays_ref as RR
    import voxel_ref as V
    from stereo_vo_amd import api
    vs = float(vm.params.voxel_size)
    c2w = np.asarray(V.rot_y(angle, (0.0, 0.0, forward)), np.float64).reshape(12)
    dims = L.default_params().dims
    origin = RR.origin_of((c2w[3], c2w[7], c2w[11]), vs, dims)
    bits = torch.empty(api.voxel_occupancy_bytes(dims) // 8, dtype=torch.int64, device="cuda")
    coarse = torch.empty(api.voxel_occupancy_coarse_bytes(dims) // 8, dtype=torch.int64, device="cuda")
    occ = torch.zeros(2, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(7, dtype=torch.int64, device="cuda")
    disp, cell = torch.empty(W * H, dtype=torch.int16, device="cuda"), torch.empty(W * H, dtype=torch.int32, device="cuda")
    n = 1 << 18
    rng = np.random.default_rng(21)
    rays = np.zeros(n, api.VoxelRay)
    centre = [(origin[r] + dims[r] / 2 + 0.37) * vs for r in range(3)]
    rays["ox"], rays["oy"], rays["oz"], rays["max_range"] = centre[0], centre[1], centre[2], 30.0
    d = rng.normal(size=(n, 3)).astype(np.float32)
    rays["dx"], rays["dy"], rays["dz"] = d[:, 0], d[:, 1], d[:, 2]
    drays = torch.from_numpy(rays.view(np.int32).reshape(-1, 8)).cuda()
    hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    vm.occupancy(bits.data_ptr(), origin, dims, counts_ptr=occ.data_ptr())
    torch.cuda.synchronize()

    def timed(tag, call):
        for _ in range(warmup):
            call()
        ctx.profile_select(tag)
        for _ in range(5):
            call()
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        assert k == 5, k
        return ms / k

    out = {"dims": list(dims), "occupancy_ms": locate["occupancy_ms"], "occupancy_counts": [int(v) for v in occ.cpu()], "rays": n, "image": [W, H]}
    out["coarse_ms"] = timed("voxel_coarse", lambda: vm.occupancy_coarse(bits.data_ptr(), dims, coarse.data_ptr()))
    words, cw = bits.cpu().numpy().view(np.uint64), coarse.cpu().numpy().view(np.uint64)
    out["coarse_blocks_set"] = int(np.unpackbits(cw.view(np.uint8)).sum())
    out["coarse_blocks"] = int(np.prod(RR.coarse_dims(dims)))
    seen = {}
    for name, cp in (("plain", None), ("skip", coarse.data_ptr())):
        out[f"raycast_{name}_ms"] = timed("voxel_rays", lambda: vm.raycast(bits.data_ptr(), origin, dims, W, H, cam, c2w12=c2w, coarse_ptr=cp, disp_ptr=disp.data_ptr(),
                                                                        cell_ptr=cell.data_ptr(), counts_ptr=cnt.data_ptr()))
        out["raycast_counts"] = [int(v) for v in cnt.cpu()]
        view = (disp.cpu().numpy().tobytes(), cell.cpu().numpy().tobytes(), out["raycast_counts"])
        out[f"rays_{name}_ms"] = timed("voxel_rays", lambda: vm.rays(bits.data_ptr(), origin, dims, drays.data_ptr(), n, hits_ptr=hits.data_ptr(), coarse_ptr=cp,
                                                                  counts_ptr=cnt.data_ptr()))
        out["rays_counts"] = [int(v) for v in cnt.cpu()[:6]]
        seen[name] = (view, hits.cpu().numpy().tobytes(), out["rays_counts"])
    assert seen["plain"] == seen["skip"], "the two walks differ"
    out["raycast_steps_per_ray"] = out["raycast_counts"][5] / (W * H)
    out["rays_steps_per_ray"] = out["rays_counts"][5] / n
    vol = RR.Volume(words, dims, cw)
    steps = jumped = jumps = 0
    for ray in rays[:4096]:
        s = RR.setup_a(*RR.widen(ray), vs, origin)
        if s is not None:
            e, j, k = RR.walk_skip(s, vol, 1)
            steps, jumped, jumps = steps + e[3], jumped + j, jumps + k
    out.update({"sample_steps": steps, "sample_jumped": jumped, "sample_jumps": jumps})
    ws = torch.empty(W * H, dtype=torch.int32, device="cuda")
    gg = torch.empty(W * H, dtype=torch.uint8, device="cuda")
    w2c = np.linalg.inv(np.vstack([c2w.reshape(3, 4), [0, 0, 0, 1]]))[:3].reshape(12)
    torch.cuda.synchronize()
    out["render_ms"] = timed("voxel_render", lambda: vm.render(W, H, cam, w2c12=w2c, workspace_ptr=ws.data_ptr(), disp_ptr=disp.data_ptr(), intensity_ptr=gg.data_ptr()))
    return {"rays": out}


def distance_steps(words, dims, max_dist, mid, dist2):
    """Section 22's steps per cell of the three passes, by the search's stop rule: words read per cell's wavefront along axis 0
    (its own, then each side up to the first non-zero word, ceil(max_dist / 64) words or the row's end), and the outward steps along
    axes 1 and 2, a batch of four at a time while g <= reach and g * g <= the pass's result (mid: the axis-1 pass's u16 squares,
    dist2: the final ones; 0xFFFF: nothing found, the search runs to its reach)."""
    d0, d1, d2 = dims
    wpr, K = d0 // 64, (max_dist + 63) // 64
    nz = (np.asarray(words).reshape(-1, wpr) != 0)
    x = np.arange(wpr)[None, :]
    last = np.maximum.accumulate(np.where(nz, x, -1), axis=1)
    prev = np.concatenate([np.full((len(nz), 1), -1), last[:, :-1]], axis=1)          # the nearest non-zero word to the left, or -1
    nxt_ = np.minimum.accumulate(np.where(nz, x, 2 * wpr)[:, ::-1], axis=1)[:, ::-1]
    nxt = np.concatenate([nxt_[:, 1:], np.full((len(nz), 1), 2 * wpr)], axis=1)      # to the right, or beyond the row
    left = np.minimum(np.minimum(K, x), np.where(prev >= 0, x - prev, K))
    right = np.minimum(np.minimum(K, wpr - 1 - x), np.where(nxt < wpr, nxt - x, K))
    row_words = float((1 + left + right).mean())
    out = [row_words]
    for arr, ax, L in ((mid, 1, d1), (dist2, 0, d2)):
        a = np.asarray(arr).reshape(d2, d1, d0)
        pos = np.arange(L).reshape((-1, 1, 1) if ax == 0 else (1, -1, 1))
        reach = np.minimum(max_dist, np.maximum(pos, L - 1 - pos))
        root = np.where(a == 0xFFFF, 255, np.floor(np.sqrt(a.astype(np.float64))).astype(np.int64))
        out.append(float((4 * (np.minimum(reach, root) // 4 + 1)).mean()))
    return out


def distance_view(torch, ctx, vm, angle, forward, warmup, locate, copy):
    """Section 22 for one filled map (`locate`: section 20's figures of this map).  Nothing in the map changes."""
    import voxel_locate_ref as L
    import voxel_rays_ref as RR
    import voxel_ref as V
    from stereo_vo_amd import api
    vs = float(vm.params.voxel_size)
    c2w = np.asarray(V.rot_y(angle, (0.0, 0.0, forward)), np.float64).reshape(12)
    dims = tuple(L.default_params().dims)
    origin = RR.origin_of((c2w[3], c2w[7], c2w[11]), vs, dims)
    cells = dims[0] * dims[1] * dims[2]
    bits = torch.empty(cells // 64, dtype=torch.int64, device="cuda")
    occ = torch.zeros(2, dtype=torch.int32, device="cuda")
    ws = torch.empty(api.voxel_distance_workspace_bytes(dims, True) // 8, dtype=torch.int64, device="cuda")
    d2 = torch.empty(cells, dtype=torch.int16, device="cuda")
    near, clr = torch.empty(cells, dtype=torch.int32, device="cuda"), torch.empty(cells, dtype=torch.float32, device="cuda")
    infl = torch.empty(cells // 64, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(6, dtype=torch.int64, device="cuda")
    n = 1 << 18
    rng = np.random.default_rng(22)
    sph = np.zeros(n, api.VoxelSphere)
    for r, k in enumerate(("x", "y", "z")):
        sph[k] = ((origin[r] + rng.uniform(-0.05 * dims[r], 1.05 * dims[r], n)) * vs).astype(np.float32)
    sph["radius"] = rng.uniform(0.0, 1.0, n).astype(np.float32)
    dsph = torch.from_numpy(sph.view(np.int32).reshape(-1, 4)).cuda()
    hits = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    vm.occupancy(bits.data_ptr(), origin, dims, counts_ptr=occ.data_ptr())
    torch.cuda.synchronize()
    words = bits.cpu().numpy().view(np.uint64)

    def timed(tag, call):
        for _ in range(warmup):
            call()
        ctx.profile_select(tag)
        for _ in range(5):
            call()
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        assert k == 5, k
        return ms / k

    out = {"dims": list(dims), "occupancy_ms": locate["occupancy_ms"], "occupancy_counts": [int(v) for v in occ.cpu()], "spheres": n,
           "bound_dist2_ms": 1e3 * 8.125 * cells / copy, "bound_all_ms": 1e3 * 22.25 * cells / copy, "runs": []}
    for md in (8, 32, 128):
        k = {"max_dist": md}
        k["dist2_ms"] = timed("voxel_distance", lambda: vm.distance(bits.data_ptr(), dims, workspace_ptr=ws.data_ptr(), dist2_ptr=d2.data_ptr(), counts_ptr=cnt.data_ptr(),
                                                                     max_dist=md, inflate_radius=3.0 * vs))
        k["counts"] = [int(v) for v in cnt.cpu()[:4]]
        plain = d2.cpu().numpy().view(np.uint16)
        mid = ws.cpu().numpy().view(np.uint16)[cells // 2:cells // 2 + cells]  # the axis-1 pass's squares: behind the u8 part
        k["steps"] = distance_steps(words, dims, md, mid, plain)
        k["all_ms"] = timed("voxel_distance", lambda: vm.distance(bits.data_ptr(), dims, workspace_ptr=ws.data_ptr(), dist2_ptr=d2.data_ptr(), nearest_ptr=near.data_ptr(),
                                                                   clearance_ptr=clr.data_ptr(), inflated_ptr=infl.data_ptr(), counts_ptr=cnt.data_ptr(), max_dist=md,
                                                                   inflate_radius=3.0 * vs))
        assert k["counts"] == [int(v) for v in cnt.cpu()[:4]] and np.array_equal(plain, d2.cpu().numpy().view(np.uint16)), "the two forms differ"
        k["query_ms"] = timed("voxel_distance_query", lambda: vm.distance_query(d2.data_ptr(), origin, dims, dsph.data_ptr(), n, hits_ptr=hits.data_ptr(),
                                                                                 counts_ptr=cnt.data_ptr()))
        k["query_counts"] = [int(v) for v in cnt.cpu()]
        out["runs"].append(k)
    return {"distance": out}


def distance_line(k):
    """Section 22's lines of the text report for one distance_view."""
    s = (f"distance field of {k['dims']} (counts' memset + three launches, mean of 5); the same run's occupancy {1e3 * k['occupancy_ms']:.1f} us "
         f"(counts {k['occupancy_counts']}); 8.125 B per cell at hbm_copy {1e3 * k['bound_dist2_ms']:.1f} us, 22.25 B per cell {1e3 * k['bound_all_ms']:.1f} us\n")
    for r in k["runs"]:
        s += (f"  max_dist {r['max_dist']}: dist2 alone {1e3 * r['dist2_ms']:.1f} us ({r['dist2_ms'] / k['bound_dist2_ms']:.1f} x its byte bound), all four outputs "
              f"{1e3 * r['all_ms']:.1f} us ({r['all_ms'] / k['bound_all_ms']:.1f} x); counts {r['counts']} (sources, reached, unreached, inflated); per cell "
              f"{r['steps'][0]:.2f} words along axis 0, {r['steps'][1]:.1f} + {r['steps'][2]:.1f} steps along axes 1 and 2; query of {k['spheres']} spheres "
              f"{1e3 * r['query_ms']:.1f} us, counts {r['query_counts']} (n, free, collides, outside, rejected, beyond)\n")
    return s


def voxel_route_view(torch, ctx, vm, angle, forward, warmup, copy):
    """Section 23 for one filled map.  Nothing in the map changes."""
    import voxel_locate_ref as L
    import voxel_rays_ref as RR
    import voxel_ref as V
    import voxel_route_ref as VR
    from stereo_vo_amd import api
    vs = float(vm.params.voxel_size)
    c2w = np.asarray(V.rot_y(angle, (0.0, 0.0, forward)), np.float64).reshape(12)
    dims = tuple(L.default_params().dims)
    origin = RR.origin_of((c2w[3], c2w[7], c2w[11]), vs, dims)
    cells = dims[0] * dims[1] * dims[2]
    bits = torch.empty(cells // 64, dtype=torch.int64, device="cuda")
    occ = torch.zeros(2, dtype=torch.int32, device="cuda")
    dws = torch.empty(api.voxel_distance_workspace_bytes(dims, False) // 8, dtype=torch.int64, device="cuda")
    d2 = torch.empty(cells, dtype=torch.int16, device="cuda")
    infl = torch.empty(cells // 64, dtype=torch.int64, device="cuda")
    ws = torch.empty(api.voxel_route_workspace_bytes(dims) // 8, dtype=torch.int64, device="cuda")
    cost = torch.empty(cells, dtype=torch.int32, device="cuda")
    nxt = torch.empty(cells, dtype=torch.uint8, device="cuda")
    n_starts, max_path = 64, 4096
    path = torch.empty(n_starts * max_path, dtype=torch.int32, device="cuda")
    plen = torch.empty(n_starts, dtype=torch.int32, device="cuda")
    pst = torch.empty(n_starts, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    vm.occupancy(bits.data_ptr(), origin, dims, counts_ptr=occ.data_ptr())
    out = {"dims": list(dims), "tile": None, "occupancy_counts": None, "hbm_copy_bytes_per_s": copy, "runs": []}
    tiles = (api.voxel_route_workspace_bytes(dims) - 64 - cells) // 8
    out["tiles"] = int(tiles)
    out["tile"] = "8 x 8 x 8" if api.voxel_route_workspace_bytes((64, 8, 4)) == 64 + 8 * 8 + 2048 else "16 x 8 x 4"  # 8 tiles or 4: the library's shape
    for radius in (0.0, 0.3):
        vm.distance(bits.data_ptr(), dims, workspace_ptr=dws.data_ptr(), dist2_ptr=d2.data_ptr(), inflated_ptr=infl.data_ptr(), max_dist=8, inflate_radius=radius)
        torch.cuda.synchronize()
        out["occupancy_counts"] = [int(v) for v in occ.cpu()]
        closed = VR.unpack(infl.cpu().numpy().view(np.uint64), dims)
        free = np.flatnonzero(~closed.ravel())
        centre = dims[0] // 2 + dims[0] * (dims[1] // 2 + dims[1] * (dims[2] // 2))
        goal = int(free[np.argmin(np.abs(free - centre))])  # the camera's cell, or the free cell whose number is nearest to it
        rng = np.random.default_rng(23)
        goals = torch.from_numpy(np.array([goal], np.uint32).view(np.int32)).cuda()
        starts = torch.from_numpy(free[rng.integers(0, len(free), n_starts)].astype(np.uint32).view(np.int32)).cuda()

        def call(max_rounds, with_d2, paths):
            vm.route(infl.data_ptr(), dims, goals.data_ptr(), 1, dist2_ptr=d2.data_ptr() if with_d2 else None, starts_ptr=starts.data_ptr() if paths else None,
                     n_starts=n_starts if paths else 0, workspace_ptr=ws.data_ptr(), cost_ptr=cost.data_ptr(), next_ptr=nxt.data_ptr() if paths else None,
                     path_ptr=path.data_ptr() if paths else None, path_len_ptr=plen.data_ptr() if paths else None, path_status_ptr=pst.data_ptr() if paths else None,
                     counts_ptr=cnt.data_ptr(), near_r2=16 if with_d2 else 0, near_weight=4 if with_d2 else 0, max_rounds=max_rounds, max_path=max_path)

        def timed(max_rounds, with_d2, paths):
            for _ in range(warmup):
                call(max_rounds, with_d2, paths)
            ctx.profile_select("voxel_route")
            for _ in range(5):
                call(max_rounds, with_d2, paths)
            ms, k = ctx.profile_read()
            ctx.profile_select("")
            assert k == 5, k
            return ms / k

        for with_d2 in (False, True):
            k = {"inflate_radius": radius, "closed": int(closed.sum()), "with_dist2": with_d2}
            call(1024, with_d2, False)
            ctx.sync()
            c = [int(v) for v in cnt.cpu()]
            k["counts"], k["rounds_run"] = c[:5], c[5]
            need = min(c[5] + 1, 4096)  # one more round finds nothing to do
            k["cost_ms"] = timed(need, with_d2, False)
            ctx.sync()
            k["converged_at_need"] = int(cnt.cpu()[4])
            k["cost_ms_64_more"] = timed(need + 64, with_d2, False)
            k["empty_round_us"] = 1e3 * (k["cost_ms_64_more"] - k["cost_ms"]) / 64
            k["ms_per_round"] = k["cost_ms"] / max(c[5], 1)
            k["default_ms"] = timed(api.voxel_route_default_params(vs).max_rounds, with_d2, False)
            ctx.sync()
            k["converged_at_default"] = int(cnt.cpu()[4])
            k["paths_ms"] = timed(need, with_d2, True)
            ctx.sync()
            lens = plen.cpu().numpy().view(np.uint32)
            k["longest_path"], k["path_status"] = int(lens.max()), np.bincount(pst.cpu().numpy(), minlength=5).tolist()
            # one pass over the arrays: cost 4 B by the memset, 4 read and 4 written by the tiles, closed 1/8 (+ dist2 2); with next and
            # paths the finish launch reads cost 4 + closed 1/8 (+ dist2 2) and writes next and the workspace's byte
            k["bound_cost_ms"] = 1e3 * (12.125 + (2 if with_d2 else 0)) * cells / copy
            k["bound_paths_ms"] = 1e3 * (12.125 + 6.125 + (4 if with_d2 else 0)) * cells / copy
            out["runs"].append(k)
    return {"voxel_route": out}


def voxel_route_line(k):
    """Section 23's lines of the text report for one voxel_route_view."""
    s = (f"route through {k['dims']}, tile {k['tile']} ({k['tiles']} workgroups per round), goal at the free cell nearest the centre, 64 random free starts, max_dist 8 "
         f"(one \"voxel_route\" bracket, mean of 5); occupancy counts {k['occupancy_counts']}; hbm_copy {k['hbm_copy_bytes_per_s'] / 1e12:.3f} TB/s in this run\n")
    for r in k["runs"]:
        s += (f"  inflate_radius {r['inflate_radius']} m ({r['closed']} closed cells), {'with' if r['with_dist2'] else 'without'} dist2: counts {r['counts']} (goals used, reached, "
              f"unreached, closed, converged at 1,024 rounds), rounds_run {r['rounds_run']}; cost alone at rounds_run + 1: {r['cost_ms']:.3f} ms (converged "
              f"{r['converged_at_need']}) = {1e3 * r['ms_per_round']:.1f} us per round; with 64 more rounds {r['cost_ms_64_more']:.3f} ms -> {r['empty_round_us']:.2f} us per "
              f"round that finds nothing to do; at the default max_rounds {r['default_ms']:.3f} ms (converged {r['converged_at_default']}); with next and 64 paths "
              f"{r['paths_ms']:.3f} ms, longest path {r['longest_path']} cells, statuses {r['path_status']}; one pass over the arrays at hbm_copy "
              f"{1e3 * r['bound_cost_ms']:.0f} us (cost alone) / {1e3 * r['bound_paths_ms']:.0f} us (with next)\n")
    return s


def rays_line(k):
    """Section 21's lines of the text report for one rays_view."""
    return (f"coarse volume of {k['dims']} (memset + launch, mean of 5): {1e3 * k['coarse_ms']:.1f} us, {k['coarse_blocks_set']} of {k['coarse_blocks']} blocks set; "
            f"the same run's occupancy {1e3 * k['occupancy_ms']:.1f} us (counts {k['occupancy_counts']}) and splat render at the defaults {1e3 * k['render_ms']:.1f} us\n"
            f"  camera form {k['image'][0]} x {k['image'][1]} from the map's own pose (counts' memset + launch, mean of 5): plain walk {1e3 * k['raycast_plain_ms']:.1f} us, "
            f"block-skipping walk {1e3 * k['raycast_skip_ms']:.1f} us -> skip / plain {k['raycast_skip_ms'] / k['raycast_plain_ms']:.3f}; counts {k['raycast_counts']} "
            f"(hit, left, range, outside, rejected, steps, pixels), {k['raycast_steps_per_ray']:.1f} steps per ray\n"
            f"  {k['rays']} random rays from the volume's centre, range 30 m: plain {1e3 * k['rays_plain_ms']:.1f} us, block-skipping {1e3 * k['rays_skip_ms']:.1f} us -> skip / plain "
            f"{k['rays_skip_ms'] / k['rays_plain_ms']:.3f}; counts {k['rays_counts']}, {k['rays_steps_per_ray']:.1f} steps per ray; of the first 4,096 rays' "
            f"{k['sample_steps']} visited cells the skipping walk jumps {k['sample_jumped']} ({100.0 * k['sample_jumped'] / max(k['sample_steps'], 1):.1f} %) in {k['sample_jumps']} jumps "
            f"(restatement); the outputs of the two walks are equal in every byte\n")


def locate_line(k, a):
    """Section 20's lines of the text report for one locate_view beside its align_view `a`."""
    s = ""
    for tag in ("8x4x8", "16x4x16"):
        s += (f"; box {tag.replace('x', ', ')}: {1e3 * k['scores_' + tag + '_ms']:.1f} us, {k['scores_' + tag + '_tests_per_s'] / 1e9:.1f} G tests/s, "
              f"identity candidate {k['scores_' + tag + '_best']}")
    out = (f"occupancy of 2^{k['capacity'].bit_length() - 1} slots into {k['dims']} (two memsets + launch, mean of 5): {1e3 * k['occupancy_ms']:.1f} us, counts "
           f"{k['occupancy_counts']} (inside, outside); the same run's extraction walk {1e3 * k['extract_ms']:.1f} us -> {k['occupancy_ms'] / k['extract_ms']:.2f}\n"
           f"  scores of the last inserted cloud ({k['points']} points), {k['K']} candidates (memsets + score launch + best launch, mean of 5; hits_max, shift, n_used, "
           f"n_inside){s}; the same run's reach-1 align sums {1e3 * a['sums_reach1_ms']:.1f} us = {k['align_lookups_per_s'] / 1e9:.2f} G look-ups/s\n")
    for name in ("point", "plane"):
        r = k["locate_" + name]
        out += (f"  locate ({name} form) from that pose moved by {k['locate_start_shift']:.3f} and 0.11 rad, defaults: {k['locate_' + name + '_wall_ms']:.3f} ms wall clock (mean of 5), "
                f"{r['status']}, candidate {r['k']} shift {r['shift']} hits {r['hits']} rank {r['rank']}, refinement {r['align_status']} after {r['align_iterations']} iterations, "
                f"shift left {r['shift_left']:.4f}\n")
    return out


def normals_line(k, a, insert_ms):
    """Section 19's lines of the text report for one normals_view beside its align_view `a`."""
    c = k['normals_counts']
    return (f"one launch over 2^{k['capacity'].bit_length() - 1} slots at load {k['load']:.3f} (counts' memset + launch, mean of 5): {1e3 * k['normals_ms']:.1f} us, counts {c} "
            f"(centres, valid, few, collinear, curved) -> {1e6 * k['normals_ms'] / max(c[0], 1):.2f} ns per live voxel\n"
            f"  plane sums of the last inserted cloud ({k['points']} points) under its own pose (memset + one launch, mean of 5): reach 0 "
            f"{1e3 * k['sums_reach0_ms']:.1f} us, counts {k['sums_reach0_counts']}; reach 1 {1e3 * k['sums_reach1_ms']:.1f} us, counts {k['sums_reach1_counts']} "
            f"(matched, rejected, unmatched, far, no normal); plane / point sums {k['sums_reach0_ms'] / a['sums_reach0_ms']:.2f} at reach 0, "
            f"{k['sums_reach1_ms'] / a['sums_reach1_ms']:.2f} at reach 1; plane / insert {k['sums_reach0_ms'] / insert_ms:.2f} and {k['sums_reach1_ms'] / insert_ms:.2f}\n"
            f"  plane align from section 18's displaced pose, defaults: {k['loop_wall_ms']:.3f} ms wall clock (mean of 5), {k['loop_iterations']} iterations, status "
            f"{k['loop_status']}, matched {k['loop_first_matched']} -> {k['loop_last_matched']}, cost word {k['loop_first_cost']} -> {k['loop_last_cost']}, shift left "
            f"{k['loop_shift_left']:.4f}; the point form from the same pose {a['loop_wall_ms']:.3f} ms, {a['loop_iterations']} iterations, shift left {a['loop_shift_left']:.4f}\n")


def grid_view(S, torch, ctx, vm, c2w, warmup, copy):
    """Section 11 for one filled map: its ground plan around the last cloud's pose, at the defaults."""
    prm = S.api.voxel_grid_default_params(vm.params.voxel_size)
    x, z = float(c2w.reshape(3, 4)[0, 3]), float(c2w.reshape(3, 4)[2, 3])
    prm.origin_a, prm.origin_b = prm.origin_a + z, prm.origin_b + x  # a = z forward, b = x right
    n = prm.na * prm.nb
    ws = torch.empty(4 * n, dtype=torch.int64, device="cuda")
    cls, inten = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2))
    top, bottom = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(2))
    nvox = torch.empty(n, dtype=torch.int32, device="cuda")
    npts, cnt = torch.empty(n, dtype=torch.int64, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    kw = dict(workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr(), top_ptr=top.data_ptr(), bottom_ptr=bottom.data_ptr(), intensity_ptr=inten.data_ptr(),
              n_voxels_ptr=nvox.data_ptr(), n_points_ptr=npts.data_ptr(), counts_ptr=cnt.data_ptr())

    def timed(pre):
        vm.grid_set_mode(pre)
        for _ in range(warmup):
            vm.grid(prm, **kw)
        ctx.profile_select("voxel_grid")
        for _ in range(5):
            vm.grid(prm, **kw)
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        vm.grid_set_mode()  # back to the default
        return ms / k, tuple(t.cpu().numpy().tobytes() for t in (ws, cls, top, bottom, inten, nvox, npts, cnt))

    modes = {}
    for _ in range(2):  # alternating
        for name, pre in (("no pre-check", False), ("pre-check", True)):
            got = timed(pre)
            modes.setdefault(name, []).append(got[0])
            assert got[1] == modes.setdefault("bytes", got[1]), "a mode of the walk changed the grid"
    del modes["bytes"]
    ms, k = timed(None)[0], 1
    counts = [int(v) for v in cnt.cpu()]
    c = cls.cpu().numpy()
    bound = 1e3 * (16 * vm.capacity + 8 * counts[0] + (64 + 26) * n) / copy
    return {"grid_ms": ms / k, "grid_counts": counts, "grid_cells": [prm.na, prm.nb], "grid_cell_voxels": prm.cell_voxels,
            "grid_classes": [int((c == v).sum()) for v in (0, 1, 2)], "grid_binned_per_cell": counts[2] / max(counts[3], 1),
            "grid_bound_ms": bound, "grid_share_of_bound": bound / (ms / k), "grid_modes_ms": modes}


def clearance_steps(cls, mask, max_dist):
    """The loop steps of the two passes summed over the cells, as the contract's suggested search takes them (one step looks at
    up to two cells): the row pass left before right until a source or the row's end, the column pass outward until g * g > best."""
    na, nb = cls.shape
    c = cls.astype(np.int64)
    src = (c < 32) & (((np.int64(mask) >> np.minimum(c, 31)) & 1) == 1)
    none = np.int64(1) << 40
    off = np.full((na, nb), none)
    ib = np.arange(nb)[None, :]
    for g in range(min(max_dist, nb - 1) + 1):
        left = np.zeros((na, nb), bool)
        left[:, g:] = src[:, :nb - g] if g else src
        right = np.zeros((na, nb), bool)
        right[:, :nb - g] = src[:, g:] if g else src
        off = np.where((off == none) & left, -g, np.where((off == none) & ~left & right, g, off))
    row_reach = np.minimum(max_dist, np.maximum(ib, nb - 1 - ib))
    row_steps = np.where(off == none, row_reach + 1, np.abs(off) + 1)
    best = np.full((na, nb), none)
    for g in range(min(max_dist, na - 1) + 1):
        for shifted in ((off[:na - g], slice(g, na)), (off[g:], slice(0, na - g))):
            o, rows = shifted
            best[rows] = np.minimum(best[rows], np.where(o == none, none, g * g + o * o))
    ia = np.arange(na)[:, None]
    col_reach = np.minimum(max_dist, np.maximum(ia, na - 1 - ia))
    col_steps = np.minimum(col_reach, np.floor(np.sqrt(np.minimum(best, 1 << 30).astype(np.float64))).astype(np.int64)) + 1
    return int(row_steps.sum()), int(col_steps.sum())


def clearance_random(torch, na, nb, density, seed=12):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.rand((na, nb), generator=g, device="cuda") < density).to(torch.uint8) * 2  # OBSTACLE with this probability, else UNKNOWN


def clearance_case(S, torch, ctx, cls, mask, max_dist, cell_size, warmup, copy, steps=False, density=None):
    """Section 12 for one (na, nb) uint8 device grid."""
    na, nb = cls.shape
    n = na * nb
    prm = S.api.GridClearanceParams(na, nb, mask, max_dist, cell_size, 2.0 * cell_size)
    ws, d2, near = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    clr = torch.empty(n, dtype=torch.float32, device="cuda")
    blk = torch.empty(n, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    kw = dict(workspace_ptr=ws.data_ptr(), dist2_ptr=d2.data_ptr(), nearest_ptr=near.data_ptr(), clearance_ptr=clr.data_ptr(),
              blocked_ptr=blk.data_ptr(), counts_ptr=cnt.data_ptr())
    for _ in range(warmup):
        ctx.grid_clearance(cls.data_ptr(), prm, **kw)
    ctx.profile_select("grid_clearance")
    for _ in range(5):
        ctx.grid_clearance(cls.data_ptr(), prm, **kw)
    ms, k = ctx.profile_read()
    ctx.profile_select("")
    bound = 1e3 * 22 * n / copy
    out = {"cells": [na, nb], "source_mask": mask, "max_dist": max_dist, "ms": ms / k, "counts": [int(v) for v in cnt.cpu()],
           "bound_ms": bound, "share_of_bound": bound / (ms / k)}
    if density is not None:
        out["density"] = density
    if steps:
        out["steps"] = clearance_steps(cls.cpu().numpy(), mask, max_dist)
    return out


def clearance_view(S, torch, ctx, vm, c2w, warmup, copy):
    """Section 12 for one filled map: the clearance of section 11's grid, with OBSTACLE cells as the sources and with UNKNOWN too."""
    gp = S.api.voxel_grid_default_params(vm.params.voxel_size)
    x, z = float(c2w.reshape(3, 4)[0, 3]), float(c2w.reshape(3, 4)[2, 3])
    gp.origin_a, gp.origin_b = gp.origin_a + z, gp.origin_b + x
    n = gp.na * gp.nb
    ws = torch.empty(4 * n, dtype=torch.int64, device="cuda")
    cls = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vm.grid(gp, workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr())
    ctx.sync()
    cp = S.api.grid_clearance_default_params(gp, vm.params.voxel_size)
    grid = cls.reshape(gp.na, gp.nb)
    return {"clearance": [clearance_case(S, torch, ctx, grid, mask, cp.max_dist, cp.cell_size, warmup, copy, steps=True)
                          for mask in (cp.source_mask, cp.source_mask | 1 << S.api.VOXEL_GRID_UNKNOWN)]}


def route_host_dijkstra(blocked, dist2, near_r2, near_weight, goal):
    """This tool's host Dijkstra over host copies (Python, a heap): the cost field only.  Returns the number of reached cells."""
    import heapq
    na, nb = blocked.shape
    B = (blocked.ravel() != 0).tolist()
    pen = np.zeros(na * nb, np.int64) if dist2 is None else np.where(dist2.ravel() < near_r2, near_weight * (near_r2 - dist2.ravel().astype(np.int64)), 0)
    unit = (16 + pen).tolist()
    cost = [-1] * (na * nb)
    if B[goal]:
        return 0
    heap, reached = [(0, goal)], 0
    best = {goal: 0}
    while heap:
        c, u = heapq.heappop(heap)
        if cost[u] >= 0:
            continue
        cost[u] = c
        reached += 1
        ua, ub = divmod(u, nb)
        for da in (-1, 0, 1):
            va = ua + da
            if va < 0 or va >= na:
                continue
            for db in (-1, 0, 1):
                vb = ub + db
                if (da == 0 and db == 0) or vb < 0 or vb >= nb:
                    continue
                v = va * nb + vb
                if B[v] or cost[v] >= 0 or (da and db and (B[va * nb + ub] or B[ua * nb + vb])):
                    continue
                c2 = c + (7 if da and db else 5) * unit[u]
                if c2 < best.get(v, 1 << 62):
                    best[v] = c2
                    heapq.heappush(heap, (c2, v))
    return reached


def route_random(torch, na, nb, density, seed=13):
    """A seeded grid, impassable with this probability, with the goal (the centre cell) and the starts (the corners) passable."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    b = (torch.rand((na, nb), generator=g, device="cuda") < density).to(torch.uint8)
    b[na // 2, nb // 2] = 0
    b[0, 0] = b[0, nb - 1] = b[na - 1, 0] = b[na - 1, nb - 1] = 0
    return b


def route_case(S, torch, ctx, blocked, dist2, near_r2, near_weight, warmup, copy, host_detour=False, density=None):
    """Section 13 for one (na, nb) uint8 device grid (passable iff 0) and its uint32 device dist2 (or None)."""
    api = S.api
    na, nb = blocked.shape
    n = na * nb
    goal = (na // 2) * nb + nb // 2
    h_starts = np.array([0, nb - 1, (na - 1) * nb, n - 1], np.uint32)
    max_path = 4096
    goals = torch.tensor([goal], dtype=torch.int32, device="cuda")
    starts = torch.from_numpy(h_starts.view(np.int32)).cuda()
    ws = torch.empty(api.grid_route_workspace_bytes(na, nb) // 8, dtype=torch.int64, device="cuda")
    cost = torch.empty(n, dtype=torch.int32, device="cuda")
    nxt = torch.empty(n, dtype=torch.uint8, device="cuda")
    path = torch.empty(len(h_starts) * max_path, dtype=torch.int32, device="cuda")
    plen = torch.zeros(len(h_starts), dtype=torch.int32, device="cuda")
    status = torch.zeros(len(h_starts), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call(max_rounds, paths=True):
        prm = api.GridRouteParams(na, nb, near_r2, near_weight, api.GRID_ROUTE_MAX_COST, max_rounds, max_path, 0)
        kw = dict(starts_ptr=starts.data_ptr(), n_starts=len(h_starts), path_ptr=path.data_ptr(), path_len_ptr=plen.data_ptr(),
                  path_status_ptr=status.data_ptr()) if paths else {}
        ctx.grid_route(blocked.data_ptr(), prm, goals.data_ptr(), 1, workspace_ptr=ws.data_ptr(), cost_ptr=cost.data_ptr(),
                       dist2_ptr=None if dist2 is None else dist2.data_ptr(), next_ptr=nxt.data_ptr(), counts_ptr=cnt.data_ptr(), **kw)

    def timed(max_rounds, paths=True):
        for _ in range(warmup):
            call(max_rounds, paths)
        ctx.profile_select("grid_route")
        for _ in range(5):
            call(max_rounds, paths)
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        return ms / k, [int(v) for v in cnt.cpu()]

    rounds = 64  # the default; a call that does not converge is repeated from the start with four times as many
    while True:
        ms, counts = timed(rounds)
        if counts[4] == 1 or rounds == 4096:
            break
        rounds *= 4
    needed = max(counts[5], 1)
    ms_needed, c_needed = timed(needed)
    ms_more, c_more = timed(min(needed + 64, 4096))
    ms_nopath, _ = timed(needed, paths=False)
    lens = [int(v) for v in plen.cpu().numpy().view(np.uint32)]
    out = {"cells": [na, nb], "near_r2": near_r2, "near_weight": near_weight, "with_dist2": dist2 is not None, "max_rounds": rounds, "ms": ms,
           "counts": counts[:6], "rounds_run": counts[5], "path_lens": lens, "path_status": [int(v) for v in status.cpu()],
           "ms_at_rounds_run": ms_needed, "converged_at_rounds_run": c_needed[4], "ms_at_64_more": ms_more,
           "idle_round_us": 1e3 * (ms_more - ms_needed) / max(min(needed + 64, 4096) - needed, 1),
           "path_launch_us": 1e3 * (ms_needed - ms_nopath), "path_us_per_step": 1e3 * (ms_needed - ms_nopath) / max(max(lens), 1),
           "bound_ms": 1e3 * (n * (1 + 4 + 1 + (4 if dist2 is not None else 0)) + 4 * n) / copy}  # blocked, cost written, next, dist2 read once; NONE memset
    if density is not None:
        out["density"] = density
    t0 = time.perf_counter()
    h_b = blocked.cpu().numpy()
    h_d = None if dist2 is None else dist2.cpu().numpy().view(np.uint32).reshape(na, nb)
    out["d2h_copies_ms"] = 1e3 * (time.perf_counter() - t0)
    if host_detour:
        t0 = time.perf_counter()
        reached = route_host_dijkstra(h_b, h_d, near_r2, near_weight, goal)
        out["host_dijkstra_ms"] = 1e3 * (time.perf_counter() - t0)
        assert reached == counts[1], (reached, counts)
    return out


def route_view(S, torch, ctx, vm, c2w, warmup, copy):
    """Section 13 for one filled map: the route over the clearance (inflation two cells) of section 11's grid."""
    gp = S.api.voxel_grid_default_params(vm.params.voxel_size)
    x, z = float(c2w.reshape(3, 4)[0, 3]), float(c2w.reshape(3, 4)[2, 3])
    gp.origin_a, gp.origin_b = gp.origin_a + z, gp.origin_b + x
    n = gp.na * gp.nb
    ws = torch.empty(4 * n, dtype=torch.int64, device="cuda")
    cls = torch.empty(n, dtype=torch.uint8, device="cuda")
    offsets, d2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    blk = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vm.grid(gp, workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr())
    cp = S.api.grid_clearance_default_params(gp, vm.params.voxel_size)
    cp.inflate_radius = 2.0 * cp.cell_size
    ctx.grid_clearance(cls.data_ptr(), cp, workspace_ptr=offsets.data_ptr(), dist2_ptr=d2.data_ptr(), blocked_ptr=blk.data_ptr())
    ctx.sync()
    return {"route": route_case(S, torch, ctx, blk.reshape(gp.na, gp.nb), d2, 64, 4, warmup, copy, host_detour=True)}


def frontier_random(torch, na, nb, p_unknown, p_obstacle, seed=14):
    """Seeded device arrays: cls drawn per cell, blocked 2 on OBSTACLE cells, cost below 2^20 with a quarter NONE."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    u = torch.rand((na, nb), generator=g, device="cuda")
    cls = torch.where(u < p_unknown, 0, torch.where(u < p_unknown + p_obstacle, 2, 1)).to(torch.uint8)
    blocked = ((cls == 2) * 2).to(torch.uint8)
    cost = torch.randint(0, 1 << 20, (na, nb), generator=g, device="cuda", dtype=torch.int32)
    cost[torch.rand((na, nb), generator=g, device="cuda") < 0.25] = -1
    return cls, blocked, cost


def frontier_serpentine(torch, n):
    """Even rows LEVEL, odd rows UNKNOWN but for one LEVEL connector at alternating ends: one frontier of about n * n / 2 cells."""
    cls = torch.ones((n, n), dtype=torch.uint8, device="cuda")
    cls[1::2] = 0
    cls[1::4, n - 1] = 1
    cls[3::4, 0] = 1
    return cls, None, None


def frontier_case(S, torch, ctx, cls, blocked, cost, warmup, copy, host_detour=False, **tags):
    """Section 14 for one (na, nb) uint8 device class grid, its uint8 device blocked and uint32 device cost (or None each)."""
    api = S.api
    na, nb = cls.shape
    n = na * nb
    prm = api.grid_frontier_default_params(api.GridClearanceParams(na, nb, 4, 64, 0.5, 0.0))
    mf = prm.max_frontiers
    ws = torch.empty(api.grid_frontier_workspace_bytes(na, nb, mf) // 8, dtype=torch.int64, device="cuda")
    rec = torch.empty(6 * mf, dtype=torch.int64, device="cuda")
    goal = torch.empty(mf, dtype=torch.int32, device="cuda")
    label = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call():
        ctx.grid_frontiers(cls.data_ptr(), prm, blocked_ptr=None if blocked is None else blocked.data_ptr(),
                           cost_ptr=None if cost is None else cost.data_ptr(), workspace_ptr=ws.data_ptr(), frontiers_ptr=rec.data_ptr(),
                           goal_cells_ptr=goal.data_ptr(), label_ptr=label.data_ptr(), counts_ptr=cnt.data_ptr())

    def timed(combine):
        ctx.grid_frontier_set_mode(combine)
        for _ in range(warmup):
            call()
        ctx.profile_select("grid_frontier")
        for _ in range(5):
            call()
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        ctx.grid_frontier_set_mode(None)
        return ms / k, [int(v) for v in cnt.cpu()], (rec.cpu().numpy().tobytes(), goal.cpu().numpy().tobytes(), label.cpu().numpy().tobytes())

    ms, counts, bytes_on = timed(True)
    ms_plain, counts_plain, bytes_off = timed(False)
    assert counts == counts_plain and bytes_on[1:] == bytes_off[1:] and bytes_on[0][:48 * counts[5]] == bytes_off[0][:48 * counts[5]]
    largest = int(np.frombuffer(bytes_on[0][:48 * counts[5]], api.GRID_FRONTIER_DTYPE)["size"].max()) if counts[5] else 0
    out = {"cells": [na, nb], "with_blocked": blocked is not None, "with_cost": cost is not None, "min_size": prm.min_size, "max_frontiers": mf, "ms": ms,
           "ms_without_combining": ms_plain, "counts": counts[:7], "largest_written": largest,
           "bound_ms": 1e3 * n * (1 + (1 if blocked is not None else 0) + 8) / copy, **tags}  # cls, blocked, 8 B of labels per cell
    t0 = time.perf_counter()
    h_cls = cls.cpu().numpy()
    h_blk = None if blocked is None else blocked.cpu().numpy()
    h_cost = None if cost is None else cost.cpu().numpy().view(np.uint32).reshape(na, nb)
    out["d2h_copies_ms"] = 1e3 * (time.perf_counter() - t0)
    if host_detour:
        import grid_frontier_ref as F
        t0 = time.perf_counter()
        want = F.frontiers_np(h_cls, h_blk, h_cost, F.Params(na, nb, prm.free_mask, prm.unknown_mask, prm.min_size, mf))
        out["host_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
        assert list(want.counts) == counts[:7], (want.counts, counts)
    return out


def frontier_view(S, torch, ctx, vm, c2w, warmup, copy):
    """Section 14 for one filled map: the frontiers of section 11's grid off section 12's clearance (inflation two cells), with the
    cost of a route from the grid's centre cell."""
    api = S.api
    gp = api.voxel_grid_default_params(vm.params.voxel_size)
    x, z = float(c2w.reshape(3, 4)[0, 3]), float(c2w.reshape(3, 4)[2, 3])
    gp.origin_a, gp.origin_b = gp.origin_a + z, gp.origin_b + x
    na, nb = gp.na, gp.nb
    n = na * nb
    ws = torch.empty(4 * n, dtype=torch.int64, device="cuda")
    cls = torch.empty(n, dtype=torch.uint8, device="cuda")
    offsets, d2, cost = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    blk = torch.empty(n, dtype=torch.uint8, device="cuda")
    goals = torch.tensor([(na // 2) * nb + nb // 2], dtype=torch.int32, device="cuda")
    rws = torch.empty(api.grid_route_workspace_bytes(na, nb) // 8, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    vm.grid(gp, workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr())
    cp = api.grid_clearance_default_params(gp, vm.params.voxel_size)
    cp.inflate_radius = 2.0 * cp.cell_size
    ctx.grid_clearance(cls.data_ptr(), cp, workspace_ptr=offsets.data_ptr(), dist2_ptr=d2.data_ptr(), blocked_ptr=blk.data_ptr())
    rp = api.grid_route_default_params(cp)
    rp.max_rounds = 1024
    ctx.grid_route(blk.data_ptr(), rp, goals.data_ptr(), 1, workspace_ptr=rws.data_ptr(), cost_ptr=cost.data_ptr(), counts_ptr=cnt.data_ptr())
    ctx.sync()
    out = frontier_case(S, torch, ctx, cls.reshape(na, nb), blk.reshape(na, nb), cost.reshape(na, nb), warmup, copy, host_detour=True)
    out["route_counts"] = [int(v) for v in cnt.cpu()[:6]]
    # section 15: the view over that call's goal_cells (all max_frontiers entries, padding included) and that route's cost
    fp = api.grid_frontier_default_params(cp)
    fws = torch.empty(api.grid_frontier_workspace_bytes(na, nb, fp.max_frontiers) // 8, dtype=torch.int64, device="cuda")
    goal = torch.empty(fp.max_frontiers, dtype=torch.int32, device="cuda")
    ctx.grid_frontiers(cls.data_ptr(), fp, blocked_ptr=blk.data_ptr(), cost_ptr=cost.data_ptr(), workspace_ptr=fws.data_ptr(), goal_cells_ptr=goal.data_ptr())
    ctx.sync()
    view = view_case(S, torch, ctx, cls.reshape(na, nb), goal, cost.reshape(na, nb), cp.max_dist, warmup, copy, host_detour=True)
    return {"frontier": out, "view": view}


def view_case(S, torch, ctx, cls, views, cost, max_range, warmup, copy, host_detour=False, sample=8, **tags):
    """Section 15 for one (na, nb) uint8 device class grid, a device list of uint32 view cells and a uint32 device cost (or None)."""
    import grid_view_ref as V
    api = S.api
    na, nb = cls.shape
    n, nv = na * nb, views.numel()
    prm = api.grid_view_default_params(api.GridClearanceParams(na, nb, 4, max_range, 0.5, 0.0))
    ws = torch.empty(api.grid_view_workspace_bytes(na, nb, nv) // 8, dtype=torch.int64, device="cuda")
    rec = torch.empty(4 * nv, dtype=torch.int64, device="cuda")
    order = torch.empty(nv, dtype=torch.int32, device="cuda")
    best = torch.empty(4, dtype=torch.int32, device="cuda")
    seen = torch.empty(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call():
        ctx.grid_view(cls.data_ptr(), views.data_ptr(), nv, prm, cost_ptr=None if cost is None else cost.data_ptr(), workspace_ptr=ws.data_ptr(),
                      records_ptr=rec.data_ptr(), order_ptr=order.data_ptr(), best_ptr=best.data_ptr(), seen_ptr=seen.data_ptr(), counts_ptr=cnt.data_ptr())

    def timed(staged):
        ctx.grid_view_set_mode(staged)
        for _ in range(warmup):
            call()
        ctx.profile_select("grid_view")
        for _ in range(5):
            call()
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        ctx.grid_view_set_mode(None)
        return ms / k, [int(v) for v in cnt.cpu()], tuple(t.cpu().numpy().tobytes() for t in (rec, order, best, seen))

    ms, counts, bytes_on = timed(True)
    ms_plain, counts_plain, bytes_off = timed(False)
    assert counts == counts_plain and bytes_on == bytes_off
    side = 2 * prm.max_range + 1
    out = {"cells": [na, nb], "n_views": nv, "max_range": prm.max_range, "with_cost": cost is not None, "ms": ms, "ms_unstaged": ms_plain,
           "staged_to_unstaged": ms / ms_plain, "counts": counts[:7], "best": [int(v) for v in best.cpu().numpy().view(np.uint32)],
           "bound_ms": 1e3 * (counts[0] * side * side + 32 * nv + 4 * n) / copy, **tags}  # the windows once per used view, the records, seen
    t0 = time.perf_counter()
    h_cls, h_views = cls.cpu().numpy(), views.cpu().numpy().view(np.uint32)
    h_cost = None if cost is None else cost.cpu().numpy().view(np.uint32).reshape(na, nb)
    out["d2h_copies_ms"] = 1e3 * (time.perf_counter() - t0)
    vp = V.Params(na, nb, prm.opaque_mask, prm.gain_mask, prm.max_range, prm.gain_weight, prm.cost_div)
    stats = {}
    if host_detour:
        t0 = time.perf_counter()
        want = V.views_np(h_cls, h_views, h_cost, vp, stats=stats)
        out["host_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
        assert list(want.counts) == counts[:7], (want.counts, counts)
        out["device_to_detour"] = ms / (out["d2h_copies_ms"] + out["host_numpy_ms"])
    else:  # the restatement over the first views only: the steps walked per target
        V.views_np(h_cls, h_views[:sample], h_cost, vp, stats=stats)
        out["steps_sampled_views"] = min(sample, nv)
    out["steps_per_target"] = stats["steps"] / max(stats["targets"], 1)
    return out


def view_synthetic(S, torch, ctx, warmup, copy):
    """Section 15's ranges: one seeded 2048 x 2048 grid, 1024 and 4096 views drawn among its LEVEL cells, max_range 64 and 255."""
    cls, _, cost = frontier_random(torch, 2048, 2048, 0.3, 0.1, seed=15)
    g = torch.Generator(device="cuda")
    g.manual_seed(15)
    level = torch.nonzero(cls.reshape(-1) == 1).reshape(-1)
    out = []
    for nv in (1024, 4096):
        views = level[torch.randint(0, level.numel(), (nv,), generator=g, device="cuda")].to(torch.int32)
        for max_range in (64, 255):
            out.append(view_case(S, torch, ctx, cls, views, cost, max_range, warmup, copy, densities=[0.3, 0.1]))
    return out


def surface_case(S, torch, ctx, cls, top, prm, warmup, copy, host_detour=False, **tags):
    """Section 16 for one (na, nb) device class grid (uint8) and its tops (float32) under a GridSurfaceParams: all four outputs and the
    counts."""
    import grid_surface_ref as G
    api = S.api
    na, nb = cls.shape
    n = na * nb
    cls_out = torch.empty(n, dtype=torch.uint8, device="cuda")
    step, relief = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(2))
    support = torch.empty(n, dtype=torch.int16, device="cuda")
    cnt = torch.zeros(6, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call():
        ctx.grid_surface(cls.data_ptr(), top.data_ptr(), prm, cls_out_ptr=cls_out.data_ptr(), step_ptr=step.data_ptr(), relief_ptr=relief.data_ptr(),
                         support_ptr=support.data_ptr(), counts_ptr=cnt.data_ptr())

    for _ in range(warmup):
        call()
    ctx.profile_select("grid_surface")
    for _ in range(5):
        call()
    ms, k = ctx.profile_read()
    ctx.profile_select("")
    ms /= k
    counts = [int(v) for v in cnt.cpu()]
    rp = G.Params(*(getattr(prm, f) for f, _ in prm._fields_))
    r2 = G.r2_of(rp)
    bound = 1e3 * (5 + 11) * n / copy  # cls and top read once; cls_out, step, relief and support written
    out = {"cells": [na, nb], "r2": r2, "footprint_cells": api.grid_surface_footprint_cells(r2), "ms": ms, "counts": counts, "bound_ms": bound,
           "share_of_bound": bound / ms, "ps_per_cell_and_footprint_cell": 1e9 * ms / n / api.grid_surface_footprint_cells(r2), **tags}
    if host_detour:
        t0 = time.perf_counter()
        h_cls, h_top = cls.cpu().numpy(), top.cpu().numpy()
        out["d2h_copies_ms"] = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        want = G.surface_np(h_cls, h_top, rp)
        out["host_numpy_ms"] = 1e3 * (time.perf_counter() - t0)
        assert list(want.counts) == counts, (want.counts, counts)
        assert np.array_equal(want.cls_out.ravel(), cls_out.cpu().numpy())
        out["device_to_detour"] = ms / (out["d2h_copies_ms"] + out["host_numpy_ms"])
    return out


def surface_view(S, torch, ctx, vm, c2w, warmup, copy):
    """Section 16 for one filled map: the surface of section 11's grid at the defaults."""
    api = S.api
    gp = api.voxel_grid_default_params(vm.params.voxel_size)
    x, z = float(c2w.reshape(3, 4)[0, 3]), float(c2w.reshape(3, 4)[2, 3])
    gp.origin_a, gp.origin_b = gp.origin_a + z, gp.origin_b + x
    na, nb = gp.na, gp.nb
    ws = torch.empty(4 * na * nb, dtype=torch.int64, device="cuda")
    cls = torch.empty(na * nb, dtype=torch.uint8, device="cuda")
    top = torch.empty(na * nb, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    vm.grid(gp, workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr(), top_ptr=top.data_ptr())
    ctx.sync()
    prm = api.grid_surface_default_params(gp, vm.params.voxel_size)
    return {"surface": surface_case(S, torch, ctx, cls.reshape(na, nb), top.reshape(na, nb), prm, warmup, copy, host_detour=True)}


def surface_random(torch, na, nb, seed=16):
    """A seeded class grid and its tops on the device: three low-frequency waves and two cliffs (tests/grid_surface_ref.py's field, made
    here because that one is numpy's), 6 % UNKNOWN (top -inf), 6 % OBSTACLE, 2 % of a class >= 32, 2 % LEVEL with a NaN top."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    rnd = np.random.default_rng(seed)
    ia = torch.arange(na, dtype=torch.float32, device="cuda")[:, None]
    ib = torch.arange(nb, dtype=torch.float32, device="cuda")[None, :]
    top = torch.zeros((na, nb), dtype=torch.float32, device="cuda")
    for _ in range(3):
        fa, fb, ph = rnd.uniform(-0.12, 0.12), rnd.uniform(-0.12, 0.12), rnd.uniform(0, 2 * np.pi)
        top += 0.25 * torch.sin(fa * ia + fb * ib + ph)
    for height in (0.45, 1.0):
        ca, cb, th = rnd.uniform(0, na), rnd.uniform(0, nb), rnd.uniform(0, np.pi)
        top += height * (((ia - ca) * np.cos(th) + (ib - cb) * np.sin(th)) > 0)
    u = torch.rand((na, nb), generator=g, device="cuda")
    cls = torch.ones((na, nb), dtype=torch.uint8, device="cuda")
    cls[u < 0.06] = 0
    top[u < 0.06] = float("-inf")
    cls[(u >= 0.06) & (u < 0.12)] = 2
    cls[(u >= 0.12) & (u < 0.14)] = 77
    top[(u >= 0.14) & (u < 0.16)] = float("nan")
    torch.cuda.synchronize()
    return cls.contiguous(), top.contiguous()


def surface_synthetic(S, torch, ctx, warmup, copy):
    """Section 16's footprints: seeded 2048 x 2048 and 8192 x 2048 grids at r2 = 0, 2, 25 and 225; max_step 0.3, max_relief 0.6,
    min_support_256 200.  The host detour is taken on the smaller grid up to r2 = 25 (the restatement makes one pass per footprint
    cell: 709 passes over 4 or 16 million cells were not waited for)."""
    import grid_surface_ref as G
    out = []
    for na, nb in ((2048, 2048), (8192, 2048)):
        cls, top = surface_random(torch, na, nb)
        for r2 in (0, 2, 25, 225):
            prm = S.api.GridSurfaceParams(na, nb, 1 << 1, 0.5, 0.3, G.radius_for(r2), 0.6, 200)
            out.append(surface_case(S, torch, ctx, cls, top, prm, warmup, copy, host_detour=na == 2048 and r2 <= 25))
        del cls, top
    return out


def surface_line(k):
    """Section 16's line of the text report for one surface_case."""
    line = (f"r2 {k['r2']} (D = {k['footprint_cells']}; the counts' memset + one launch, all four outputs, mean of 5): {1e3 * k['ms']:.1f} us, counts {k['counts']} "
            f"(ground, step, rough, unsupported, nonfinite, kept); 5 B read + 11 B written per cell at hbm_copy {1e3 * k['bound_ms']:.2f} us -> "
            f"{100 * k['share_of_bound']:.1f} % of that bound; {k['ps_per_cell_and_footprint_cell']:.2f} ps per cell and footprint cell")
    if "host_numpy_ms" in k:
        line += (f"; device-to-host copies of cls and top {1e3 * k['d2h_copies_ms']:.0f} us and the restatement's numpy route on the host {k['host_numpy_ms']:.0f} ms: "
                 f"device / detour {k['device_to_detour']:.6f}")
    return line + "\n"


WAYPOINT_LOOKS = (16, 64, 255)


def waypoint_case(S, torch, ctx, blocked, starts, warmup, one_path=False, host_detour=False, **tags):
    """Section 17 for one (na, nb) uint8 device grid (passable iff 0): the route from `starts` to the centre cell, then the waypoints of
    its paths at each max_look.  one_path: of the starts only the one with the longest complete path is used."""
    import grid_waypoints_ref as G
    api = S.api
    na, nb = blocked.shape
    n = na * nb
    ns, max_path, max_way = len(starts), 4096, 256
    goals = torch.tensor([(na // 2) * nb + nb // 2], dtype=torch.int32, device="cuda")
    d_starts = torch.from_numpy(np.asarray(starts, np.uint32).view(np.int32)).cuda()
    ws = torch.empty(api.grid_route_workspace_bytes(na, nb) // 8, dtype=torch.int64, device="cuda")
    cost = torch.empty(n, dtype=torch.int32, device="cuda")
    path = torch.empty(ns * max_path, dtype=torch.int32, device="cuda")
    plen = torch.zeros(ns, dtype=torch.int32, device="cuda")
    status = torch.zeros(ns, dtype=torch.uint8, device="cuda")
    rcnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    rounds = 64
    while True:  # a call that does not converge is repeated from the start with four times as many rounds
        ctx.grid_route(blocked.data_ptr(), api.GridRouteParams(na, nb, 0, 0, api.GRID_ROUTE_MAX_COST, rounds, max_path, 0), goals.data_ptr(), 1,
                       workspace_ptr=ws.data_ptr(), cost_ptr=cost.data_ptr(), starts_ptr=d_starts.data_ptr(), n_starts=ns, path_ptr=path.data_ptr(),
                       path_len_ptr=plen.data_ptr(), path_status_ptr=status.data_ptr(), counts_ptr=rcnt.data_ptr())
        ctx.sync()
        if int(rcnt.cpu()[4]) == 1 or rounds == 4096:
            break
        rounds *= 4
    lens, stat = plen.cpu().numpy().view(np.uint32), status.cpu().numpy()
    row, n_paths = 0, ns
    if one_path:
        ok = np.flatnonzero(stat == 0)
        if len(ok) == 0:
            return {"cells": [na, nb], "no_path": True, "path_status": stat.tolist(), **tags}
        row, n_paths = int(ok[np.argmax(lens[ok])]), 1
    way, index = (torch.empty(n_paths * max_way, dtype=torch.int32, device="cuda") for _ in range(2))
    wlen = torch.zeros(n_paths, dtype=torch.int32, device="cuda")
    wstat = torch.zeros(n_paths, dtype=torch.uint8, device="cuda")
    length = torch.zeros(n_paths, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    out = {"cells": [na, nb], "n_paths": n_paths, "path_cells": int(lens[row]) if one_path else int(lens.sum()), "route_rounds": rounds, "looks": [], **tags}
    for look in WAYPOINT_LOOKS:
        prm = api.GridWaypointParams(na, nb, max_path, look, 0, max_way, 0.5)

        def call():
            ctx.grid_waypoints(blocked.data_ptr(), path.data_ptr() + 4 * row * max_path, plen.data_ptr() + 4 * row, n_paths, prm,
                               path_status_ptr=status.data_ptr() + row, way_ptr=way.data_ptr(), way_index_ptr=index.data_ptr(), way_len_ptr=wlen.data_ptr(),
                               way_status_ptr=wstat.data_ptr(), length_ptr=length.data_ptr(), counts_ptr=cnt.data_ptr())

        for _ in range(warmup):
            call()
        ctx.profile_select("grid_waypoints")
        for _ in range(5):
            call()
        ms, calls = ctx.profile_read()
        ctx.profile_select("")
        k = {"max_look": look, "us": 1e3 * ms / calls}
        k["counts"] = [int(v) for v in cnt.cpu()[:7]]
        if host_detour and look <= 64:
            t0 = time.perf_counter()
            h_path = path.cpu().numpy().view(np.uint32).reshape(ns, max_path)[row:row + n_paths]
            h_len, h_stat, h_b = lens[row:row + n_paths].copy(), status.cpu().numpy()[row:row + n_paths], blocked.cpu().numpy()
            k["d2h_copies_ms"] = 1e3 * (time.perf_counter() - t0)
            t0 = time.perf_counter()
            want = G.waypoints_py(h_b, None, h_path, h_len, h_stat, G.Params(na, nb, max_path, look, 0, max_way, 0.5))
            k["host_python_ms"] = 1e3 * (time.perf_counter() - t0)
            assert list(want.counts) == k["counts"], (want.counts, k["counts"])
            assert np.array_equal(want.way_len, wlen.cpu().numpy().view(np.uint32)) and want.length.tobytes() == length.cpu().numpy().tobytes()
        out["looks"].append(k)
    return out


def waypoint_view(S, torch, ctx, vm, c2w, warmup, copy):
    """Section 17 for one filled map: the waypoints of the route over the clearance (inflation two cells) of section 11's grid."""
    gp = S.api.voxel_grid_default_params(vm.params.voxel_size)
    x, z = float(c2w.reshape(3, 4)[0, 3]), float(c2w.reshape(3, 4)[2, 3])
    gp.origin_a, gp.origin_b = gp.origin_a + z, gp.origin_b + x
    n = gp.na * gp.nb
    ws = torch.empty(4 * n, dtype=torch.int64, device="cuda")
    cls = torch.empty(n, dtype=torch.uint8, device="cuda")
    offsets, d2 = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    blk = torch.empty(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    vm.grid(gp, workspace_ptr=ws.data_ptr(), cls_ptr=cls.data_ptr())
    cp = S.api.grid_clearance_default_params(gp, vm.params.voxel_size)
    cp.inflate_radius = 2.0 * cp.cell_size
    ctx.grid_clearance(cls.data_ptr(), cp, workspace_ptr=offsets.data_ptr(), dist2_ptr=d2.data_ptr(), blocked_ptr=blk.data_ptr())
    ctx.sync()
    corners = [0, gp.nb - 1, (gp.na - 1) * gp.nb, n - 1]
    return {"waypoints": waypoint_case(S, torch, ctx, blk.reshape(gp.na, gp.nb), corners, warmup, one_path=True, host_detour=True)}


def waypoint_synthetic(S, torch, ctx, warmup):
    """Section 17's seeded grid: 2048 x 2048, blocked density 0.1, from one corner and from 4,096 seeded starts."""
    na = nb = 2048
    blocked = route_random(torch, na, nb, 0.1, seed=17)
    starts = np.random.default_rng(17).integers(0, na * nb, 4096)
    return [waypoint_case(S, torch, ctx, blocked, [0, nb - 1, (na - 1) * nb, na * nb - 1], warmup, one_path=True, host_detour=True, density=0.1),
            waypoint_case(S, torch, ctx, blocked, starts, warmup, density=0.1)]


def waypoint_line(k):
    """Section 17's lines of the text report for one waypoint_case."""
    if k.get("no_path"):
        return f"no corner has a path to the centre cell (status {k['path_status']})\n"
    line = f"{k['n_paths']} path(s) of {k['path_cells']} cells in all (the counts' memset + one launch, all five outputs, mean of 5):\n"
    for q in k["looks"]:
        line += (f"    max_look {q['max_look']}: {q['us']:.1f} us"
                 f"; counts {q['counts']} (used, skipped, cells in, waypoints, forced, full, max_d2)")
        if "host_python_ms" in q:
            line += (f"; device-to-host copies of path, path_len, path_status and blocked {1e3 * q['d2h_copies_ms']:.0f} us and the restatement's Python walk "
                     f"on the host {q['host_python_ms']:.0f} ms")
        line += "\n"
    return line


def render_view(S, torch, ctx, cam, vm, c2w, warmup, copy):
    """Section 9 for one filled map: what it shows a camera at the last cloud's pose."""
    w2c = np.linalg.inv(np.vstack([c2w.reshape(3, 4), [0, 0, 0, 1]]))[:3].reshape(12)
    ws = torch.empty(W * H, dtype=torch.int32, device="cuda")
    dd = torch.empty(W * H, dtype=torch.int16, device="cuda")
    gg = torch.empty(W * H, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def timed(max_radius, coop=True, pre=False):
        vm.render_set_mode(coop, pre)
        kw = dict(w2c12=w2c, max_radius=max_radius, workspace_ptr=ws.data_ptr(), disp_ptr=dd.data_ptr(), intensity_ptr=gg.data_ptr(),
                  counts_ptr=cnt.data_ptr())
        for _ in range(warmup):
            vm.render(W, H, cam, **kw)
        ctx.profile_select("voxel_render")
        for _ in range(5):
            vm.render(W, H, cam, **kw)
        ms, k = ctx.profile_read()
        ctx.profile_select("")
        vm.render_set_mode()  # back to the defaults
        return ms / k, [int(v) for v in cnt.cpu()], dd.cpu().numpy().tobytes(), gg.cpu().numpy().tobytes()

    prm = S.api.voxel_render_default_params()
    out = {}
    for name, radius in (("render", prm.max_radius), ("render_r0", 0)):
        ms, counts, _, _ = timed(radius)
        bound = 1e3 * (8 * vm.capacity + 32 * counts[0] + 11 * W * H) / copy
        out.update({name + "_ms": ms, name + "_counts": counts, name + "_bound_ms": bound, name + "_share_of_bound": bound / ms})
    ref = timed(prm.max_radius)
    modes = {}
    for coop, pre in ((True, True), (True, False), (False, True), (False, False)):
        got = timed(prm.max_radius, coop, pre)
        modes[("cooperative" if coop else "own lane") + (", pre-check" if pre else ", no pre-check")] = got[0]
        assert got[1:] == ref[1:], "a drawing mode changed the render"
    out.update({"render_max_radius": prm.max_radius, "render_modes_ms": modes})
    return out


def carve_and_copy(S, torch, ctx, cam, dm, vm, c2w, warmup, copy):
    """Section 8 for one filled map: the copy into a cleared map of the same shape, then the carve with the last map of the batch."""
    live = vm.stats()["n_voxels"]  # nothing was carved yet: every claimed slot is live
    dst = S.VoxelMap(ctx, voxel_size=vm.params.voxel_size, capacity_log2=vm.params.capacity_log2)
    for _ in range(warmup):
        dst.clear()
        vm.copy_live_to(dst)
    dst.clear()
    ctx.profile_select("voxel_copy")
    vm.copy_live_to(dst)
    copy_ms, _ = ctx.profile_read()
    ctx.profile_select("")
    copied = dst.stats()
    dst.close()
    w2c = np.linalg.inv(np.vstack([c2w.reshape(3, 4), [0, 0, 0, 1]]))[:3].reshape(12)
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    last = dm[dm.shape[0] - 1]
    for _ in range(warmup):
        vm.carve(last.data_ptr(), W, H, cam, w2c12=w2c, keep_count=1, counts_ptr=cnt.data_ptr())
    ctx.profile_select("voxel_carve")
    for _ in range(5):
        vm.carve(last.data_ptr(), W, H, cam, w2c12=w2c, keep_count=1, counts_ptr=cnt.data_ptr())
    dry_ms, k = ctx.profile_read()
    dry = [int(v) for v in cnt.cpu()]
    ctx.profile_select("voxel_carve")
    vm.carve(last.data_ptr(), W, H, cam, w2c12=w2c, counts_ptr=cnt.data_ptr())
    carve_ms, _ = ctx.profile_read()
    ctx.profile_select("")
    real = [int(v) for v in cnt.cpu()]
    carve_bound = 1e3 * (8 * vm.capacity + 32 * live) / copy
    copy_bound = 1e3 * (8 * vm.capacity + 32 * live + 40 * copied["n_voxels"]) / copy
    return {"live_slots": live, "copy_ms": copy_ms, "copy_stats": copied, "copy_bound_ms": copy_bound, "copy_share_of_bound": copy_bound / copy_ms,
            "carve_dry_ms": dry_ms / k, "carve_dry_counts": dry, "carve_ms": carve_ms, "carve_counts": real, "carve_bound_ms": carve_bound,
            "carve_dry_share_of_bound": carve_bound / (dry_ms / k), "carve_share_of_bound": carve_bound / carve_ms}


LEDGER_HELD = 4
LEDGER_DELTA = np.array([0.0, 0.0, 0.5 * np.deg2rad(0.1), 0.0, 0.01, 0.0, 0.0])  # pose7: 0.1 degrees about y and 1 cm


def grouped(S, torch, lanes, n_groups, frames, warmup, steps, rounds, step_px, ledger_only=False):
    from stereo_vo_amd import api
    bench.group_lines(n_groups)
    seeds = [0x5EED0001 + i for i in range(lanes)]
    groups = [bench._Group(S, torch, 0, seeds[gi::n_groups], frames) for gi in range(n_groups)]
    torch.cuda.synchronize()
    prm = api.CloudParams(step_px, 0.0, ((W + step_px - 1) // step_px) * ((H + step_px - 1) // step_px))

    import ctypes as C
    lane_maps = [None] * n_groups  # one map per lane, made on first use; never cleared: every step replays the same frames

    def insert_clouds(gi, g, carve=False):  # every keyframe cloud of the last call into its lane's map, from the table's device pointers
        if lane_maps[gi] is None:
            lane_maps[gi] = [S.VoxelMap(g.ctx, capacity_log2=VOXEL_LANE_LOG2) for _ in range(g.pipe.n_lanes)]
        n, tab = C.c_int(0), C.POINTER(api.KeyframeCloud)()
        g.ctx._chk(g.pipe.L.svo_pipeline_group_keyframe_clouds(g.pipe.h, C.byref(n), C.byref(tab)), "svo_pipeline_group_keyframe_clouds")
        for i in range(n.value):
            e = tab[i]
            q = list(g.all_res[e.lane][e.frame].pose7)
            q = q if any(q[:4]) else [1, 0, 0, 0, 0, 0, 0]
            if carve:  # the keyframe's own map first carves what the earlier keyframes left in its view (defaults)
                lane_maps[gi][e.lane].carve(g.pipe.keyframe_disparity(i), W, H, g.pipe.prm.cam, pose7=q)
            lane_maps[gi][e.lane].insert(e.dev, e.n_stored, pose7=q)

    lane_ledgers = [None] * n_groups  # per lane: its own map, a ledger on it, and what the ledger holds as [id, pose7, moved?]

    def ledger_clouds(gi, g):  # the ledger loop of INTEGRATION 4a: retire the oldest of four, insert the new, then move every held one
        if lane_ledgers[gi] is None:
            maps = [S.VoxelMap(g.ctx, capacity_log2=VOXEL_LANE_LOG2) for _ in range(g.pipe.n_lanes)]
            lane_ledgers[gi] = [{"map": m, "led": S.VoxelLedger(m, LEDGER_HELD, prm.max_points), "held": [], "next": 0} for m in maps]
        n, tab = C.c_int(0), C.POINTER(api.KeyframeCloud)()
        g.ctx._chk(g.pipe.L.svo_pipeline_group_keyframe_clouds(g.pipe.h, C.byref(n), C.byref(tab)), "svo_pipeline_group_keyframe_clouds")
        for i in range(n.value):
            e = tab[i]
            q = list(g.all_res[e.lane][e.frame].pose7)
            q = np.array(q if any(q[:4]) else [1, 0, 0, 0, 0, 0, 0], np.float64)
            st = lane_ledgers[gi][e.lane]
            if len(st["held"]) == LEDGER_HELD:
                st["led"].retire(st["held"].pop(0)[0])
            st["led"].insert(st["next"], e.dev, e.n_stored, q)
            st["held"].append([st["next"], q, False])
            st["next"] += 1
        for st in lane_ledgers[gi]:
            for h in st["held"]:  # there and back in turn: every update moves the cloud
                h[2] = not h[2]
                st["led"].update(h[0], h[1] + LEDGER_DELTA if h[2] else h[1])

    def run(k, voxel=False, carve=False, ledger=False):
        def work(gi, g):
            for _ in range(k):
                g.step()
                if voxel:
                    insert_clouds(gi, g, carve)
                if ledger:
                    ledger_clouds(gi, g)
        bench.run_threads([lambda gi=gi, g=g: work(gi, g) for gi, g in enumerate(groups)])

    def table_len(pipe):  # entries of the last call's table (no point is copied)
        import ctypes as C
        n, tab = C.c_int(0), C.c_void_p()
        pipe.ctx._chk(pipe.L.svo_pipeline_group_keyframe_clouds(pipe.h, C.byref(n), C.byref(tab)), "svo_pipeline_group_keyframe_clouds")
        return n.value

    def timed(on, speckle=False, lr=False, sgm=False, voxel=False, carve=False, ledger=False):
        for g in groups:
            g.pipe.set_keyframe_clouds(-1, prm if on else None)
            if on:
                g.pipe.set_keyframe_speckle_filter(SPECKLE_SIZES[0] if speckle else None, SPECKLE_DIFF)
                g.pipe.set_keyframe_lr_check(LR_DIFF if lr else None)
                g.pipe.set_keyframe_sgm(on=sgm)
            g.clear_counters()
        run(warmup, voxel, carve, ledger)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(steps, voxel, carve, ledger)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        kf = sum(table_len(g.pipe) for g in groups) if on else 0  # of the last step
        return lanes * frames * steps / dt, 1e3 * dt / steps, kf

    plain, cloud, filt, chk, sg, vox, crv, led = [], [], [], [], [], [], [], []

    def ledger_result():
        held = sum(len(st["held"]) for sts in lane_ledgers if sts for st in sts)
        lstats = {k: sum(st["map"].stats()[k] for sts in lane_ledgers if sts for st in sts) for k in ("n_voxels", "n_inserted", "n_rejected", "n_dropped")}
        for sts in lane_ledgers:
            for st in sts or []:
                st["led"].close()
                st["map"].close()
        return {"lanes": lanes, "groups": n_groups, "frames_per_step_per_lane": frames, "steps": steps, "rounds": rounds, "cloud_step": step_px,
                "ledger_held_per_lane": LEDGER_HELD, "ledger_held_at_the_end": held, "ledger_totals_over_all_lane_maps": lstats,
                "frames_per_s_clouds": float(np.median([x[0] for x in cloud])), "step_ms_clouds": float(np.median([x[1] for x in cloud])),
                "all_clouds": [x[0] for x in cloud], "frames_per_s_clouds_ledger": float(np.median([x[0] for x in led])),
                "step_ms_clouds_ledger": float(np.median([x[1] for x in led])), "all_clouds_ledger": [x[0] for x in led],
                "ratio_ledger_to_clouds": float(np.median([x[0] for x in led])) / float(np.median([x[0] for x in cloud])),
                "round_ratios_ledger_to_clouds": [b[0] / a[0] for a, b in zip(cloud, led)]}

    if ledger_only:
        for _ in range(rounds):
            cloud.append(timed(True))
            led.append(timed(True, ledger=True))
            print(f"bench_dense: ledger round {len(led)} of {rounds} done", file=sys.stderr, flush=True)
        out = ledger_result()
        for g in groups:
            g.close()
        return out
    for _ in range(rounds):  # alternating: other people's work shares the host
        plain.append(timed(False))
        cloud.append(timed(True))
        led.append(timed(True, ledger=True))
        filt.append(timed(True, True))
        chk.append(timed(True, False, True))
        sg.append(timed(True, sgm=True))
        vox.append(timed(True, voxel=True))
        crv.append(timed(True, voxel=True, carve=True))
        print(f"bench_dense: round {len(crv)} of {rounds} done", file=sys.stderr, flush=True)
    vstats = {k: sum(m.stats()[k] for ms in lane_maps if ms for m in ms) for k in ("n_voxels", "n_inserted", "n_rejected", "n_dropped")}
    for ms in lane_maps:
        for m in ms or []:
            m.close()
    ledger = ledger_result()  # reads the lane maps' counters and closes them: before their contexts go
    for g in groups:
        g.close()
    med = lambda xs: float(np.median(xs))
    fp, fc, ff, fl = med([x[0] for x in plain]), med([x[0] for x in cloud]), med([x[0] for x in filt]), med([x[0] for x in chk])
    return {"lanes": lanes, "groups": n_groups, "frames_per_step_per_lane": frames, "steps": steps, "rounds": rounds, "cloud_step": step_px,
            "frames_per_s_plain": fp, "frames_per_s_clouds": fc, "ratio": fc / fp,
            "step_ms_plain": med([x[1] for x in plain]), "step_ms_clouds": med([x[1] for x in cloud]),
            "keyframes_in_last_step": [x[2] for x in cloud],
            "all_plain": [x[0] for x in plain], "all_clouds": [x[0] for x in cloud],
            "speckle_max_size": SPECKLE_SIZES[0], "speckle_max_diff16": SPECKLE_DIFF, "frames_per_s_clouds_speckle": ff,
            "ratio_speckle_to_clouds": ff / fc, "step_ms_clouds_speckle": med([x[1] for x in filt]), "all_clouds_speckle": [x[0] for x in filt],
            "lr_max_diff16": LR_DIFF, "frames_per_s_clouds_lr_check": fl, "ratio_lr_check_to_clouds": fl / fc,
            "step_ms_clouds_lr_check": med([x[1] for x in chk]), "all_clouds_lr_check": [x[0] for x in chk],
            "round_ratios_lr_check_to_clouds": [b[0] / a[0] for a, b in zip(cloud, chk)],
            "frames_per_s_clouds_sgm": med([x[0] for x in sg]), "ratio_sgm_to_clouds": med([x[0] for x in sg]) / fc,
            "step_ms_clouds_sgm": med([x[1] for x in sg]), "all_clouds_sgm": [x[0] for x in sg],
            "round_ratios_sgm_to_clouds": [b[0] / a[0] for a, b in zip(cloud, sg)],
            "frames_per_s_clouds_voxel": med([x[0] for x in vox]), "ratio_voxel_to_clouds": med([x[0] for x in vox]) / fc,
            "step_ms_clouds_voxel": med([x[1] for x in vox]), "all_clouds_voxel": [x[0] for x in vox],
            "round_ratios_voxel_to_clouds": [b[0] / a[0] for a, b in zip(cloud, vox)], "voxel_lane_log2": VOXEL_LANE_LOG2,
            "voxel_totals_over_all_lane_maps": vstats,
            "frames_per_s_clouds_voxel_carve": med([x[0] for x in crv]), "ratio_carve_to_voxel": med([x[0] for x in crv]) / med([x[0] for x in vox]),
            "step_ms_clouds_voxel_carve": med([x[1] for x in crv]), "all_clouds_voxel_carve": [x[0] for x in crv],
            "round_ratios_carve_to_voxel": [b[0] / a[0] for a, b in zip(vox, crv)],
            **{k: v for k, v in ledger.items() if "ledger" in k}}


def view_line(k):
    """Section 15's line of the text report for one view_case."""
    line = (f"{k['n_views']} views, max_range {k['max_range']} (two memsets + cast + rank, mean of 5): {1e3 * k['ms']:.1f} us staged in LDS, "
            f"{1e3 * k['ms_unstaged']:.1f} us with every step reading cls (the same bytes): staged / unstaged {k['staged_to_unstaged']:.3f}; counts {k['counts']} "
            f"(used, ignored, in range, visible, gain, covered, gain covered), best {k['best']} (cell, index, score, gain), "
            f"{k['steps_per_target']:.2f} steps walked per target in range (restatement")
    line += f", the first {k['steps_sampled_views']} views)" if "steps_sampled_views" in k else ")"
    line += f"; the windows once per used view + records + seen at hbm_copy {1e3 * k['bound_ms']:.2f} us; device-to-host copies of cls, views and cost {1e3 * k['d2h_copies_ms']:.0f} us"
    if "host_numpy_ms" in k:
        line += f" and the restatement's numpy route on the host {k['host_numpy_ms']:.0f} ms: device / detour {k['device_to_detour']:.5f}"
    return line + "\n"


def api_sub():
    from stereo_vo_amd import api
    return api.SGM_KEYFRAME_SUB_BATCH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lanes", type=int, default=96)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cloud-step", type=int, default=4)
    ap.add_argument("--skip-groups", action="store_true")
    ap.add_argument("--ledger-only", action="store_true", help="of the 96-lane loads only clouds alone and clouds with the ledger loop")
    ap.add_argument("--surface-only", action="store_true", help="section 16's seeded grids alone")
    ap.add_argument("--waypoints-only", action="store_true", help="section 17's seeded grid alone")
    ap.add_argument("--align-only", action="store_true", help="section 7's fill and sections 10, 18, 19, 20, 21, 22 and 23 alone")
    ap.add_argument("--route-only", action="store_true", help="section 7's fill and section 23 alone")
    ap.add_argument("--out", help="write the text report here as well")
    a = ap.parse_args()
    import torch
    import stereo_vo_amd as S
    if not torch.cuda.is_available():
        sys.exit("bench_dense: needs the GPU (nothing is measured without it)")
    if a.surface_only:
        ctx = S.Context(W, H, max_batch=1, max_corners=64, max_candidates=1 << 12, max_features=64)
        copy = ctx.measure_peak("hbm_copy")
        res = {"hbm_copy_bytes_per_s": copy, "surface_synthetic": surface_synthetic(S, torch, ctx, 3, copy)}
        ctx.close()
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                for k in res["surface_synthetic"]:
                    f.write(f"surface of a synthetic {k['cells'][0]} x {k['cells'][1]} grid: " + surface_line(k))
        return
    if a.waypoints_only:
        ctx = S.Context(W, H, max_batch=1, max_corners=64, max_candidates=1 << 12, max_features=64)
        res = {"waypoint_synthetic": waypoint_synthetic(S, torch, ctx, 3)}
        ctx.close()
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                for k in res["waypoint_synthetic"]:
                    f.write(f"waypoints over a synthetic {k['cells'][0]} x {k['cells'][1]} grid, blocked density {k['density']}: " + waypoint_line(k))
        return
    if a.route_only:
        ctx = S.Context(W, H, max_batch=a.batch, max_corners=64, max_candidates=1 << 12, max_features=64)
        p = S.synth_default(W, H)
        cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
        pairs = [S.synth_render(p, i) for i in range(a.batch)]
        dl = torch.from_numpy(np.stack([x[0] for x in pairs])).cuda()
        dr = torch.from_numpy(np.stack([x[1] for x in pairs])).cuda()
        dm = torch.empty((a.batch, H, W), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        copy = ctx.measure_peak("hbm_copy")
        ctx.stereo_bm_batch(dl.data_ptr(), dr.data_ptr(), a.batch, W, H, W, W * H, dm.data_ptr(), NDISP, BLOCK)
        ctx.sync()
        res = {"hbm_copy_bytes_per_s": copy, "voxel": voxel(S, torch, ctx, cam, dm, dl, a.batch, 3, copy, only_route=True)}
        ctx.close()
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                for c in res["voxel"]:
                    f.write(f"voxel map, clouds at step {c['cloud_step']} ({c['points_per_cloud']:.0f} points per cloud), voxel {c['voxel_size']} m, 2^{c['capacity_log2']} slots, "
                            f"{c['stats_after_fresh']['n_voxels']} voxels, load {c['load']:.3f}:\n  " + voxel_route_line(c['voxel_route']))
        return
    if a.align_only:
        ctx = S.Context(W, H, max_batch=a.batch, max_corners=64, max_candidates=1 << 12, max_features=64)
        p = S.synth_default(W, H)
        cam = S.CameraInfo(p.focal, p.cx, p.cy, 0, 0, 0, 0, p.baseline)
        pairs = [S.synth_render(p, i) for i in range(a.batch)]
        dl = torch.from_numpy(np.stack([x[0] for x in pairs])).cuda()
        dr = torch.from_numpy(np.stack([x[1] for x in pairs])).cuda()
        dm = torch.empty((a.batch, H, W), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        copy = ctx.measure_peak("hbm_copy")
        ctx.stereo_bm_batch(dl.data_ptr(), dr.data_ptr(), a.batch, W, H, W, W * H, dm.data_ptr(), NDISP, BLOCK)
        ctx.sync()
        res = {"hbm_copy_bytes_per_s": copy, "voxel": voxel(S, torch, ctx, cam, dm, dl, a.batch, 3, copy, only_align=True)}
        ctx.close()
        print(json.dumps(res))
        if a.out:
            with open(a.out, "w") as f:
                for c in res["voxel"]:
                    f.write(f"voxel map, clouds at step {c['cloud_step']} ({c['points_per_cloud']:.0f} points per cloud), voxel {c['voxel_size']} m, 2^{c['capacity_log2']} slots, "
                            f"{c['stats_after_fresh']['n_voxels']} voxels, load {c['load']:.3f}:\n  align: " + align_line(c['align'], c['insert_ms']) +
                            "  normals: " + normals_line(c['normals'], c['align'], c['insert_ms']) + "  locate: " + locate_line(c['locate'], c['align']) + "  sight lines: " + rays_line(c['rays']) +
                            "  " + distance_line(c['distance']) + "  " + voxel_route_line(c['voxel_route']))
        return
    res = {"standalone": standalone(S, torch, a.batch, 3, a.reps)}
    print("bench_dense: standalone sections done", file=sys.stderr, flush=True)
    if not a.skip_groups:
        res["pipeline_groups"] = grouped(S, torch, a.lanes, a.groups, a.frames, a.warmup, a.steps, a.rounds, a.cloud_step, a.ledger_only)
    try:
        res["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        res["commit"] = None
    print(json.dumps(res))
    if a.out:
        s, g = res["standalone"], res.get("pipeline_groups")
        with open(a.out, "w") as f:
            f.write(f"dense map, {W} x {H}, StereoBM({NDISP}, {BLOCK}), HIP events:\n"
                    f"  stereo_dense_batch_kernel, {s['batch']} pairs per launch: {s['fused_ms_per_pair']:.4f} ms per pair (mean of {s['fused_launches_timed']} launches)\n"
                    f"  the three launches inside svo_stereo_bm, one pair per call: {s['three_launch_ms_per_pair']:.4f} ms per pair "
                    f"(mean of {s['three_launch_calls_timed']} calls); ratio fused / three-launch {s['fused_ms_per_pair'] / s['three_launch_ms_per_pair']:.3f}; "
                    f"maps identical: {s['fused_equals_three_launch']}\n")
            for c in s["cloud"]:
                f.write(f"cloud (count + scan + write), step {c['step']}: {c['ms_per_pair']:.4f} ms per pair, {c['kept_per_pair']:.0f} points kept per pair, "
                        f"{c['algorithmic_bytes_per_pair'] / 1e6:.3f} MB per pair -> {c['bytes_per_s'] / 1e12:.3f} TB/s "
                        f"({100 * c['share_of_copy_rate']:.1f} % of svo_measure_peak(hbm_copy) = {s['hbm_copy_bytes_per_s'] / 1e12:.3f} TB/s, same run)\n")
            for c in s["speckle"]:
                f.write(f"speckle filter (tile + seam + count + apply), max_size {c['max_size']}, max_diff16 {c['max_diff16']}: {c['ms_per_pair']:.4f} ms per pair "
                        f"(mean of {c['sequences_timed']} sequences of {s['batch']} maps), {c['removed_per_pair']:.0f} of {c['valid_per_pair']:.0f} valid pixels removed per pair; "
                        f"{c['ratio_to_fused_dense']:.3f} x the fused dense launch; 19 A = {c['budget_bytes_per_pair'] / 1e6:.3f} MB per pair -> "
                        f"{c['bytes_per_s'] / 1e12:.3f} TB/s ({100 * c['share_of_copy_rate']:.1f} % of hbm_copy, same run)\n")
            c = s["lr_check"]
            f.write(f"left-right check, max_diff16 {c['max_diff16']}: cost form of the fused dense launch {c['cost_ms_per_pair']:.4f} ms per pair beside the plain form "
                    f"{c['plain_ms_per_pair']:.4f} (medians of 3 alternating blocks of {c['launches_per_block']} launches; plain {[round(x, 4) for x in c['all_plain_ms']]}, "
                    f"cost {[round(x, 4) for x in c['all_cost_ms']]}): ratio {c['ratio_cost_to_plain']:.3f}; maps identical: {c['cost_map_equals_plain_map']}\n"
                    f"  the check (one launch): {1e3 * c['check_ms_per_pair']:.1f} us per pair (mean of {c['calls_timed']} calls of {s['batch']} maps), "
                    f"{c['removed_per_pair']:.0f} of {c['valid_per_pair']:.0f} valid pixels removed per pair; {c['ratio_to_fused_dense']:.3f} x the fused dense launch; "
                    f"4 A = {c['budget_bytes_per_pair'] / 1e6:.3f} MB per pair -> {c['bytes_per_s'] / 1e12:.3f} TB/s ({100 * c['share_of_copy_rate']:.1f} % of hbm_copy, same run)\n")
            c = s["sgm"]
            f.write(f"semi-global matching, p1 {c['p1']}, p2 {c['p2']} (fill + volume + four paths, with the cost form): {c['sgm_ms_per_pair']:.4f} ms per pair beside the plain "
                    f"fused dense launch {c['plain_ms_per_pair']:.4f} (medians of 3 alternating blocks of {c['sequences_per_block']}; plain "
                    f"{[round(x, 4) for x in c['all_plain_ms']]}, sgm {[round(x, 4) for x in c['all_sgm_ms']]}): {c['ratio_to_fused_dense']:.2f} x the fused dense launch\n"
                    f"  bytes counted from the code: {c['bytes_per_pair'] / 1e6:.1f} MB per pair (work space {c['workspace_bytes_per_pair'] / 1e6:.1f} MB per pair) -> "
                    f"{c['bytes_per_s'] / 1e12:.3f} TB/s = {100 * c['share_of_copy_rate']:.1f} % of hbm_copy, same run (the byte bound is {c['bound_ms_per_pair']:.4f} ms per pair); "
                    f"valid pixels per pair {c['valid_per_pair_sgm']:.0f} against block matching's {c['valid_per_pair_bm']:.0f}\n")
            for c in s["voxel"]:
                f.write(f"voxel map, clouds at step {c['cloud_step']} ({c['points_per_cloud']:.0f} points per cloud), voxel {c['voxel_size']} m, 2^{c['capacity_log2']} slots: insert "
                        f"{1e3 * c['fresh_ms_per_cloud']:.1f} us per cloud into the cleared map, {1e3 * c['again_ms_per_cloud']:.1f} us again into the filled one (medians of 3 "
                        f"alternating blocks of {s['batch']} clouds; fresh {[round(1e3 * x, 1) for x in c['all_fresh_ms']]}, again {[round(1e3 * x, 1) for x in c['all_again_ms']]}); "
                        f"16 B per point at hbm_copy {1e3 * c['record_bytes_bound_ms']:.2f} us -> {100 * c['fresh_share_of_bound']:.1f} % / {100 * c['again_share_of_bound']:.1f} % "
                        f"of the byte bound; run heads per point (cloud 0, restatement) {c['run_heads_per_point_cloud0']:.3f}; after the {s['batch']} clouds: "
                        f"{c['stats_after_fresh']}, load {c['load']:.3f}\n"
                        f"  extraction (min_count 1): {1e3 * c['extract_ms']:.1f} us for {c['extract_n_total']} voxels; 40 B per slot at hbm_copy "
                        f"{1e3 * c['table_bytes_bound_ms']:.1f} us -> {100 * c['extract_share_of_bound']:.1f} % of that bound\n"
                        f"  copy of the live voxels into a cleared map of the same capacity: {1e3 * c['copy_ms']:.1f} us (one launch), {c['copy_stats']}; 8 B per slot + 32 B "
                        f"per live slot ({c['live_slots']}) + 40 B per copied voxel at hbm_copy {1e3 * c['copy_bound_ms']:.1f} us -> {100 * c['copy_share_of_bound']:.1f} % of that bound\n"
                        f"  carve with the batch's last map under its pose (radius 1, margin16 8): keep_count 1 (every voxel protected) {1e3 * c['carve_dry_ms']:.1f} us "
                        f"(mean of 5), counts {c['carve_dry_counts']}; keep_count 0 {1e3 * c['carve_ms']:.1f} us (one launch), counts {c['carve_counts']} (live, tested, carved); "
                        f"8 B per slot + 32 B per live slot at hbm_copy {1e3 * c['carve_bound_ms']:.1f} us -> {100 * c['carve_dry_share_of_bound']:.1f} % / "
                        f"{100 * c['carve_share_of_bound']:.1f} % of that bound\n"
                        f"  render at {W} x {H} under the last cloud's pose (two memsets + splat + resolve, mean of 5): max_radius {c['render_max_radius']} "
                        f"{1e3 * c['render_ms']:.1f} us, counts {c['render_counts']} (qualifying, drawn, splat = atomic requests, pixels); 8 B per slot + 32 B per "
                        f"qualifying slot + 11 B per pixel at hbm_copy {1e3 * c['render_bound_ms']:.1f} us -> {100 * c['render_share_of_bound']:.1f} % of that bound; "
                        f"max_radius 0 {1e3 * c['render_r0_ms']:.1f} us, counts {c['render_r0_counts']}, {100 * c['render_r0_share_of_bound']:.1f} % of its bound "
                        f"({1e3 * c['render_r0_bound_ms']:.1f} us)\n"
                        f"  the default render by drawing mode of the splat launch (same image in all four, us): "
                        f"{ {k: round(1e3 * v, 1) for k, v in c['render_modes_ms'].items()} }\n"
                        f"  grid of {c['grid_cells'][0]} x {c['grid_cells'][1]} cells of {c['grid_cell_voxels']} voxels around the last cloud's pose (two memsets + walk + "
                        f"resolve, mean of 5): {1e3 * c['grid_ms']:.1f} us, counts {c['grid_counts']} (qualifying, in band, binned = 4 atomic requests each, cells, "
                        f"obstacles), classes {c['grid_classes']} (unknown, level, obstacle), {c['grid_binned_per_cell']:.1f} binned voxels per occupied cell; "
                        f"16 B per slot + 8 B per qualifying slot + 90 B per cell at hbm_copy {1e3 * c['grid_bound_ms']:.1f} us -> {100 * c['grid_share_of_bound']:.1f} % "
                        f"of that bound; {c['grid_ms'] / c['carve_dry_ms']:.2f} x the carve with every voxel protected, {c['grid_ms'] / c['render_ms']:.2f} x the render\n"
                        f"  the grid by mode of the walk (same bytes in both, two alternating blocks of 5, us): "
                        f"{ {k: [round(1e3 * x, 1) for x in v] for k, v in c['grid_modes_ms'].items()} }; the figure above is the default mode's\n"
                        + "".join(
                            f"  clearance of that grid, sources = classes of mask {k['source_mask']:#x}, max_dist {k['max_dist']} (counts' memset + row pass + column pass, all four "
                            f"outputs, mean of 5): {1e3 * k['ms']:.1f} us, counts {k['counts']} (sources, reached, unreached, blocked at a radius of 2 cells); loop steps "
                            f"summed over the cells {k['steps'][0]} (row pass) + {k['steps'][1]} (column pass); 22 B per cell at hbm_copy {1e3 * k['bound_ms']:.2f} us -> "
                            f"{100 * k['share_of_bound']:.1f} % of that bound\n" for k in c['clearance']) +
                        "".join(
                            f"  route over that grid's clearance at an inflation of two cells, near_r2 {k['near_r2']}, near_weight {k['near_weight']}, goal at the centre cell, starts at the "
                            f"corners (memsets + goals + rounds + verdict + finish + paths, mean of 5): "
                            f"{1e3 * k['ms']:.1f} us at max_rounds {k['max_rounds']}, rounds_run {k['rounds_run']}, counts {k['counts'][:5]} (goals used, reached, unreached, impassable, "
                            f"converged), path lengths {k['path_lens']} with status {k['path_status']}; at max_rounds = rounds_run {1e3 * k['ms_at_rounds_run']:.1f} us (converged "
                            f"{k['converged_at_rounds_run']}), with 64 more {1e3 * k['ms_at_64_more']:.1f} us -> {k['idle_round_us']:.2f} us per round that finds nothing to do; the path "
                            f"launch {k['path_launch_us']:.1f} us = {k['path_us_per_step']:.3f} us per step of the longest path; one pass over the arrays at hbm_copy "
                            f"{1e3 * k['bound_ms']:.2f} us; device-to-host copies of blocked and dist2 {1e3 * k['d2h_copies_ms']:.0f} us"
                            f" and this tool's Python Dijkstra on the host {k['host_dijkstra_ms']:.0f} ms\n" for k in [c['route']]) +
                        "".join(
                            f"  frontiers of that grid off that clearance, cost from a route out of the centre cell (route counts {k['route_counts']}), min_size {k['min_size']}, "
                            f"max_frontiers {k['max_frontiers']} (counts' memset + ten launches, mean of 5): {1e3 * k['ms']:.1f} us, without the combining of runs "
                            f"{1e3 * k['ms_without_combining']:.1f} us, counts {k['counts']} (free, unknown, frontier cells, frontiers, kept, written, kept cells), largest "
                            f"written {k['largest_written']} cells; cls + blocked + 8 B of labels per cell at hbm_copy {1e3 * k['bound_ms']:.2f} us; device-to-host copies of "
                            f"cls, blocked and cost {1e3 * k['d2h_copies_ms']:.0f} us and the restatement's numpy route on the host {k['host_numpy_ms']:.0f} ms\n"
                            for k in [c['frontier']]) +
                        "  view over those frontiers' goal_cells and that route's cost: " + view_line(c['view']) +
                        "  surface of that grid's cls and top at the defaults: " + surface_line(c['surface']) +
                        "  waypoints of the route from a corner to the centre cell over that clearance: " + waypoint_line(c['waypoints']) +
                        f"  removal of the last inserted cloud ({c['remove_move_points']} points, mean of 5): {1e3 * c['remove_ms']:.1f} us, counts {c['remove_counts']} "
                        f"(removed, rejected, missing, short); move to a pose 1 cm and 0.1 degrees away (removal + insert): {1e3 * c['move_ms']:.1f} us, counts "
                        f"{c['move_counts']}; the same cloud inserted once more, same run: {1e3 * c['insert_ms']:.1f} us -> removal / insert "
                        f"{c['remove_ms'] / c['insert_ms']:.2f}, move / insert {c['move_ms'] / c['insert_ms']:.2f}; 16 B per record at hbm_copy "
                        f"{1e3 * c['remove_move_bound_ms']:.2f} us\n"
                        "  align: " + align_line(c['align'], c['insert_ms']) +
                        "  normals: " + normals_line(c['normals'], c['align'], c['insert_ms']) + "  locate: " + locate_line(c['locate'], c['align']) + "  sight lines: " + rays_line(c['rays']) +
                        "  " + distance_line(c['distance']) + "  " + voxel_route_line(c['voxel_route']))
            for k in s["clearance_synthetic"]:
                f.write(f"clearance of a synthetic {k['cells'][0]} x {k['cells'][1]} grid, source density {k['density']}, max_dist {k['max_dist']} (all four outputs, mean of 5): "
                        f"{1e3 * k['ms']:.1f} us, counts {k['counts']} (sources, reached, unreached, blocked); 22 B per cell at hbm_copy {1e3 * k['bound_ms']:.1f} us -> "
                        f"{100 * k['share_of_bound']:.1f} % of that bound\n")
            for k in s["route_synthetic"]:
                f.write(f"route over a synthetic {k['cells'][0]} x {k['cells'][1]} grid, blocked density {k['density']}, no dist2, goal at the centre cell, starts at the corners (mean of 5): "
                        f"{1e3 * k['ms']:.1f} us at max_rounds {k['max_rounds']}, rounds_run {k['rounds_run']}, counts {k['counts'][:5]} (goals used, reached, unreached, impassable, "
                        f"converged), path lengths {k['path_lens']} with status {k['path_status']}; at max_rounds = rounds_run {1e3 * k['ms_at_rounds_run']:.1f} us (converged "
                        f"{k['converged_at_rounds_run']}), with 64 more {1e3 * k['ms_at_64_more']:.1f} us -> {k['idle_round_us']:.2f} us per round that finds nothing to do; the path "
                        f"launch {k['path_launch_us']:.1f} us = {k['path_us_per_step']:.3f} us per step of the longest path; one pass over the arrays at hbm_copy "
                        f"{1e3 * k['bound_ms']:.2f} us; device-to-host copies of blocked and dist2 {1e3 * k['d2h_copies_ms']:.0f} us"
                        f"\n")
            for k in s["frontier_synthetic"]:
                f.write(f"frontiers of a synthetic {k['cells'][0]} x {k['cells'][1]} grid, (unknown, obstacle) densities {k['densities']}, min_size {k['min_size']}, max_frontiers "
                        f"{k['max_frontiers']} (mean of 5): {1e3 * k['ms']:.1f} us, without the combining of runs {1e3 * k['ms_without_combining']:.1f} us, counts {k['counts']} "
                        f"(free, unknown, frontier cells, frontiers, kept, written, kept cells), largest written {k['largest_written']} cells; cls + blocked + 8 B of labels "
                        f"per cell at hbm_copy {1e3 * k['bound_ms']:.2f} us; device-to-host copies of the inputs {1e3 * k['d2h_copies_ms']:.0f} us\n")
            for k in s["view_synthetic"]:
                f.write(f"view over a synthetic {k['cells'][0]} x {k['cells'][1]} grid, (unknown, obstacle) densities {k['densities']}: " + view_line(k))
            for k in s["surface_synthetic"]:
                f.write(f"surface of a synthetic {k['cells'][0]} x {k['cells'][1]} grid: " + surface_line(k))
            for k in s["waypoint_synthetic"]:
                f.write(f"waypoints over a synthetic {k['cells'][0]} x {k['cells'][1]} grid, blocked density {k['density']}: " + waypoint_line(k))
            if g and "ratio_ledger_to_clouds" in g:
                f.write(f"{g['lanes']} lanes in {g['groups']} groups, {g['frames_per_step_per_lane']}-frame steps, {g['rounds']} alternating rounds of {g['steps']} steps, clouds at "
                        f"step {g['cloud_step']}, every lane's ledger holding {g['ledger_held_per_lane']} keyframes and moving all of them (1 cm, 0.1 degrees) after each call: "
                        f"{g['frames_per_s_clouds_ledger']:.0f} frames/s ({g['step_ms_clouds_ledger']:.1f} ms / step) beside clouds alone {g['frames_per_s_clouds']:.0f}: ratio "
                        f"{g['ratio_ledger_to_clouds']:.3f}; rounds: {[round(x) for x in g['all_clouds_ledger']]} beside {[round(x) for x in g['all_clouds']]}; per round "
                        f"{[round(x, 3) for x in g['round_ratios_ledger_to_clouds']]}; held at the end {g['ledger_held_at_the_end']}; totals over all lane maps: "
                        f"{g['ledger_totals_over_all_lane_maps']}\n")
            if g and "frames_per_s_plain" in g:
                f.write(f"{g['lanes']} lanes in {g['groups']} groups, {g['frames_per_step_per_lane']}-frame steps, median of {g['rounds']} alternating rounds of "
                        f"{g['steps']} steps, clouds at step {g['cloud_step']}:\n  without clouds {g['frames_per_s_plain']:.0f} frames/s ({g['step_ms_plain']:.1f} ms / step), "
                        f"with {g['frames_per_s_clouds']:.0f} frames/s ({g['step_ms_clouds']:.1f} ms / step): ratio {g['ratio']:.3f}\n"
                        f"  rounds without: {[round(x) for x in g['all_plain']]}, with: {[round(x) for x in g['all_clouds']]}; "
                        f"keyframes in the last step of each round with clouds: {g['keyframes_in_last_step']}\n"
                        f"  with clouds and the speckle filter (max_size {g['speckle_max_size']}, max_diff16 {g['speckle_max_diff16']}): "
                        f"{g['frames_per_s_clouds_speckle']:.0f} frames/s ({g['step_ms_clouds_speckle']:.1f} ms / step): ratio to clouds alone "
                        f"{g['ratio_speckle_to_clouds']:.3f}; rounds: {[round(x) for x in g['all_clouds_speckle']]}\n"
                        f"  with clouds and the left-right check (max_diff16 {g['lr_max_diff16']}): {g['frames_per_s_clouds_lr_check']:.0f} frames/s "
                        f"({g['step_ms_clouds_lr_check']:.1f} ms / step): ratio to clouds alone {g['ratio_lr_check_to_clouds']:.3f}; rounds: "
                        f"{[round(x) for x in g['all_clouds_lr_check']]}; per round {[round(x, 3) for x in g['round_ratios_lr_check_to_clouds']]}\n"
                        f"  with clouds from semi-global matching (defaults, sub-batches of {api_sub()} keyframes): {g['frames_per_s_clouds_sgm']:.0f} frames/s "
                        f"({g['step_ms_clouds_sgm']:.1f} ms / step): ratio to clouds alone {g['ratio_sgm_to_clouds']:.3f}; rounds: "
                        f"{[round(x) for x in g['all_clouds_sgm']]}; per round {[round(x, 3) for x in g['round_ratios_sgm_to_clouds']]}\n"
                        f"  with clouds, every keyframe cloud inserted into its lane's voxel map after each call (0.1 m, 2^{g['voxel_lane_log2']} slots per lane): "
                        f"{g['frames_per_s_clouds_voxel']:.0f} frames/s ({g['step_ms_clouds_voxel']:.1f} ms / step): ratio to clouds alone "
                        f"{g['ratio_voxel_to_clouds']:.3f}; rounds: {[round(x) for x in g['all_clouds_voxel']]}; per round "
                        f"{[round(x, 3) for x in g['round_ratios_voxel_to_clouds']]}; totals over all lane maps: {g['voxel_totals_over_all_lane_maps']}\n"
                        f"  the same with every keyframe's map carving its lane's map before its cloud goes in (defaults): {g['frames_per_s_clouds_voxel_carve']:.0f} frames/s "
                        f"({g['step_ms_clouds_voxel_carve']:.1f} ms / step): ratio to insert only {g['ratio_carve_to_voxel']:.3f}; rounds: "
                        f"{[round(x) for x in g['all_clouds_voxel_carve']]}; per round {[round(x, 3) for x in g['round_ratios_carve_to_voxel']]}\n")


if __name__ == "__main__":
    main()
