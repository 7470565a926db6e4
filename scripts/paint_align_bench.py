"""Times the paint alignment (csrc/prh_align.hpp, pointnet_refine_amd/align.py) on the detector-run-
sized input of scripts/ground_lift_bench.py - 2,000 frames x 12 lines over generated float64 slices
- and writes a report (default profiles/r19_paint_align_bench.txt) that ends in one JSON line:

  filter_ms           prh_align_select_count + the scan + prh_align_select_write over all frames
                      (device events), next to the bytes they move - every point twice, the survivors'
                      records once - and their time at 5 TB/s
  score_*             prh_align_score over the coarse table (441 shifts) on the first --score-frames
                      frames, at intensity_floor 0 and at a paint-only floor (40): device events, and
                      (candidate, shift, segment) products per second, next to fuse_project's 6.5e11
                      pairs / s (profiles/r10_map_fusion_bench.txt), the same projection
  align_lines_ms      align_lines whole on the first --align-frames frames at the paint-only floor (wall
                      clock), and the share of it the host spends on CSR, bitmaps, plans and picks
  refine_*_ms         link.refine_predictions(batched=True) without and with align, in this run, on a
                      generated drive of --e2e-frames frames x --e2e-lanes lanes with paint on the lanes
  numpy_frame_ms      the numpy restatement of the rule (tests/_align_cases.py) on ONE frame's coarse
                      table; numpy_scaled_s is that figure times the number of frames: scaled, not measured

A frame's slice is a flat road of --points-per-frame points over the 52 m x 46 m the lines cover,
intensity uniform in 0 .. 60, generated on the device: a third of it passes the paint-only floor.

    python scripts/paint_align_bench.py [--frames 2000] [--lanes 12] [--points-per-frame 50000] [--out FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HBM_BYTES_PER_S = 5e12
FUSE_PROJECT_PAIRS_PER_S = 6.5e11
PAINT_FLOOR = 40.0


def write_painted_drive(root, n_frames, n_lanes, rng):
    """A straight drive with the road at ego z = 0: poses 2.5 m apart, lanes 3.5 m apart with 20 paint
    points / m at intensity 40-60, asphalt at 4 points / m^2 and intensity 0-10; the detector's lines
    lie (0.3, 0.44) m beside the lanes."""
    import _fuse_oracle as O
    from pointnet_refine_amd.pcd import write_pcd_host
    os.makedirs(os.path.join(root, "pose"))
    length, half = 2.5 * n_frames + 60.0, 1.75 * n_lanes + 2.0
    n = int(4 * length * 2 * half)
    parts = [np.column_stack([rng.uniform(-30.0, length - 30.0, n), rng.uniform(-half, half, n), rng.normal(0.0, 0.02, n),
                              rng.uniform(0.0, 10.0, n)])]
    lanes = [3.5 * (l - (n_lanes - 1) / 2) for l in range(n_lanes)]
    for y in lanes:
        m = int(20 * length)
        parts.append(np.column_stack([rng.uniform(-30.0, length - 30.0, m), y + rng.uniform(-0.075, 0.075, m),
                                      rng.normal(0.0, 0.02, m), rng.uniform(40.0, 60.0, m)]))
    cloud = np.concatenate(parts)
    write_pcd_host(os.path.join(root, "merged.pcd"), cloud)
    results = {}
    for k in range(n_frames):
        ts = 1000 + k
        pose = np.array([2.5 * k, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": 0.0, "qy": 0.0, "qz": 0.0, "qw": 1.0},
                  open(os.path.join(root, "pose", f"{ts}.json"), "w"))
        inst = []
        for y in lanes:
            x = np.linspace(-24.0, 24.0, 13)
            ego = O.to_ego(np.column_stack([pose[0] + x, np.full(13, y), np.zeros(13)]), pose)
            inst.append({"data": np.stack([(25.0 - (ego[:, 1] + 0.44)) / 0.05, (25.0 - (ego[:, 0] + 0.3)) / 0.05], 1).tolist(),
                         "score": 0.9})
        results[f"cam/{ts}.jpg"] = {"pred_instances": inst}
    json.dump(results, open(os.path.join(root, "results.json"), "w"))
    return len(cloud)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--lanes", type=int, default=12)
    ap.add_argument("--points-per-frame", type=int, default=50000)
    ap.add_argument("--score-frames", type=int, default=8)
    ap.add_argument("--align-frames", type=int, default=40)
    ap.add_argument("--e2e-frames", type=int, default=40)
    ap.add_argument("--e2e-lanes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_paint_align_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("paint_align_bench.py needs a GPU")
    import _align_cases as C
    from link_bench import events_ms, make_run, wall_ms
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import align as AL
    from pointnet_refine_amd import link
    dev = G.device("align")

    def median_wall(fn, reps=args.reps):
        fn()
        runs = [wall_ms(fn)[0] for _ in range(reps)]
        return float(np.median(runs)), [round(v, 3) for v in runs]

    # ---- the run of link_bench.py: its pieces are the lines, on the road at z = 0
    pieces, _, _ = make_run(args.frames, args.lanes, np.random.default_rng(0))
    pieces[:, :, 2] = 0.0
    lines = [list(pieces[f * args.lanes:(f + 1) * args.lanes]) for f in range(args.frames)]
    n_pts = args.points_per_frame
    gen = torch.Generator(device=dev).manual_seed(0)
    points = torch.empty((args.frames * n_pts, 4), dtype=torch.float64, device=dev)
    points[:, 0] = torch.rand(len(points), generator=gen, device=dev, dtype=torch.float64) * 52.0 - 26.0
    points[:, 1] = torch.rand(len(points), generator=gen, device=dev, dtype=torch.float64) * 46.0 - 23.0
    points[:, 2] = 0.02 * torch.randn(len(points), generator=gen, device=dev, dtype=torch.float64)
    points[:, 3] = torch.rand(len(points), generator=gen, device=dev, dtype=torch.float64) * 60.0
    off = np.arange(args.frames + 1, dtype=np.int64) * n_pts
    coarse = AL.shift_grid((0.0, 0.0), AL.COARSE_HALF, AL.COARSE_STEP)

    def tables(n):
        return np.concatenate([coarse] * n), np.arange(n + 1, dtype=np.int64) * len(coarse)

    # ---- the filter over all frames
    sh, k_off = tables(args.frames)
    filt = {}
    for name, floor in (("floor0", 0.0), ("paint", PAINT_FLOOR)):
        p = AL.prepare(points, off, lines, sh, k_off, AL.RADIUS, floor, AL.CELL, "bench")
        runs = events_ms(lambda: AL.select_candidates(p), args.reps)
        rec, _, c_off = AL.select_candidates(p)
        moved = 2 * int(off[-1]) * 32 + int(rec.shape[0]) * 32
        filt[name] = {"ms": float(np.median(runs)), "runs": [round(v, 3) for v in runs], "candidates": int(rec.shape[0]),
                      "bytes": moved, "cells": p["maps"]["n_cells"], "set": int(np.unpackbits(p["maps"]["bitmap"].view(np.uint8)).sum())}
        del rec, p

    # ---- the score sweep on the first frames
    nf = args.score_frames
    sh, k_off = tables(nf)
    segments = sum(len(v) - 1 for ls in lines[:nf] for v in ls) // nf
    score = {}
    for name, floor in (("floor0", 0.0), ("paint", PAINT_FLOOR)):
        p = AL.prepare(points[:nf * n_pts], off[:nf + 1], lines[:nf], sh, k_off, AL.RADIUS, floor, AL.CELL, "bench")
        rec, cand_off, c_off = AL.select_candidates(p)
        runs = events_ms(lambda: AL.score_candidates(p, rec, cand_off, c_off), args.reps)
        products = int(sum(int(c) * len(coarse) * sum(len(v) - 1 for v in lines[f]) for f, c in enumerate(np.diff(c_off))))
        ms = float(np.median(runs))
        score[name] = {"ms": ms, "runs": [round(v, 3) for v in runs], "candidates": int(rec.shape[0]), "products": products,
                       "per_s": products / (ms * 1e-3)}
        if name == "paint":
            acc = AL.score_candidates(p, rec, cand_off, c_off).cpu().numpy()

    # ---- numpy on one frame's coarse table at the paint-only floor, scaled
    p0 = points[:n_pts].cpu().numpy()
    t = time.perf_counter()
    one = C.paint_scores_np(p0, [0, n_pts], [lines[0]], coarse, [0, len(coarse)], AL.RADIUS, PAINT_FLOOR)
    numpy_frame_ms = (time.perf_counter() - t) * 1e3
    same = bool(np.array_equal(one["score"], acc[:len(coarse), 0]) and np.array_equal(one["hits"], acc[:len(coarse), 1]))

    # ---- align_lines whole, and the host's part of it
    na = args.align_frames
    a_pts, a_off, a_lines = points[:na * n_pts], off[:na + 1], lines[:na]
    whole_ms, whole_all = median_wall(lambda: AL.align_lines(a_pts, a_off, a_lines, intensity_floor=PAINT_FLOOR))
    sh_a, k_a = tables(na)

    def host_part():
        for _ in range(2):                                   # the coarse and the fine stage
            verts, l_off, sl_off = AL.lines_csr(a_lines)
            maps = AL.segment_bitmaps(verts, l_off, sl_off, AL.slice_reach(sh_a, k_a, AL.RADIUS), AL.CELL)
            AL.work_items(np.arange(na + 1) * 6000, k_a, np.diff(l_off[sl_off]))
            for s in range(na):
                AL.pick_shift(coarse, np.arange(len(coarse)), np.full(len(coarse), 99))
        return maps

    host_ms, host_all = median_wall(host_part)
    del points, a_pts

    # ---- refine_predictions on a painted drive, without and with align
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    model = LineRefineNet()
    model.load_state_dict(P.linerefine_state_dict(0))
    model = model.cuda().eval()
    with tempfile.TemporaryDirectory() as root:
        n_cloud = write_painted_drive(root, args.e2e_frames, args.e2e_lanes, np.random.default_rng(1))
        rj = os.path.join(root, "results.json")
        plain_ms, plain_all = median_wall(lambda: link.refine_predictions(model, root, rj, batched=True), 3)
        align_ms, align_all = median_wall(lambda: link.refine_predictions(model, root, rj, batched=True, align=True), 3)
        rep = link.refine_predictions(model, root, rj, batched=True, align=True)["report"]
    norm = np.hypot(rep["align_shifts"][:, 0], rep["align_shifts"][:, 1])

    out = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "lanes": args.lanes, "points": int(off[-1]),
           "points_per_frame": n_pts, "shifts": len(coarse), "segments_per_frame": segments, "reps": args.reps,
           "filter_floor0_ms": round(filt["floor0"]["ms"], 3), "filter_paint_ms": round(filt["paint"]["ms"], 3),
           "filter_bytes": filt["floor0"]["bytes"], "filter_bytes_at_5TBs_ms": round(filt["floor0"]["bytes"] / HBM_BYTES_PER_S * 1e3, 3),
           "filter_candidates_floor0": filt["floor0"]["candidates"], "filter_candidates_paint": filt["paint"]["candidates"],
           "cells": filt["floor0"]["cells"], "cells_set": filt["floor0"]["set"], "score_frames": nf,
           "score_floor0_ms": round(score["floor0"]["ms"], 3), "score_floor0_products": score["floor0"]["products"],
           "score_floor0_products_per_s": float(f"{score['floor0']['per_s']:.4g}"),
           "score_paint_ms": round(score["paint"]["ms"], 3), "score_paint_products": score["paint"]["products"],
           "score_paint_products_per_s": float(f"{score['paint']['per_s']:.4g}"),
           "fuse_project_pairs_per_s": FUSE_PROJECT_PAIRS_PER_S, "align_frames": na, "align_lines_ms": round(whole_ms, 1),
           "align_lines_host_ms": round(host_ms, 1), "numpy_frame_ms": round(numpy_frame_ms, 1),
           "numpy_scaled_s": round(numpy_frame_ms * args.frames / 1e3, 1), "numpy_frame_bitwise_equal": same,
           "e2e_frames": args.e2e_frames, "e2e_lanes": args.e2e_lanes, "e2e_cloud_points": n_cloud,
           "refine_plain_ms": round(plain_ms, 1), "refine_align_ms": round(align_ms, 1),
           "e2e_frames_aligned": rep["align_frames_aligned"], "e2e_shift_median_m": round(float(np.median(norm)), 3)}
    text = f"""Paint alignment: the xy shift that puts every frame's detector lines on the paint, read from the frames' own slices
(prh_align_select_count, prh_align_select_write, prh_align_score; align.align_lines).
Command: python scripts/paint_align_bench.py   (--frames {args.frames} --lanes {args.lanes} --points-per-frame {n_pts} --score-frames {nf} --align-frames {na} --e2e-frames {args.e2e_frames} --e2e-lanes {args.e2e_lanes} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, one process, {time.strftime('%Y-%m-%d')}.
Timing: device events, median of {args.reps} after one warm-up call, for the filter and the score sweep; wall clock, median
after one warm-up call, for align_lines, its host part ({args.reps} runs) and refine_predictions (3 runs).

{args.frames} frames x {args.lanes} lines ({segments} segments per frame), {int(off[-1])} float64 points ({n_pts} per frame, intensity 0 .. 60),
{filt['floor0']['cells']} bitmap cells of {AL.CELL} m, {filt['floor0']['set']} set (coarse table: reach {AL.RADIUS + AL.COARSE_HALF + AL.GUARD:.6f} m).
filter (count + scan + write), intensity_floor 0: runs (ms) {filt['floor0']['runs']} median {filt['floor0']['ms']:.3f}, {filt['floor0']['candidates']} candidates;
  it reads every point twice and writes the records once: {filt['floor0']['bytes']} B, which take {filt['floor0']['bytes'] / HBM_BYTES_PER_S * 1e3:.3f} ms at 5 TB/s.
filter, paint-only floor {PAINT_FLOOR:g}: runs (ms) {filt['paint']['runs']} median {filt['paint']['ms']:.3f}, {filt['paint']['candidates']} candidates.
prh_align_score, {len(coarse)} shifts, first {nf} frames, intensity_floor 0: runs (ms) {score['floor0']['runs']} median {score['floor0']['ms']:.3f};
  {score['floor0']['candidates']} candidates, {score['floor0']['products']} (candidate, shift, segment) products: {score['floor0']['per_s']:.3e} products / s.
prh_align_score, paint-only floor: runs (ms) {score['paint']['runs']} median {score['paint']['ms']:.3f};
  {score['paint']['candidates']} candidates, {score['paint']['products']} products: {score['paint']['per_s']:.3e} products / s.
  fuse_project, the same projection: 6.5e11 pairs / s (profiles/r10_map_fusion_bench.txt).  A product is counted whether or
  not the box compare skipped it.
align_lines whole, first {na} frames, paint-only floor, runs (ms): {whole_all} median {whole_ms:.1f};
  its host part alone (CSR, bitmaps, plans, picks of both stages), runs (ms): {host_all} median {host_ms:.1f}.
numpy restatement on ONE frame's coarse table at the paint-only floor: {numpy_frame_ms:.1f} ms, bitwise equal to the device: {same};
  scaled by {args.frames} frames: {numpy_frame_ms * args.frames / 1e3:.1f} s (scaled, not measured).
refine_predictions(batched=True) on a painted generated drive ({args.e2e_frames} frames x {args.e2e_lanes} lines, {n_cloud} cloud points, the lines
  (0.3, 0.44) m beside the paint): without align {plain_all} median {plain_ms:.1f} ms;
  with align {align_all} median {align_ms:.1f} ms ({rep['align_frames_aligned']} of {rep['align_frames']} frames aligned, median |shift| {float(np.median(norm)):.3f} m).

{json.dumps(out)}
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
