"""Times the rigid paint alignment (prh_align_score_rigid and the cell-ordered select passes of
csrc/prh_align.hpp, align.align_lines_rigid) on the workload of scripts/paint_align_bench.py - frames of
12 lines over generated float64 slices of 50,000 points, intensity_floor 0 and a paint-only floor (40)
- and writes a report (default profiles/r20_paint_align_rigid_bench.txt) that ends in one JSON line:

  prologue_*   (a) prh_align_score on the 441-row coarse shift table against prh_align_score_rigid on
               the same table with theta = 0, both over the same arrival-order records of 8 frames: the
               cost of the pose prologue, with prh_align_score as the yardstick
  order_*      (b) prh_align_score_rigid on the 4,851-row coarse pose table of 8 frames over
               arrival-order records and over cell-order records, and the two select passes on their own
  whole_*      (c) align_lines_rigid whole on 40 frames at the paint-only floor, in both orders, next
               to align_lines (wall clock)

Device events, median of --reps after one warm-up call, one process; every pair of tables compared is
also checked for bitwise equality.

    python scripts/paint_align_rigid_bench.py [--score-frames 8] [--align-frames 40] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PAINT_FLOOR = 40.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=12)
    ap.add_argument("--points-per-frame", type=int, default=50000)
    ap.add_argument("--score-frames", type=int, default=8)
    ap.add_argument("--align-frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_paint_align_rigid_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("paint_align_rigid_bench.py needs a GPU")
    from link_bench import events_ms, make_run, wall_ms
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import align as AL
    dev = G.device("align")
    frames = max(args.score_frames, args.align_frames)

    def stat(runs):
        return {"ms": float(np.median(runs)), "runs": [round(v, 3) for v in runs]}

    def median_wall(fn):
        fn()
        return stat([wall_ms(fn)[0] for _ in range(args.reps)])

    # ---- paint_align_bench.py's run: link_bench.py's pieces are the lines, on the road at z = 0
    pieces, _, _ = make_run(frames, args.lanes, np.random.default_rng(0))
    pieces[:, :, 2] = 0.0
    lines = [list(pieces[f * args.lanes:(f + 1) * args.lanes]) for f in range(frames)]
    n_pts = args.points_per_frame
    gen = torch.Generator(device=dev).manual_seed(0)
    points = torch.empty((frames * n_pts, 4), dtype=torch.float64, device=dev)
    points[:, 0] = torch.rand(len(points), generator=gen, device=dev, dtype=torch.float64) * 52.0 - 26.0
    points[:, 1] = torch.rand(len(points), generator=gen, device=dev, dtype=torch.float64) * 46.0 - 23.0
    points[:, 2] = 0.02 * torch.randn(len(points), generator=gen, device=dev, dtype=torch.float64)
    points[:, 3] = torch.rand(len(points), generator=gen, device=dev, dtype=torch.float64) * 60.0
    off = np.arange(frames + 1, dtype=np.int64) * n_pts
    nf = args.score_frames
    s_pts, s_off, s_lines = points[:nf * n_pts], off[:nf + 1], lines[:nf]
    shifts = AL.shift_grid((0.0, 0.0), AL.COARSE_HALF, AL.COARSE_STEP)
    flat = np.column_stack([shifts, np.zeros(len(shifts))])
    coarse = AL.pose_grid((0.0, 0.0), AL.COARSE_HALF, AL.COARSE_STEP, 0.0, AL.COARSE_YAW, AL.COARSE_YAW_STEP)

    def tables(t, n):
        return np.concatenate([t] * n), np.arange(n + 1, dtype=np.int64) * len(t)

    res = {}
    for name, floor in (("floor0", 0.0), ("paint", PAINT_FLOOR)):
        # (a) the prologue: the same records, the same 441 rows
        p = AL.prepare(s_pts, s_off, s_lines, *tables(shifts, nf), AL.RADIUS, floor, AL.CELL, "bench")
        q = AL.prepare(s_pts, s_off, s_lines, *tables(flat, nf), AL.RADIUS, floor, AL.CELL, "bench", rigid=True)
        assert np.array_equal(p["reach"], q["reach"])
        rec, cand_off, c_off = AL.select_candidates(p)
        shift = stat(events_ms(lambda: AL.score_candidates(p, rec, cand_off, c_off), args.reps))
        rigid = stat(events_ms(lambda: AL.score_candidates(q, rec, cand_off, c_off), args.reps))
        same_a = bool(torch.equal(AL.score_candidates(p, rec, cand_off, c_off), AL.score_candidates(q, rec, cand_off, c_off)))
        # (b) the order of the candidates under the 4,851-row table
        r = AL.prepare(s_pts, s_off, s_lines, *tables(coarse, nf), AL.RADIUS, floor, AL.CELL, "bench", rigid=True)
        sel_a = stat(events_ms(lambda: AL.select_candidates(r), args.reps))
        sel_c = stat(events_ms(lambda: AL.select_candidates(r, "cell"), args.reps))
        ra, oa, ha = AL.select_candidates(r)
        rc, oc, hc = AL.select_candidates(r, "cell")
        sc_a = stat(events_ms(lambda: AL.score_candidates(r, ra, oa, ha), args.reps))
        sc_c = stat(events_ms(lambda: AL.score_candidates(r, rc, oc, hc), args.reps))
        same_b = bool(torch.equal(AL.score_candidates(r, ra, oa, ha), AL.score_candidates(r, rc, oc, hc)))
        res[name] = {"candidates_441": int(rec.shape[0]), "score_shift": shift, "score_rigid_theta0": rigid, "equal_a": same_a,
                     "candidates_4851": int(ra.shape[0]), "cells": r["maps"]["n_cells"], "reach": float(r["reach"][0]),
                     "select_arrival": sel_a, "select_cell": sel_c, "score_arrival": sc_a, "score_cell": sc_c, "equal_b": same_b}
        del rec, ra, rc, p, q, r

    # (c) the whole procedure
    na = args.align_frames
    a_pts, a_off, a_lines = points[:na * n_pts], off[:na + 1], lines[:na]
    whole = {"align_lines": median_wall(lambda: AL.align_lines(a_pts, a_off, a_lines, intensity_floor=PAINT_FLOOR))}
    default = AL.ORDER
    for order in ("arrival", "cell"):
        AL.ORDER = order
        whole[order] = median_wall(lambda: AL.align_lines_rigid(a_pts, a_off, a_lines, intensity_floor=PAINT_FLOOR))
    AL.ORDER = default

    out = {"device": torch.cuda.get_device_name(0), "lanes": args.lanes, "points_per_frame": n_pts, "score_frames": nf,
           "align_frames": na, "reps": args.reps, "rows_shift": len(shifts), "rows_coarse": len(coarse),
           "default_order": default, "results": res, "whole": whole}
    rows = []
    for name, label in (("floor0", "intensity_floor 0"), ("paint", f"paint-only floor {PAINT_FLOOR:g}")):
        v = res[name]
        rows.append(f"""{label}:
  (a) 441 rows, {v['candidates_441']} arrival-order candidates of {nf} frames.
      prh_align_score            runs (ms) {v['score_shift']['runs']} median {v['score_shift']['ms']:.3f}
      prh_align_score_rigid, theta = 0  runs (ms) {v['score_rigid_theta0']['runs']} median {v['score_rigid_theta0']['ms']:.3f}   tables bitwise equal: {v['equal_a']}
  (b) {len(coarse)} rows, reach {v['reach']:.6f} m, {v['cells']} cells, {v['candidates_4851']} candidates of {nf} frames.
      select, arrival order (count + scan + write)  runs (ms) {v['select_arrival']['runs']} median {v['select_arrival']['ms']:.3f}
      select, cell order (count + scan + write)     runs (ms) {v['select_cell']['runs']} median {v['select_cell']['ms']:.3f}
      prh_align_score_rigid, arrival order  runs (ms) {v['score_arrival']['runs']} median {v['score_arrival']['ms']:.3f}
      prh_align_score_rigid, cell order     runs (ms) {v['score_cell']['runs']} median {v['score_cell']['ms']:.3f}   tables bitwise equal: {v['equal_b']}""")
    body = "\n".join(rows)
    text = f"""Rigid paint alignment: yaw about the sensor plus xy shift of every frame's detector lines, read from the frames' own slices
(prh_align_score_rigid, prh_align_select_cells_count, prh_align_select_cells_write; align.align_lines_rigid).
Command: python scripts/paint_align_rigid_bench.py   (--lanes {args.lanes} --points-per-frame {n_pts} --score-frames {nf} --align-frames {na} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, one process, {time.strftime('%Y-%m-%d')}.
Timing: device events around the call (its uploads of the tables included), median of {args.reps} after one warm-up call, for (a) and
(b); wall clock, median of {args.reps} after one warm-up call, for (c).

{body}
(c) whole, first {na} frames, paint-only floor, wall clock (ms):
      align_lines                         runs {whole['align_lines']['runs']} median {whole['align_lines']['ms']:.1f}
      align_lines_rigid, arrival order    runs {whole['arrival']['runs']} median {whole['arrival']['ms']:.1f}
      align_lines_rigid, cell order       runs {whole['cell']['runs']} median {whole['cell']['ms']:.1f}
      (align.ORDER, the default, is '{default}')

{json.dumps(out)}
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
