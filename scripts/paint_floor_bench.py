"""Times the paint floor (csrc/prh_floor.hpp, pointnet_refine_amd/paintfloor.py) and writes a report
(default profiles/r22_paint_floor_bench.txt) that ends in one JSON line:

  hist_*     prh_floor_hist (its memset of the table included) over the slices of a generated drive -
             --slices x --points-per-slice points, asphalt at intensity 0-10 over the whole window, 3 % of
             the points paint at 40-60 - as float64 and as float32, next to prh_trace_hist on the same
             points in the same run and next to the bytes it must read (every row once) at 5 TB/s
  copies_*   prh_test_floor_hist with 1, 2, 4 and 8 LDS copies of a block's histogram, float64
  ground     paintfloor.surface_ground: the ground table through ground.ground_heights, wall clock
  otsu       prh_floor_otsu over the slices' rows and the drive's row
  whole      paintfloor.paint_floor, wall clock
  drive_*    trace.refine_cloud with a fixed floor and with "auto", whole, on one generated drive
             directory, wall clock

Device events, median of --reps after one warm-up call, one process; every variant's table is checked
for equality with the float64 table of prh_floor_hist.

    python scripts/paint_floor_bench.py [--slices 40] [--points-per-slice 500000] [--out FILE]
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
TRACE_FLOOR = 20.0


def generated_slices(n_slices, n_pts, lanes, dev, torch):
    """(S * n_pts, 4) float64 CUDA of float32 values: 3 of every 100 points are paint."""
    gen = torch.Generator(device=dev).manual_seed(0)
    n = n_slices * n_pts

    def rand(lo, hi):
        return torch.rand(n, generator=gen, device=dev, dtype=torch.float32) * (hi - lo) + lo

    pts = torch.empty((n, 4), dtype=torch.float32, device=dev)
    pts[:, 0] = rand(-25.0, 25.0)
    pts[:, 1] = rand(-12.8, 12.8)
    pts[:, 2] = 0.02 * torch.randn(n, generator=gen, device=dev, dtype=torch.float32)
    pts[:, 3] = rand(0.0, 10.0)
    paint = torch.arange(n, device=dev) % 100 < 3
    lane = torch.randint(0, lanes, (n,), generator=gen, device=dev).to(torch.float32)
    pts[paint, 1] = ((lane - (lanes - 1) / 2.0) * 3.5 + rand(-0.075, 0.075))[paint]
    pts[paint, 3] = rand(40.0, 60.0)[paint]
    return pts.to(torch.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--points-per-slice", type=int, default=500000)
    ap.add_argument("--lanes", type=int, default=6)
    ap.add_argument("--drive-length", type=float, default=400.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_paint_floor_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("paint_floor_bench.py needs a GPU")
    from link_bench import events_ms, wall_ms
    from paint_trace_bench import write_drive
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    from pointnet_refine_amd import paintfloor as PF
    from pointnet_refine_amd import trace as T
    dev = G.device("paintfloor")
    lib = L.lib()

    def stat(runs):
        return {"ms": float(np.median(runs)), "runs": [round(v, 3) for v in runs]}

    def median_wall(fn):
        fn()
        return stat([wall_ms(fn)[0] for _ in range(args.reps)])

    n_s, n_pts = args.slices, args.points_per_slice
    p64 = generated_slices(n_s, n_pts, args.lanes, dev, torch)
    p32 = p64.to(torch.float32)
    off = np.arange(n_s + 1, dtype=np.int64) * n_pts
    off_t = torch.from_numpy(off).to(dev)
    p = PF._params("bench")
    res = {"ground": median_wall(lambda: PF.surface_ground(p64, off))}
    ground = PF.surface_ground(p64, off)
    cells_without_ground = int(torch.isnan(ground).sum().item())
    hist = torch.empty((n_s, p["n_bins"]), dtype=torch.int64, device=dev)

    def floor_hist(pts, copies=None):
        a = (G.ptr(pts), 1 if pts.dtype == torch.float64 else 0, G.ptr(off_t), n_s, pts.shape[0], p["half_length"],
             p["half_width"], p["ground_cell"], p["gx"], p["gy"], G.ptr(ground), p["band"], p["bin_width"], p["n_bins"],
             G.ptr(hist), dev.index, G.stream(dev))
        L.check(lib.prh_floor_hist(*a) if copies is None else lib.prh_test_floor_hist(copies, *a), "prh_floor_hist")

    tp = T._params("bench", intensity_floor=TRACE_FLOOR)
    nb = lib.prh_trace_workspace_bytes(n_s, tp["nx"], tp["ny"])
    ws = G.workspace(nb, dev)

    def trace_hist(pts):
        L.check(lib.prh_trace_hist(G.ptr(pts), 1 if pts.dtype == torch.float64 else 0, G.ptr(off_t), n_s, 0, pts.shape[0],
                                   tp["half_length"], tp["col"], tp["nx"], tp["half_width"], tp["cell"], tp["ny"], TRACE_FLOOR,
                                   G.ptr(ws), nb, dev.index, G.stream(dev)), "prh_trace_hist")

    res["hist_f64"] = stat(events_ms(lambda: floor_hist(p64), args.reps))
    want = hist.clone()
    res["hist_f32"] = stat(events_ms(lambda: floor_hist(p32), args.reps))
    equal = bool(torch.equal(hist, want))
    for copies in (1, 2, 4, 8):
        res[f"copies_{copies}"] = stat(events_ms(lambda: floor_hist(p64, copies), args.reps))
        equal = equal and bool(torch.equal(hist, want))
    res["trace_hist_f64"] = stat(events_ms(lambda: trace_hist(p64), args.reps))
    res["trace_hist_f32"] = stat(events_ms(lambda: trace_hist(p32), args.reps))
    res["hist_f64_again"] = stat(events_ms(lambda: floor_hist(p64), args.reps))
    del ws
    rows = torch.cat([want, want.sum(0, keepdim=True)])
    res["otsu"] = stat(events_ms(lambda: PF.otsu_floors(rows, p["min_points"], p["bin_width"]), args.reps))
    res["paint_floor"] = median_wall(lambda: PF.paint_floor(p64, off))
    floor, report = PF.paint_floor(p64, off)
    surface = int(want.sum().item())
    del p64, p32

    # ---- whole: one generated drive directory with a fixed floor and with "auto"
    from oracle import procedural as P
    from pointnet_refine_amd.model import LineRefineNet
    model = LineRefineNet()
    model.load_state_dict(P.linerefine_state_dict(0))
    model = model.cuda().eval()
    with tempfile.TemporaryDirectory() as root:
        drive, _, n_cloud = write_drive(root, args.drive_length, 500.0, 300.0)
        auto = T.refine_cloud(model, drive, intensity_floor="auto", batched=True)
        fixed_floor = auto["report"]["floor"]
        fixed = T.refine_cloud(model, drive, intensity_floor=fixed_floor, batched=True)
        whole = {"fixed": median_wall(lambda: T.refine_cloud(model, drive, intensity_floor=fixed_floor, batched=True)),
                 "auto": median_wall(lambda: T.refine_cloud(model, drive, intensity_floor="auto", batched=True))}
    whole.update(cloud_points=n_cloud, floor=fixed_floor, slices=auto["report"]["slices"],
                 surface_points=auto["report"]["floor_surface_points"], paint_share=auto["report"]["floor_paint_share"],
                 same_pieces=bool(auto["pieces"].tobytes() == fixed["pieces"].tobytes()),
                 clusters=auto["report"]["clusters_kept"])

    n = n_s * n_pts
    out = {"device": torch.cuda.get_device_name(0), "slices": n_s, "points_per_slice": n_pts, "lanes": args.lanes,
           "reps": args.reps, "gx": p["gx"], "gy": p["gy"], "n_bins": p["n_bins"], "surface_points": surface,
           "cells_without_ground": cells_without_ground, "floor": floor, "plateau": list(report["plateau"]),
           "paint_share": report["paint_share"], "contrast": report["contrast"], "tables_equal": equal, "results": res,
           "whole": whole}

    def row(key, label, nbytes=None):
        v = res[key]
        tail = ""
        if nbytes is not None:
            floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
            tail = (f"   must read {nbytes / 1e6:.0f} MB: {floor_ms:.3f} ms at 5 TB/s, {100.0 * floor_ms / v['ms']:.1f} % of that "
                    f"rate reached")
        return f"  {label:<52} runs (ms) {v['runs']} median {v['ms']:.3f}{tail}"

    text = f"""Paint floor: the intensity threshold between asphalt and paint read from the road surface (prh_floor_hist, prh_floor_otsu;
paintfloor.surface_ground, paintfloor.paint_floor, intensity_floor="auto").
Command: python scripts/paint_floor_bench.py   (--slices {n_s} --points-per-slice {n_pts} --lanes {args.lanes} --drive-length {args.drive_length:g} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, one process, {time.strftime('%Y-%m-%d')}.
Timing: device events around the call, median of {args.reps} after one warm-up call, unless a row says wall clock.

Generated slices: {n_s} x {n_pts} = {n} points, 3 % of them paint in {args.lanes} bands; surface grid {p['gx']} x {p['gy']} cells
({cells_without_ground} of {n_s * p['gx'] * p['gy']} without ground), {p['n_bins']} bins; {surface} surface points; floor {floor:g}, plateau {list(report['plateau'])},
paint share {report['paint_share']:.4f}, contrast {report['contrast']:.2f}; float32 and every copy count give the float64 table: {equal}.
{row('hist_f64', 'prh_floor_hist, float64 (memset included)', n * 32)}
{row('hist_f64_again', 'the same once more, after the other rows', n * 32)}
{row('hist_f32', 'prh_floor_hist, float32 (memset included)', n * 16)}
{row('copies_1', 'prh_test_floor_hist, float64, 1 LDS copy', n * 32)}
{row('copies_2', 'prh_test_floor_hist, float64, 2 LDS copies', n * 32)}
{row('copies_4', 'prh_test_floor_hist, float64, 4 LDS copies', n * 32)}
{row('copies_8', 'prh_test_floor_hist, float64, 8 LDS copies', n * 32)}
{row('trace_hist_f64', 'prh_trace_hist, float64, same points, floor 20', n * 32)}
{row('trace_hist_f32', 'prh_trace_hist, float32, same points, floor 20', n * 16)}
{row('ground', 'paintfloor.surface_ground (ground table), wall clock')}
{row('otsu', f'prh_floor_otsu, {n_s + 1} rows (otsu_floors: its outputs allocated)')}
{row('paint_floor', 'paintfloor.paint_floor whole, wall clock')}

Whole, one generated drive directory ({n_cloud} points, {args.drive_length:g} m, poses 25 m apart), batched contexts, wall clock (ms),
merged.pcd read and parsed inside both calls; procedural weights, so the maps say nothing about accuracy:
  trace.refine_cloud, intensity_floor={whole['floor']:g}      runs {whole['fixed']['runs']} median {whole['fixed']['ms']:.1f}
  trace.refine_cloud, intensity_floor="auto"   runs {whole['auto']['runs']} median {whole['auto']['ms']:.1f}   floor {whole['floor']:g} from {whole['surface_points']} surface points of {whole['slices']} slices, paint share {whole['paint_share']:.4f}; the same pieces: {whole['same_pieces']}; {whole['clusters']} clusters

{json.dumps(out)}
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
