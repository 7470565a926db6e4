"""Times paint tracing (csrc/prh_trace.hpp, pointnet_refine_amd/trace.py) and writes a report (default
profiles/r21_paint_trace_bench.txt) that ends in one JSON line:

  hist_*     prh_trace_hist (its memset of the tables included) over the slices of a generated drive -
             --slices x --points-per-slice points, asphalt at intensity 0-10 over the whole grid, --lanes
             bands of paint at 40-60, intensity_floor 20 - as float64 and as float32, next to the bytes
             it must read (every row once) at 5 TB/s and next to bev.bev_maps on the same points
  peaks_*    prh_trace_peaks_count, prh_trace_peaks_write and prh_trace_link on those tables
  chains_*   trace.chain_lines on the host (wall clock)
  whole_*    trace.refine_cloud against link.refine_predictions, whole, on one generated drive
             directory (the detector's lines are the lanes themselves), wall clock
  numpy_*    the numpy restatement (tests/_trace_cases.paint_peaks_np) on one slice, wall clock, and
             that time multiplied by the number of slices: scaled, not measured

Device events, median of --reps after one warm-up call, one process; paint_peaks on the float64 and
float32 points is checked for bitwise equality.

    python scripts/paint_trace_bench.py [--slices 40] [--points-per-slice 500000] [--out FILE]
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

FLOOR = 20.0
HBM_BYTES_PER_S = 5e12


def generated_slices(n_slices, n_pts, lanes, dev, torch):
    """(S * n_pts, 4) float64 CUDA of float32 values: a twentieth of every slice is paint."""
    gen = torch.Generator(device=dev).manual_seed(0)
    n = n_slices * n_pts

    def rand(lo, hi):
        return torch.rand(n, generator=gen, device=dev, dtype=torch.float32) * (hi - lo) + lo

    pts = torch.empty((n, 4), dtype=torch.float32, device=dev)
    pts[:, 0] = rand(-25.0, 25.0)
    pts[:, 1] = rand(-12.8, 12.8)
    pts[:, 2] = 0.02 * torch.randn(n, generator=gen, device=dev, dtype=torch.float32)
    pts[:, 3] = rand(0.0, 10.0)
    paint = torch.arange(n, device=dev) % 20 == 0
    lane = torch.randint(0, lanes, (n,), generator=gen, device=dev).to(torch.float32)
    pts[paint, 1] = ((lane - (lanes - 1) / 2.0) * 3.5 + rand(-0.075, 0.075))[paint]
    pts[paint, 3] = rand(40.0, 60.0)[paint]
    return pts.to(torch.float64)


def write_drive(root, length, per_m2, paint_per_m):
    """A generated drive directory: merged.pcd, pose/*.json 25 m apart, and a results JSON whose
    pixels are the two lanes in every pose's frame.  Returns (drive_dir, results_json, points)."""
    import _align_cases as AC
    from pointnet_refine_amd.pcd import write_pcd_host
    cloud = AC.paint_cloud(np.random.default_rng(1), -8.0, length + 28.0, per_m2, paint_per_m).astype(np.float32)
    drive = os.path.join(root, "drive")
    os.makedirs(os.path.join(drive, "pose"))
    write_pcd_host(os.path.join(drive, "merged.pcd"), cloud)
    results = {}
    for k in range(int(length // 25.0)):
        ts, x = 1000 + k, 25.0 * (k + 1)
        json.dump({"ts": str(ts), "x": x, "y": 0.0, "z": 0.0, "qx": 0.0, "qy": 0.0, "qz": 0.0, "qw": 1.0},
                  open(os.path.join(drive, "pose", f"{ts}.json"), "w"))
        ex = np.linspace(-24.0, 24.0, 25)
        results[f"cam/{ts}.jpg"] = {"pred_instances": [
            {"data": np.stack([(25.0 - np.full(25, y)) / 0.05, (25.0 - ex) / 0.05], 1).tolist(), "score": 0.9}
            for y in AC.LANE_Y]}
    path = os.path.join(root, "results.json")
    json.dump(results, open(path, "w"))
    return drive, path, len(cloud)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--points-per-slice", type=int, default=500000)
    ap.add_argument("--lanes", type=int, default=6)
    ap.add_argument("--drive-length", type=float, default=400.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_paint_trace_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("paint_trace_bench.py needs a GPU")
    import _trace_cases as TC
    from link_bench import events_ms, wall_ms
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    from pointnet_refine_amd import bev, link
    from pointnet_refine_amd import trace as T
    dev = G.device("trace")
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
    p = T._params("bench", intensity_floor=FLOOR)
    nx, ny = p["nx"], p["ny"]
    nb = lib.prh_trace_workspace_bytes(n_s, nx, ny)
    ws = G.workspace(nb, dev)

    def hist(pts):
        L.check(lib.prh_trace_hist(G.ptr(pts), 1 if pts.dtype == torch.float64 else 0, G.ptr(off_t), n_s, 0, pts.shape[0],
                                   p["half_length"], p["col"], nx, p["half_width"], p["cell"], ny, FLOOR, G.ptr(ws), nb,
                                   dev.index, G.stream(dev)), "prh_trace_hist")

    res = {"hist_f64": stat(events_ms(lambda: hist(p64), args.reps)), "hist_f32": stat(events_ms(lambda: hist(p32), args.reps)),
           "memset": stat(events_ms(lambda: ws.zero_(), args.reps)),
           "bev_maps_f64": stat(events_ms(lambda: bev.bev_maps(p64, off, (-12.8, 12.8, -25.0, 25.0), 0.05), args.reps))}
    hist(p64)
    counts = torch.empty((n_s * nx,), dtype=torch.int32, device=dev)
    peak = (p["nms"], p["min_points"], p["min_weight"])

    def count():
        L.check(lib.prh_trace_peaks_count(G.ptr(ws), nb, n_s, nx, ny, *peak, G.ptr(counts), dev.index, G.stream(dev)), "count")

    res["peaks_count"] = stat(events_ms(count, args.reps))
    col_off = G.exclusive_scan(counts)
    total = int(col_off[-1].item())
    iy, cnt, col = (torch.empty((total,), dtype=torch.int32, device=dev) for _ in range(3))
    weight = torch.empty((total,), dtype=torch.int64, device=dev)
    xyz = torch.empty((total, 3), dtype=torch.float64, device=dev)
    succ, pred = (torch.empty((total,), dtype=torch.int32, device=dev) for _ in range(2))

    def write():
        L.check(lib.prh_trace_peaks_write(G.ptr(ws), nb, n_s, nx, ny, *peak, G.ptr(col_off), total, 0, G.ptr(iy), G.ptr(weight),
                                          G.ptr(cnt), G.ptr(xyz), G.ptr(col), dev.index, G.stream(dev)), "write")

    def links():
        L.check(lib.prh_trace_link(G.ptr(col_off), n_s * nx, nx, G.ptr(iy), G.ptr(col), total, p["link_cells"], p["gap_slope"],
                                   p["max_gap_cols"], G.ptr(succ), G.ptr(pred), dev.index, G.stream(dev)), "link")

    res["peaks_write"] = stat(events_ms(write, args.reps))
    res["link"] = stat(events_ms(links, args.reps))
    host = [a.cpu().numpy() for a in (xyz, col, succ, pred)]
    chains = []
    for _ in range(args.reps):
        t = time.perf_counter()
        lines, dropped = T.chain_lines(*host, n_s, nx)
        chains.append((time.perf_counter() - t) * 1e3)
    res["chains_host"] = stat(chains)
    res["paint_peaks_f64"] = median_wall(lambda: T.paint_peaks(p64, off, intensity_floor=FLOOR))
    res["trace_lines_f64"] = median_wall(lambda: T.trace_lines(p64, off, intensity_floor=FLOOR))
    a, b = T.paint_peaks(p64, off, intensity_floor=FLOOR), T.paint_peaks(p32, off, intensity_floor=FLOOR)
    equal = all(torch.equal(a[k].view(torch.int64) if a[k].dtype == torch.float64 else a[k],
                            b[k].view(torch.int64) if b[k].dtype == torch.float64 else b[k]) for k in a)
    bright = int(a["bright_points"].item())
    one = p64[:n_pts].cpu().numpy()
    t = time.perf_counter()
    TC.paint_peaks_np(one, np.array([0, n_pts]), intensity_floor=FLOOR)
    numpy_ms = (time.perf_counter() - t) * 1e3
    del p64, p32, ws

    # ---- whole: one generated drive directory through both tools
    from oracle import procedural as P
    from pointnet_refine_amd.model import LineRefineNet
    model = LineRefineNet()
    model.load_state_dict(P.linerefine_state_dict(0))
    model = model.cuda().eval()
    with tempfile.TemporaryDirectory() as root:
        drive, results, n_cloud = write_drive(root, args.drive_length, 500.0, 300.0)
        rc = T.refine_cloud(model, drive, intensity_floor=FLOOR, batched=True)
        rp = link.refine_predictions(model, drive, results, batched=True)
        whole = {"refine_cloud": median_wall(lambda: T.refine_cloud(model, drive, intensity_floor=FLOOR, batched=True)),
                 "refine_predictions": median_wall(lambda: link.refine_predictions(model, drive, results, batched=True))}
    whole.update(cloud_points=n_cloud, cloud_slices=rc["report"]["slices"], cloud_pieces=rc["report"]["pieces"],
                 cloud_clusters=rc["report"]["clusters_kept"], pred_slices=rp["report"]["slices"],
                 pred_pieces=rp["report"]["pieces"], pred_clusters=rp["report"]["clusters_kept"],
                 trace=[rc["report"][k] for k in ("trace_bright_points", "trace_peaks", "trace_lines")])

    n = n_s * n_pts
    out = {"device": torch.cuda.get_device_name(0), "slices": n_s, "points_per_slice": n_pts, "lanes": args.lanes,
           "reps": args.reps, "nx": nx, "ny": ny, "table_bytes": int(nb), "bright_points": bright, "peaks": total,
           "links": int((host[2] >= 0).sum()), "lines": int(sum(len(ls) for ls in lines)), "chains_dropped": dropped,
           "f32_equals_f64": bool(equal), "results": res, "numpy_one_slice_ms": numpy_ms,
           "numpy_scaled_ms": numpy_ms * n_s, "whole": whole}

    def row(key, label, nbytes=None):
        v = res[key]
        tail = ""
        if nbytes is not None:
            floor_ms = nbytes / HBM_BYTES_PER_S * 1e3
            tail = (f"   must read {nbytes / 1e6:.0f} MB: {floor_ms:.3f} ms at 5 TB/s, {100.0 * floor_ms / v['ms']:.1f} % of that "
                    f"rate reached")
        return f"  {label:<46} runs (ms) {v['runs']} median {v['ms']:.3f}{tail}"

    text = f"""Paint tracing: lane candidates from the bright ridges of every slice's cloud (prh_trace_hist, prh_trace_peaks_count,
prh_trace_peaks_write, prh_trace_link; trace.paint_peaks, trace.chain_lines, trace.refine_cloud).
Command: python scripts/paint_trace_bench.py   (--slices {n_s} --points-per-slice {n_pts} --lanes {args.lanes} --drive-length {args.drive_length:g} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, one process, {time.strftime('%Y-%m-%d')}.
Timing: device events around the call, median of {args.reps} after one warm-up call, unless a row says wall clock.

Generated slices: {n_s} x {n_pts} = {n} points, a twentieth of them paint in {args.lanes} bands, intensity_floor {FLOOR:g}; grid {nx} x {ny},
tables {nb / 1e6:.1f} MB in one chunk; {bright} bright points, {total} peaks, {out['links']} links, {out['lines']} lines
({dropped} chains left out); paint_peaks on float32 points bitwise equal to float64: {equal}.
{row('hist_f64', 'prh_trace_hist, float64 (memset included)', n * 32)}
{row('hist_f32', 'prh_trace_hist, float32 (memset included)', n * 16)}
{row('memset', 'the tables zeroed on their own (torch)')}
{row('bev_maps_f64', 'bev.bev_maps, float64, same points, 0.05 m', n * 32)}
{row('peaks_count', 'prh_trace_peaks_count')}
{row('peaks_write', 'prh_trace_peaks_write')}
{row('link', 'prh_trace_link')}
{row('chains_host', 'trace.chain_lines, host, wall clock')}
{row('paint_peaks_f64', 'trace.paint_peaks whole, wall clock')}
{row('trace_lines_f64', 'trace.trace_lines whole, wall clock')}
  numpy restatement (tests/_trace_cases.paint_peaks_np), one slice, wall clock: {numpy_ms:.1f} ms; times {n_s} slices = {numpy_ms * n_s:.0f} ms
  (scaled from one slice, not measured)

Whole, one generated drive directory ({n_cloud} points, {args.drive_length:g} m, poses 25 m apart), batched contexts, wall clock (ms),
merged.pcd read and parsed inside both calls; procedural weights, so the maps say nothing about accuracy:
  trace.refine_cloud         runs {whole['refine_cloud']['runs']} median {whole['refine_cloud']['ms']:.1f}   {whole['cloud_slices']} slices, {whole['trace'][0]} bright points, {whole['trace'][1]} peaks, {whole['trace'][2]} traced lines, {whole['cloud_pieces']} pieces, {whole['cloud_clusters']} clusters
  link.refine_predictions    runs {whole['refine_predictions']['runs']} median {whole['refine_predictions']['ms']:.1f}   {whole['pred_slices']} frames, {whole['pred_pieces']} pieces, {whole['pred_clusters']} clusters

{json.dumps(out)}
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
