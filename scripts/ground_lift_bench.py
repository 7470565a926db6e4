"""Times the ground lift (csrc/prh_ground.hpp, pointnet_refine_amd/ground.py) on the detector-run-
sized input of scripts/link_sync_bench.py - 2,000 frames x 12 lines, stations every metre - and
writes a report (default profiles/r17_ground_lift_bench.txt) that ends in one JSON line:

  bin_ms              prh_ground_bin_count + the scan + prh_ground_bin_write (device events)
  query_ms            prh_ground_query (device events), next to the bytes it reads - rows, x y of every
                      row of the walked cells, z of every hit, twice - and their time at 5 TB/s
  stations_ms, lift_ms   line_stations and lift_vertices on the host (wall clock)
  numpy_frame_ms      the numpy restatement of the rule (tests/test_ground_cpu.py) on ONE frame;
                      numpy_scaled_s is that figure times the number of frames: scaled, not measured
  refine_*_ms         link.refine_predictions(batched=True) without and with lift on a generated
                      drive of --e2e-frames frames whose road is at ego z = 0, so that both runs
                      refine every line and the difference is the lift

Every frame's slice is a synthetic road (a pitched plane 1.7 m below the pose with 2 cm noise) of
--points-per-frame float64 points over the 50 m x 46 m the lines cover, generated on the device.

    python scripts/ground_lift_bench.py [--frames 2000] [--lanes 12] [--points-per-frame 50000] [--out FILE]
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


def walked_rows(q, qoff, grids, cell_off):
    """Rows of `rows` the query kernel visits in one sweep: per query the cells between those of q -
    reach and q + reach, clipped to the grid - the kernel's expressions, in numpy."""
    s = np.repeat(np.arange(len(qoff) - 1), np.diff(qoff))
    org, shape, base = grids["origin"][s], grids["shape"][s].astype(np.int64), grids["cell_base"][s]
    lo = np.maximum(np.floor(((q - grids["reach"]) - org) / grids["cell"]), 0).astype(np.int64)
    hi = np.minimum(np.floor(((q + grids["reach"]) - org) / grids["cell"]), shape - 1).astype(np.int64)
    total = np.zeros(len(q), dtype=np.int64)
    for k in range(int((hi[:, 1] - lo[:, 1]).max()) + 1):
        iy = lo[:, 1] + k
        ok = iy <= hi[:, 1]
        row0 = base + np.where(ok, iy, 0) * shape[:, 0]
        total += np.where(ok, cell_off[row0 + hi[:, 0] + 1] - cell_off[row0 + lo[:, 0]], 0)
    return int(total.sum())


def write_flat_drive(root, n_frames, n_lanes, rng):
    """A straight drive with the road at ego z = 0: poses 2.5 m apart, lanes 3.5 m apart, 30 points / m^2."""
    import _fuse_oracle as O
    from pointnet_refine_amd.pcd import write_pcd_host
    os.makedirs(os.path.join(root, "pose"))
    length, half = 2.5 * n_frames + 60.0, 1.75 * n_lanes + 2.0
    n = int(30 * length * 2 * half)
    cloud = np.column_stack([rng.uniform(-30.0, length - 30.0, n), rng.uniform(-half, half, n), rng.normal(0.0, 0.02, n),
                             rng.uniform(0.0, 60.0, n)])
    write_pcd_host(os.path.join(root, "merged.pcd"), cloud)
    results = {}
    for k in range(n_frames):
        ts = 1000 + k
        pose = np.array([2.5 * k, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
        json.dump({"ts": str(ts), "x": pose[0], "y": pose[1], "z": pose[2], "qx": 0.0, "qy": 0.0, "qz": 0.0, "qw": 1.0},
                  open(os.path.join(root, "pose", f"{ts}.json"), "w"))
        inst = []
        for l in range(n_lanes):
            x = np.linspace(-24.0, 24.0, 13)
            ego = O.to_ego(np.column_stack([pose[0] + x, np.full(13, 3.5 * (l - (n_lanes - 1) / 2)), np.zeros(13)]), pose)
            inst.append({"data": np.stack([(25.0 - ego[:, 1]) / 0.05, (25.0 - ego[:, 0]) / 0.05], 1).tolist(), "score": 0.9})
        results[f"cam/{ts}.jpg"] = {"pred_instances": inst}
    json.dump(results, open(os.path.join(root, "results.json"), "w"))
    return len(cloud)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--lanes", type=int, default=12)
    ap.add_argument("--points-per-frame", type=int, default=50000)
    ap.add_argument("--e2e-frames", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_ground_lift_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ground_lift_bench.py needs a GPU")
    from link_bench import events_ms, make_run, wall_ms
    from test_ground_cpu import restate
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import ground as GR
    from pointnet_refine_amd import link
    dev = G.device("ground")

    def median_wall(fn):
        fn()
        runs = [wall_ms(fn)[0] for _ in range(args.reps)]
        return float(np.median(runs)), [round(v, 3) for v in runs]

    # ---- the run of link_bench.py: its pieces are the lines, flattened to z = 0 as the detector gives them
    pieces, frame, _ = make_run(args.frames, args.lanes, np.random.default_rng(0))
    pieces[:, :, 2] = 0.0
    lines = [list(pieces[f * args.lanes:(f + 1) * args.lanes]) for f in range(args.frames)]
    flat = [l for ls in lines for l in ls]
    n_pts = args.points_per_frame
    gen = torch.Generator(device=dev).manual_seed(0)
    points = torch.empty((args.frames * n_pts, 4), dtype=torch.float64, device=dev)
    points[:, 0] = torch.rand(len(points), generator=gen, device=dev, dtype=torch.float64) * 52.0 - 26.0
    points[:, 1] = torch.rand(len(points), generator=gen, device=dev, dtype=torch.float64) * 46.0 - 23.0
    points[:, 2] = -1.7 + 0.02 * points[:, 0] + 0.02 * torch.randn(len(points), generator=gen, device=dev, dtype=torch.float64)
    points[:, 3] = 0.0
    off = np.arange(args.frames + 1, dtype=np.int64) * n_pts

    stations_ms, stations_all = median_wall(lambda: GR.line_stations(flat, 1.0))
    xy, arc, s_off = GR.line_stations(flat, 1.0)
    qoff = s_off[np.arange(args.frames + 1) * args.lanes]
    params = GR._params(GR.RADIUS, GR.MIN_POINTS, GR.PEAK_SHARE, GR.Z_LO, GR.BIN, GR.N_BINS, "bench")
    grids = GR.slice_grids(xy, qoff, GR.RADIUS, GR.RADIUS)
    off_t, q_t, qoff_t = torch.from_numpy(off).to(dev), torch.from_numpy(xy).to(dev), torch.from_numpy(qoff).to(dev)
    bin_all = events_ms(lambda: GR.bin_points(points, off_t, grids, dev), args.reps)
    cell_off, rows, g_t = GR.bin_points(points, off_t, grids, dev)
    query_all = events_ms(lambda: GR.query_heights(points, off_t, q_t, qoff_t, grids, g_t, cell_off, rows, params, dev), args.reps)
    res = GR.query_heights(points, off_t, q_t, qoff_t, grids, g_t, cell_off, rows, params, dev)
    height, hits = res["height"].cpu().numpy(), res["hits"].cpu().numpy()
    lift_ms, lift_all = median_wall(lambda: GR.lift_vertices(flat, arc, s_off, height))
    whole_ms, whole_all = median_wall(lambda: GR.lift_lines(points, off_t, lines))
    lifted, report = GR.lift_lines(points, off_t, lines)
    plane_err = max(float(np.abs(l[:, 2] - (-1.7 + 0.02 * l[:, 0])).max()) for ls in lifted[:50] for l in ls)
    visited = walked_rows(xy, qoff, grids, cell_off.cpu().numpy())
    n_hits = int(hits.astype(np.int64).sum())
    q_bytes = 2 * (visited * (4 + 16) + n_hits * 8) + len(xy) * (16 + 4 * 8) + len(xy) * 20
    bin_ms, query_ms = float(np.median(bin_all)), float(np.median(query_all))

    # ---- numpy on one frame, scaled
    p0 = points[:n_pts].cpu().numpy()
    t = time.perf_counter()
    one = restate(p0, np.array([0, n_pts]), xy[:qoff[1]], np.array([0, qoff[1]]))
    numpy_frame_ms = (time.perf_counter() - t) * 1e3
    same = one["height"].tobytes() == height[:qoff[1]].tobytes() and one["hits"].tobytes() == hits[:qoff[1]].tobytes()

    # ---- refine_predictions on a flat drive, without and with lift
    n_rows = int(rows.shape[0])
    del points, rows, cell_off
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    model = LineRefineNet()
    model.load_state_dict(P.linerefine_state_dict(0))
    model = model.cuda().eval()
    with tempfile.TemporaryDirectory() as root:
        n_cloud = write_flat_drive(root, args.e2e_frames, args.lanes, np.random.default_rng(1))
        rj = os.path.join(root, "results.json")
        plain_ms, plain_all = median_wall(lambda: link.refine_predictions(model, root, rj, batched=True))
        lift_e2e_ms, lift_e2e_all = median_wall(lambda: link.refine_predictions(model, root, rj, batched=True, lift=True))
        rep_plain = link.refine_predictions(model, root, rj, batched=True)["report"]
        rep_lift = link.refine_predictions(model, root, rj, batched=True, lift=True)["report"]

    out = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "lanes": args.lanes, "points": int(off[-1]),
           "points_per_frame": n_pts, "stations": int(len(xy)), "cells": grids["n_cells"], "cell_m": grids["cell"],
           "binned_points": n_rows, "reps": args.reps,
           "bin_ms": round(bin_ms, 3), "query_ms": round(query_ms, 3), "query_bytes": q_bytes,
           "query_bytes_at_5TBs_ms": round(q_bytes / HBM_BYTES_PER_S * 1e3, 3), "rows_walked_per_sweep": visited, "hits": n_hits,
           "stations_ms": round(stations_ms, 1), "lift_ms": round(lift_ms, 1), "lift_lines_ms": round(whole_ms, 1),
           "stations_without_ground": report["stations_without_ground"], "max_plane_error_m": round(plane_err, 4),
           "numpy_frame_ms": round(numpy_frame_ms, 1), "numpy_scaled_s": round(numpy_frame_ms * args.frames / 1e3, 1),
           "numpy_frame_bitwise_equal": bool(same), "e2e_frames": args.e2e_frames, "e2e_cloud_points": n_cloud,
           "refine_plain_ms": round(plain_ms, 1), "refine_lift_ms": round(lift_e2e_ms, 1),
           "e2e_pieces_plain": rep_plain["pieces"], "e2e_pieces_lift": rep_lift["pieces"]}
    text = f"""Ground lift: the road height under every metre of every detector line, read from the frames' own slices
(prh_ground_bin_count, prh_ground_bin_write, prh_ground_query; ground.lift_lines).
Command: python scripts/ground_lift_bench.py   (--frames {args.frames} --lanes {args.lanes} --points-per-frame {n_pts} --e2e-frames {args.e2e_frames} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, one process, {time.strftime('%Y-%m-%d')}.
Timing: device events, median of {args.reps} after one warm-up call, for the bin and query stages; wall clock, median of
{args.reps} after one warm-up call, for the host stages and the whole calls.

{args.frames} frames x {args.lanes} lines, {len(xy)} stations (every metre), {int(off[-1])} float64 points ({n_pts} per frame), {grids['n_cells']} cells of {grids['cell']} m.
bin count + scan + write, runs (ms): {[round(v, 3) for v in bin_all]} median {bin_ms:.3f}
query kernel, runs (ms): {[round(v, 3) for v in query_all]} median {query_ms:.3f}
  it walks {visited} rows per sweep and finds {n_hits} hits: {q_bytes} B read (rows, x y, z of hits, twice; queries, grids, outputs),
  which take {q_bytes / HBM_BYTES_PER_S * 1e3:.3f} ms at 5 TB/s.
host: line_stations {stations_all} median {stations_ms:.1f} ms; lift_vertices {lift_all} median {lift_ms:.1f} ms
lift_lines whole (stations, upload, bin, query, copy, lift), runs (ms): {whole_all} median {whole_ms:.1f}
{report['stations_without_ground']} of {report['stations']} stations without ground; max |z - plane| over the first 50 frames' lines {plane_err:.4f} m.
numpy restatement on ONE frame ({qoff[1]} stations, {n_pts} points): {numpy_frame_ms:.1f} ms, bitwise equal to the device: {same};
  scaled by {args.frames} frames: {numpy_frame_ms * args.frames / 1e3:.1f} s (scaled, not measured).
refine_predictions(batched=True) on a flat generated drive ({args.e2e_frames} frames x {args.lanes} lines, {n_cloud} cloud points, road at ego z = 0,
  so both runs refine every line): without lift {plain_all} median {plain_ms:.1f} ms ({rep_plain['pieces']} pieces);
  with lift {lift_e2e_all} median {lift_e2e_ms:.1f} ms ({rep_lift['pieces']} pieces).

{json.dumps(out)}
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
