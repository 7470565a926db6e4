"""Times cloud support (csrc/prh_support.hpp, pointnet_refine_amd/support.py) and writes a report
(default profiles/r14_cloud_support_bench.txt) that ends in one JSON line:

  kernel_ms          prh_support_accumulate on resident buffers, device events: --points cloud points
                     against the --lines lines of a generated --slices slice drive, next to the
                     bytes it must read (16 per point) and the spec-derived floor for them
  bev_map_ms         bev.bev_map over the same cloud in the same process: the other one-pass reader
  kernel_no_hits_ms  the same launch with the lines lifted 100 m in z: the same cells, lists and
                     projections and not one hit, so the difference is what the atomics cost
  hits, atomics      hits, 64-bit atomic adds and their bytes per second
  grid_build_ms      support.segment_grid on the host
  node_support_ms    the whole call on a resident cloud (grid, uploads, kernel, download, derive)
  refine_drive_*     fuse.refine_drive(batched=True) with and without support=True, wall clock
  numpy_ms_scaled    tests/_support_oracle.support_numpy (vectorised over points, every segment for
                     every point) on the first --numpy-share of the points, SCALED by points

    python scripts/support_bench.py [--points 20000000] [--slices 80] [--lines 6] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HBM_BYTES_PER_S = 5.0e12        # a spec-derived figure, not measured for this access pattern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--slices", type=int, default=80)
    ap.add_argument("--lines", type=int, default=6)
    ap.add_argument("--drive-cloud-points", type=int, default=4_000_000)
    ap.add_argument("--numpy-share", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_cloud_support_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("support_bench.py needs a GPU")
    import _support_oracle as O
    from map_fusion_bench import events_ms, make_drive, wall_ms
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    from pointnet_refine_amd import bev, fuse
    from pointnet_refine_amd import support as S
    dev = G.device("support")
    lib = L.lib()
    rng = np.random.default_rng(0)
    cloud, poses, lines = make_drive(args.points, args.slices, args.lines, rng)
    pts = torch.from_numpy(cloud).to(dev)
    step, radius, floor = S.STEP, S.RADIUS, 20.0
    org = np.zeros(3)

    # ---- the kernel on resident buffers
    cums = [fuse.carrier_cum(v) for v in lines]
    counts = np.array([int(np.floor(c[-1] / step)) + 1 for c in cums], dtype=np.int64)
    node_off = np.concatenate(([0], np.cumsum(counts)))
    n_nodes = int(node_off[-1])
    t = time.perf_counter()
    grid = S.segment_grid(lines, radius, S.CELL)
    grid_ms = (time.perf_counter() - t) * 1e3
    verts, off_t, _ = G.lines_csr(lines, dev)
    cum_t = torch.from_numpy(np.concatenate(cums)).to(dev)
    no_t = torch.from_numpy(node_off).to(dev)
    co_t = torch.from_numpy(grid["cell_offsets"]).to(dev)
    en_t = torch.from_numpy(grid["entries"]).to(dev)
    acc = torch.zeros((n_nodes, S.COLS), dtype=torch.int64, device=dev)

    def kernel():
        L.check(lib.prh_support_accumulate(
            G.ptr(pts), pts.shape[0], 0.0, 0.0, 0.0, grid["x0"], grid["y0"], grid["cell"], grid["nx"], grid["ny"],
            G.ptr(co_t), G.ptr(en_t), len(grid["entries"]), G.ptr(verts), G.ptr(off_t), G.ptr(cum_t), len(lines),
            G.ptr(no_t), n_nodes, step, radius * radius, floor, G.ptr(acc), dev.index, G.stream(dev)),
            "prh_support_accumulate")

    kernel_all = events_ms(kernel, args.reps)                  # acc keeps growing: the work per run is the same
    # the same launch with the lines lifted 100 m: the same cells, lists and projections, not one hit
    lifted, _, _ = G.lines_csr([v + [0.0, 0.0, 100.0] for v in lines], dev)
    verts, flat_verts = lifted, verts
    no_hit_all = events_ms(kernel, args.reps)
    verts = flat_verts
    no_hit_ms = float(np.median(no_hit_all))
    acc.zero_()
    kernel()
    acc_h = acc.cpu().numpy()
    hits, paint = int(acc_h[:, 0].sum()), int(acc_h[:, 1].sum())
    atomics = 4 * hits + 3 * paint                             # count, qt, qt^2, qz; painted count, qi, qi qt
    kernel_ms = float(np.median(kernel_all))
    read_bytes = 16.0 * args.points
    floor_ms = read_bytes / HBM_BYTES_PER_S * 1e3
    per_cell = np.diff(grid["cell_offsets"])
    bev_all = events_ms(lambda: bev.bev_map(pts), args.reps)
    bev_ms = float(np.median(bev_all))
    node_ms, node = wall_ms(lambda: S.node_support(pts, lines, step, radius, floor, origin=org))
    assert np.array_equal(node["acc"], acc_h)

    # ---- the numpy restatement on a share of the points, scaled
    n_np = max(int(args.points * args.numpy_share), 1)
    t = time.perf_counter()
    acc_np, _ = O.support_numpy(cloud[:n_np], lines, step, radius, floor, origin=org)
    numpy_ms = (time.perf_counter() - t) * 1e3
    part = S.node_support(pts[:n_np], lines, step, radius, floor, origin=org)["acc"]
    numpy_equal = bool(np.array_equal(acc_np, part))

    # ---- refine_drive with and without support
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    model = LineRefineNet()
    model.load_state_dict(P.linerefine_state_dict(0))
    model = model.cuda().eval()
    dcloud, dposes, dlines = make_drive(args.drive_cloud_points, args.slices, args.lines, rng)
    cl = torch.from_numpy(dcloud).to(dev)
    fuse.refine_drive(model, cl, dposes, dlines, batched=True, support=True, intensity_floor=floor)      # warm-up
    plain_ms, _ = wall_ms(lambda: fuse.refine_drive(model, cl, dposes, dlines, batched=True))
    with_ms, res = wall_ms(lambda: fuse.refine_drive(model, cl, dposes, dlines, batched=True, support=True,
                                                     intensity_floor=floor))
    sup = res["support"]

    out = {"device": torch.cuda.get_device_name(0), "points": args.points, "lines": len(lines),
           "segments": int(sum(len(v) - 1 for v in lines)), "nodes": n_nodes, "reps": args.reps,
           "grid_cells": grid["nx"] * grid["ny"], "grid_cell_m": grid["cell"], "grid_entries": int(len(grid["entries"])),
           "grid_cells_used": int((per_cell > 0).sum()), "grid_mean_list": round(float(per_cell[per_cell > 0].mean()), 2),
           "grid_max_list": int(per_cell.max()), "grid_build_ms": round(grid_ms, 2),
           "kernel_ms": round(kernel_ms, 3), "kernel_ms_all": [round(v, 3) for v in kernel_all],
           "kernel_no_hits_ms": round(no_hit_ms, 3),
           "kernel_no_hits_ms_all": [round(v, 3) for v in no_hit_all], "read_bytes": read_bytes, "read_floor_ms": round(floor_ms, 4), "kernel_over_floor": round(kernel_ms / floor_ms, 1),
           "read_bytes_per_s": read_bytes / (kernel_ms * 1e-3), "hits": hits, "hit_share": round(hits / args.points, 4),
           "largest_node": int(acc_h[:, 0].max()), "atomics": atomics, "atomic_bytes": 8 * atomics,
           "hits_per_s": hits / (kernel_ms * 1e-3), "atomic_bytes_per_s": 8 * atomics / (kernel_ms * 1e-3),
           "bev_map_ms": round(bev_ms, 3), "bev_map_ms_all": [round(v, 3) for v in bev_all],
           "node_support_ms": round(node_ms, 2), "numpy_points": n_np, "numpy_ms_measured": round(numpy_ms, 0),
           "numpy_ms_scaled": round(numpy_ms * args.points / n_np, 0), "numpy_equal": numpy_equal,
           "drive_cloud_points": args.drive_cloud_points, "drive_slices": res["report"]["slices"],
           "drive_pieces": res["report"]["pieces"], "refine_drive_batched_ms": round(plain_ms, 1),
           "refine_drive_batched_support_ms": round(with_ms, 1),
           "drive_input_supported_share": round(sup["input"]["supported_share"], 4),
           "drive_fused_supported_share": round(sup["fused"]["supported_share"], 4)}
    text = f"""Cloud support: prh_support_accumulate on a generated drive, support.node_support, fuse.refine_drive with and without support.
Command: python scripts/support_bench.py   (--points {args.points} --slices {args.slices} --lines {args.lines} --drive-cloud-points {args.drive_cloud_points} --numpy-share {args.numpy_share} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, {time.strftime('%Y-%m-%d')}.
Timing: device events around the library call on resident buffers, median of {args.reps} after one warm-up call; node_support,
the grid build and refine_drive by wall clock around synchronised calls (refine_drive after one warm-up run).
The read floor is 16 bytes per point at 5 TB/s, a spec-derived figure nobody has measured for this access pattern.

{json.dumps(out)}

support kernel runs (ms): {[round(v, 3) for v in kernel_all]}
no-hit runs (ms):         {[round(v, 3) for v in no_hit_all]}
bev_map runs (ms):        {[round(v, 3) for v in bev_all]}
support kernel: {args.points} points ({read_bytes / 1e6:.0f} MB) against {out['segments']} segments / {n_nodes} stations in {kernel_ms:.3f} ms
= {out['read_bytes_per_s'] / 1e12:.2f} TB/s of cloud read, {out['kernel_over_floor']} x the {floor_ms * 1e3:.0f} us read floor; bev_map over the same cloud: {bev_ms:.3f} ms.
grid: {out['grid_cells']} cells of {grid['cell']} m, {out['grid_cells_used']} with a list, {out['grid_entries']} entries, mean list {out['grid_mean_list']}, longest {out['grid_max_list']}; built on the host in {grid_ms:.2f} ms.
hits: {hits} ({100.0 * hits / args.points:.2f} % of the points, largest node {out['largest_node']}), {atomics} 64-bit atomic adds = {8 * atomics / 1e6:.1f} MB:
{out['hits_per_s']:.3g} hits/s, {out['atomic_bytes_per_s'] / 1e9:.1f} GB/s of added bytes.
the same launch without a hit (lines lifted 100 m: same cells, lists and projections): {no_hit_ms:.3f} ms, so the atomics cost
{kernel_ms - no_hit_ms:.3f} ms of the {kernel_ms:.3f} ms = {8 * atomics / max(kernel_ms - no_hit_ms, 1e-9) / 1e6:.1f} GB/s of added bytes while they run.
node_support on the resident cloud (grid, uploads, kernel, download, derived arrays): {node_ms:.2f} ms.
numpy restatement (vectorised over points, every segment for every point): {numpy_ms:.0f} ms for the first {n_np} points,
equal to the kernel on them: {numpy_equal}; SCALED by points to {args.points}: {numpy_ms * args.points / n_np / 1e3:.0f} s (an estimate, not a measurement of that size).
refine_drive(batched=True), {res['report']['slices']} slices, {args.drive_cloud_points} cloud points, {len(dlines)} lines, {res['report']['pieces']} pieces: {plain_ms:.1f} ms without,
{with_ms:.1f} ms with support=True (input and fused map scored: {100.0 * sup['input']['supported_share']:.1f} % of the input's stations and {100.0 * sup['fused']['supported_share']:.1f} % of the
fused map's are supported; procedural weights move the lines off the ground, so the second figure says nothing about accuracy).
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
