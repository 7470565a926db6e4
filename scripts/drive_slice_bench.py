"""Times the drive slicer (csrc/prh_drive.hpp) on a generated drive: P cloud points along a path of
S slices (25 m apart, UTM-sized coordinates) and a few hundred GT polylines.  Prints one JSON line:

  upload_ms            host -> device copy of the cloud (16 B per point)
  slice_ms             slice_cloud on the resident cloud (count pass, scans, write pass), device events
  clip_ms              clip_lines, wall clock (it returns host arrays)
  gpu_total_ms         upload + slice + clip
  slice_gbps           algorithmic bytes / slice_ms: 16 B per point per pass, two passes, plus 40 B
                       per emitted point (4 fp64 + the int64 source index)
  host_ms              the reference's per-slice loop restated in numpy (float32 radius mask, gather,
                       fp64 rotation, x-crop, and the polyline clip) on --host-slices slices spread
                       over the drive, run on --threads threads, scaled to S slices
  speedup              host_ms / gpu_total_ms

    python scripts/drive_slice_bench.py [--points 20000000] [--slices 80] [--lines 200] [--json OUT]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_drive(n_points, n_slices, n_lines, seed=0):
    rng = np.random.default_rng(seed)
    origin = np.array([4.0e5, 5.0e6, 30.0])
    px = origin[0] + 25.0 * np.arange(1, n_slices + 1)
    py = origin[1] + 10.0 * np.sin(px / 80.0)
    yaw = np.arctan2(np.gradient(py), np.gradient(px)) + rng.normal(0, 0.02, n_slices)
    q = np.stack([np.zeros(n_slices), np.zeros(n_slices), np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    poses = np.column_stack([px, py, np.full(n_slices, origin[2]), q])
    length = 25.0 * (n_slices + 1)
    x = rng.uniform(-30, length + 30, n_points).astype(np.float32) + np.float32(origin[0])
    cloud = np.empty((n_points, 4), dtype=np.float32)
    cloud[:, 0] = x
    cloud[:, 1] = origin[1] + rng.uniform(-50, 50, n_points)
    cloud[:, 2] = origin[2] + rng.uniform(-2, 8, n_points)
    cloud[:, 3] = rng.uniform(0, 255, n_points)
    lines = []
    for k in range(n_lines):
        a = rng.uniform(0, length - 100)
        xs = origin[0] + np.linspace(a, a + rng.uniform(60, 400), int(rng.integers(20, 200)))
        lines.append(np.column_stack([xs, origin[1] + 10.0 * np.sin(xs / 80.0) + 3.5 * (k % 7 - 3),
                                      np.full_like(xs, origin[2])]))
    return cloud, poses, lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=20_000_000)
    ap.add_argument("--slices", type=int, default=80)
    ap.add_argument("--lines", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-slices", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    import test_drive_cpu as R
    from pointnet_refine_amd import drive
    if not torch.cuda.is_available():
        raise SystemExit("drive_slice_bench.py needs a GPU")
    cloud, poses, lines = make_drive(args.points, args.slices, args.lines)
    dev = torch.device("cuda")
    host = torch.from_numpy(cloud)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    cl = host.to(dev)                                                 # warm-up: allocator, library load, kernels
    drive.slice_cloud(cl, poses)
    drive.clip_lines(lines, poses)
    torch.cuda.synchronize()
    up, sl, cp = [], [], []
    for _ in range(args.reps):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        cl = host.to(dev)
        e1.record()
        pts, off, idx = drive.slice_cloud(cl, poses)
        e2.record()
        torch.cuda.synchronize()
        t = time.perf_counter()
        drive.clip_lines(lines, poses)
        cp.append((time.perf_counter() - t) * 1e3)
        up.append(e0.elapsed_time(e1)); sl.append(e1.elapsed_time(e2))
    emitted = int(off[-1].item())
    upload_ms, slice_ms, clip_ms = float(np.median(up)), float(np.median(sl)), float(np.median(cp))
    byts = 2 * 16.0 * args.points + 40.0 * emitted

    pick = np.unique(np.linspace(0, args.slices - 1, min(args.host_slices, args.slices)).astype(int))

    def one(s):
        R.slice_ref(cloud, poses[s:s + 1])
        R.clip_lines_ref(lines, poses[s:s + 1])

    t = time.perf_counter()
    with ThreadPoolExecutor(args.threads) as ex:
        list(ex.map(one, pick))
    host_ms = (time.perf_counter() - t) * 1e3 * args.slices / len(pick)
    total = upload_ms + slice_ms + clip_ms
    out = {"device": torch.cuda.get_device_name(0), "points": args.points, "slices": args.slices, "lines": args.lines,
           "emitted_points": emitted, "reps": args.reps, "upload_ms": round(upload_ms, 3),
           "slice_ms": round(slice_ms, 3), "slice_ms_all": [round(v, 3) for v in sl], "clip_ms": round(clip_ms, 3),
           "gpu_total_ms": round(total, 3), "algorithmic_bytes": byts, "slice_gbps": round(byts / slice_ms / 1e6, 1),
           "host_ms": round(host_ms, 1), "host_slices_timed": len(pick), "host_threads": args.threads,
           "speedup": round(host_ms / total, 1)}
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
