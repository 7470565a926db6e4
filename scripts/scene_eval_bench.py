"""Times the scene-evaluation kernels (csrc/prh_metrics.hpp) on one synthetic scene of the size
the issue names: L lines, each with a raw noisy candidate of V vertices (resampled to 32 points)
and a GT polyline of GV vertices.  Prints one JSON line:

  metric_ms / metric_rows_per_s   line_metrics over all L lines (device time, synchronised)
  sweep_ms                        one shift_sweep launch of 600 shifts (P = L*V, G = L*GV)
  calibrate_ms                    calibrate_alignment (coarse 400 + fine ~200 shifts)
  sweep_pairs_per_s               P*G*600 / sweep time
  sweep_fp64_share                fp64 VALU instructions issued (SWEEP_OPS_PER_PAIR from the ISA)
                                  over the spec rate, FP64_LANE_OPS_PER_S - a spec figure, not measured
  host_*                          the same work through scipy KDTree on the host (the reference's
                                  method), when scipy imports; --no-host skips it

    python scripts/scene_eval_bench.py [--lines 256] [--verts 64] [--gt-verts 200] [--json OUT]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# met_sweep_kernel's inner loop issues 244 fp64 VALU instructions (130 add, 66 mul, 32 min,
# 16 max) per 2 GT points x 16 shifts: 7.625 per (query, GT point, shift) pair
SWEEP_OPS_PER_PAIR = 244 / 32
# MI355X spec fp64 vector rate, 78.6 TFLOP/s counting an FMA as 2: 39.3e12 lane-instructions/s
FP64_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9


def scene(L, V, GV, seed=0):
    rng = np.random.default_rng(seed)
    origin = np.array([4.0e5, 5.0e6, 30.0])
    gts, raws = [], []
    for i in range(L):
        row, col = divmod(i, 16)
        x0 = 120.0 * col
        xg = x0 + np.sort(rng.uniform(0, 100, GV))
        gts.append(np.stack([xg, 3.5 * row + 0.3 * np.sin(xg / 20.0), rng.normal(0, 0.02, GV)], 1) + origin)
        a, b = np.sort(rng.uniform(x0, x0 + 100, 2))
        xv = np.linspace(a, b, V)
        raws.append(np.stack([xv, 3.5 * row + 0.3 * np.sin(xv / 20.0) + rng.normal(0.3, 0.05, V),
                              rng.normal(0, 0.05, V)], 1) + origin)
    return gts, raws


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3, out


def host_times(gts, raws, noisy, refined, max_s=600):
    from scipy.spatial import KDTree
    t = time.perf_counter()
    for g, nz, rf in zip(gts, noisy, refined):        # crop + 4 KDTree builds / queries per line
        ds, de = np.linalg.norm(g - nz[0], axis=1), np.linalg.norm(g - nz[-1], axis=1)
        a, b = sorted((int(np.argmin(ds)), int(np.argmin(de))))
        crop = g[a:b + 1]
        for line in (nz, rf):
            KDTree(crop).query(line)
            KDTree(line).query(crop)
    metric_ms = (time.perf_counter() - t) * 1e3
    pred, gt = np.vstack(raws), np.vstack(gts)
    tree = KDTree(gt)
    n = 20                                              # time 20 shifts, scale to the sweep's 600
    t = time.perf_counter()
    for k in range(n):
        np.mean(tree.query(pred + np.array([0.1 * k, 0.05 * k, 0]))[0])
    sweep_ms = (time.perf_counter() - t) * 1e3 / n * max_s
    return metric_ms, sweep_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=256)
    ap.add_argument("--verts", type=int, default=64)
    ap.add_argument("--gt-verts", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    from pointnet_refine_amd.context import resample_polyline
    from pointnet_refine_amd.metrics import calibrate_alignment, line_metrics, shift_sweep
    if not torch.cuda.is_available():
        raise SystemExit("scene_eval_bench.py needs a GPU")
    gts, raws = scene(args.lines, args.verts, args.gt_verts)
    noisy = np.stack([resample_polyline(r, 32) for r in raws])
    refined = noisy + np.random.default_rng(1).normal(0, 0.05, noisy.shape)
    dev = torch.device("cuda")
    nz_t, rf_t = torch.from_numpy(noisy).to(dev), torch.from_numpy(refined).to(dev)
    metric_ms, res = timed(lambda: line_metrics(nz_t, rf_t, gts), args.reps)
    pred, gt = np.vstack(raws), np.vstack(gts)
    pred_t, gt_t = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    shifts = np.array([(dx, dy) for dx in np.arange(-20, 20, 2.0) for dy in np.arange(-10, 10, 1.0)]
                      + [(0.2 * i - 2.0, 0.2 * j - 1.0) for i in range(20) for j in range(10)])
    sweep_ms, _ = timed(lambda: shift_sweep(pred_t, gt_t, shifts), args.reps)
    cal_ms, cal = timed(lambda: calibrate_alignment(raws, gts), args.reps)
    pairs = float(len(pred)) * len(gt) * len(shifts)
    out = {"lines": args.lines, "pred_points": len(pred), "gt_points": len(gt), "shifts": len(shifts),
           "metric_ms": round(metric_ms, 3), "metric_rows_per_s": round(args.lines / metric_ms * 1e3, 1),
           "sweep_ms": round(sweep_ms, 3), "calibrate_ms": round(cal_ms, 3),
           "sweep_pairs_per_s": pairs / sweep_ms * 1e3,
           "sweep_fp64_share": round(pairs * SWEEP_OPS_PER_PAIR / (sweep_ms * 1e-3) / FP64_LANE_OPS_PER_S, 3),
           "calibration": [float(cal[0][0]), float(cal[0][1]), float(cal[1])],
           "valid_rows": int(res["valid"].sum()), "mean_lat_noisy": float(np.nanmean(res["lat_noisy"]))}
    if not args.no_host:
        try:
            hm, hs = host_times(gts, raws, noisy, refined, len(shifts))
            out.update(host_metric_ms=round(hm, 1), host_sweep_ms_est=round(hs, 1),
                       host_threads=1, host_sweep_note="20 KDTree queries timed, scaled to the shift count")
        except ImportError:
            out["host"] = "scipy not importable"
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
