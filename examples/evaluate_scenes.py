"""Whole-scene evaluation (the metric half of the reference's inference_whole_scene.py, without the
plotly output): for every scene of DATA_DIR, refine every (item, candidate) line on the GPU and
print the reference's per-line lines, its SCENE CALIBRATION line and a summary.

    python examples/evaluate_scenes.py DATA_DIR [--checkpoint PATH] [--max-scenes 50]
                                       [--precision fp32|fp16] [--json OUT]
                                       [--batched [--max-points N]]

Without --checkpoint the model carries deterministic procedural weights (numbers then say
nothing about accuracy; the run exercises the path).  Summary: mean ADE / Lat before and after
over valid, non-bad-match rows, and the rows/s of the metric stage (line metrics + calibration).

--batched loads every scene first (the PCDs are parsed on the device) and makes ONE
metrics.evaluate_scenes call: one ragged context build and forward, one line-metric launch and two
ragged sweep launches for the whole data set; --max-points N bounds the cloud points held on the
device per forward group.  The printed lines and their order are the same.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("data_dir")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--max-scenes", type=int, default=50)
    ap.add_argument("--precision", choices=("fp32", "fp16"), default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--batched", action="store_true", help="one metrics.evaluate_scenes call for the whole set")
    ap.add_argument("--max-points", type=int, default=None, help="--batched: cloud points per forward group")
    args = ap.parse_args()

    from pointnet_refine_amd import io, metrics, pcd
    from pointnet_refine_amd.model import LineRefineNet
    model = LineRefineNet()
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
        print(f"Loaded model from {args.checkpoint}")
    else:
        from oracle import procedural as P
        model.load_state_dict(P.linerefine_state_dict(0))
        print("No checkpoint: procedural weights")
    model = model.cuda().eval()

    json_files = sorted(f for f in os.listdir(args.data_dir) if f.endswith(".json"))
    print(f"Found {len(json_files)} scenes. Processing top {args.max_scenes}...")
    per_scene, keep = [], {k: [] for k in ("ade_noisy", "ade_refined", "lat_noisy", "lat_refined")}
    metric_s, metric_rows = 0.0, 0

    def report(name, res):
        for r in range(len(res["item_index"])):
            if not res["valid"][r]:
                continue
            a, b = res["item_index"][r], res["candidate_index"][r]
            if res["bad_match"][r]:
                print(f"    Line {a}-{b} [SKIP METRIC]: Initial Lat {res['lat_noisy'][r]:.3f}m > 1.0m (Likely Wrong Match)")
            else:
                print(f"    Line {a}-{b}: ADE {res['ade_noisy'][r]:.3f}->{res['ade_refined'][r]:.3f} | "
                      f"Lat {res['lat_noisy'][r]:.3f}->{res['lat_refined'][r]:.3f}")
                for k in keep:
                    keep[k].append(float(res[k][r]))
        cal = res["calibration"]
        if cal is not None:
            (dx, dy), score = cal
            print(f"XXX SCENE CALIBRATION XXX: Best Offset (dx, dy) = ({dx:.2f}, {dy:.2f}) with MeanDist={score:.3f}")
        entry = {"scene": name, "rows": len(res["item_index"]), "valid": int(res["valid"].sum()),
                 "bad_match": int(res["bad_match"].sum()),
                 "calibration": None if cal is None else [float(cal[0][0]), float(cal[0][1]), float(cal[1])],
                 "calibration_refined": None if res["calibration_refined"] is None else
                 [float(res["calibration_refined"][0][0]), float(res["calibration_refined"][0][1]),
                  float(res["calibration_refined"][1])]}
        for k in ("ade_noisy", "ade_refined", "cd_noisy", "cd_refined", "lat_noisy", "lat_refined"):
            entry[k] = [None if np.isnan(v) else float(v) for v in res[k]]
        per_scene.append(entry)

    loaded = []                                  # --batched: (index, name, cloud on the device, items)
    for i, name in enumerate(json_files[:args.max_scenes]):
        json_path = os.path.join(args.data_dir, name)
        pcd_path = json_path.replace(".json", ".pcd")
        if not os.path.exists(pcd_path):
            print(f"PCD not found for {name}, skipping.")
            continue
        items = io.load_scene_items(json_path)
        if args.batched:
            loaded.append((i, name, pcd.read_pcd(pcd_path, device="cuda"), items))
            continue
        print(f"Processing Scene {i}: {name}")
        cloud = io.load_pcd_data(pcd_path)
        res = metrics.evaluate_scene(model, cloud, items, precision=args.precision)
        # metric stage alone, timed again on the scene's own rows (refined lines already known)
        rows, raw, gts, cal_gt = metrics.scene_rows(items)
        torch.cuda.synchronize()
        t = time.perf_counter()
        if rows:
            metrics.line_metrics(res["noisy"], res["refined"], gts, [-1 if g is None else r for r, g in enumerate(gts)])
        if raw and cal_gt:
            metrics.calibrate_alignment(raw, cal_gt)
        torch.cuda.synchronize()
        metric_s += time.perf_counter() - t
        metric_rows += len(rows)
        report(name, res)
    if args.batched:
        results = metrics.evaluate_scenes(model, [(cloud, items) for _, _, cloud, items in loaded],
                                          precision=args.precision, max_points=args.max_points)
        # metric stage alone, timed again for the whole set (refined lines already known)
        plans = [metrics.scene_rows(items) for _, _, _, items in loaded]
        gts_all, gt_index = [], []
        for rows, raw, gts, cal_gt in plans:
            gt_index += [-1 if g is None else len(gts_all) + r for r, g in enumerate(gts)]
            gts_all += gts
        cal = [(raw, cal_gt) for rows, raw, gts, cal_gt in plans if raw and cal_gt]
        torch.cuda.synchronize()
        t = time.perf_counter()
        if gt_index:
            metrics.line_metrics(np.concatenate([r["noisy"] for r in results]), np.concatenate([r["refined"] for r in results]),
                                 gts_all, gt_index)
        if cal:
            metrics.calibrate_alignments([c[0] for c in cal], [c[1] for c in cal])
        torch.cuda.synchronize()
        metric_s, metric_rows = time.perf_counter() - t, len(gt_index)
        for (i, name, _, _), res in zip(loaded, results):
            print(f"Processing Scene {i}: {name}")
            report(name, res)

    summary = {k: (float(np.mean(v)) if v else None) for k, v in keep.items()}
    summary["rows_scored"] = len(keep["ade_noisy"])
    summary["metric_rows_per_s"] = metric_rows / metric_s if metric_s > 0 else None
    fmt = lambda v: "n/a" if v is None else f"{v:.3f}"
    print(f"SUMMARY over {summary['rows_scored']} valid, non-bad rows: "
          f"ADE {fmt(summary['ade_noisy'])}->{fmt(summary['ade_refined'])} | "
          f"Lat {fmt(summary['lat_noisy'])}->{fmt(summary['lat_refined'])} | "
          f"metric stage {fmt(summary['metric_rows_per_s'])} rows/s")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"summary": summary, "scenes": per_scene}, f)


if __name__ == "__main__":
    main()
