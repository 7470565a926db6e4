"""Prediction scenes (the reference's tools/generate_inference_data_vma.py): DRIVE_DIR holds
pose/*.json and merged.pcd, GT_JSON the drive's GT polylines, RESULTS_JSON the lane detector's
per-frame BEV-pixel polylines; OUT_DIR receives one TS.pcd / TS.json scene per camera frame, each
prediction paired with the GT line the global assignment gives it - the files
examples/evaluate_scenes.py reads.  Every frame of the drive goes through one slice, one clip, one
cost and one assignment launch on the GPU.

    python examples/predictions_to_scenes.py DRIVE_DIR GT_JSON RESULTS_JSON OUT_DIR [--evaluate CHECKPOINT [--batched]]
                                             [--lift] [--align [--align-max-yaw RAD]]

--evaluate CHECKPOINT scores what was written with metrics.evaluate_scene (CHECKPOINT: a
LineRefineNet state_dict, or "procedural" for deterministic weights that exercise the path only)
and prints the mean ADE / Lat before and after over valid, non-bad-match rows.  --batched scores
every written frame with one metrics.evaluate_scenes call (clouds parsed on the device) instead.
--lift writes the candidates with the z of the road under them, read from each frame's own cloud
(pointnet_refine_amd/ground.py), instead of the detector's z = 0.
--align writes the candidates with their x y moved onto the paint of each frame's own cloud
(pointnet_refine_amd/align.py); the matches and everything else in the files stay as they are.
--align-max-yaw RAD also sweeps a yaw of up to RAD radians about each frame's ego origin, for the
heading error a shift cannot take out; the PAINT ALIGN line then carries the median and largest yaw.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("drive_dir")
    ap.add_argument("gt_json")
    ap.add_argument("results_json")
    ap.add_argument("out_dir")
    ap.add_argument("--evaluate", metavar="CHECKPOINT", default=None)
    ap.add_argument("--batched", action="store_true", help="--evaluate: one metrics.evaluate_scenes call for all frames")
    ap.add_argument("--lift", action="store_true", help="candidates carry the road height read from the cloud")
    ap.add_argument("--align", action="store_true", help="candidates are moved in x y onto the paint read from the cloud")
    ap.add_argument("--align-max-yaw", type=float, default=0.0, metavar="RAD",
                    help="with --align: also sweep a yaw of up to RAD radians about each frame's ego origin")
    args = ap.parse_args()
    from pointnet_refine_amd import io, metrics, predictions
    res = predictions.predictions_to_scenes(args.drive_dir, args.gt_json, args.results_json, args.out_dir, lift=args.lift,
                                            align=args.align, align_max_yaw=args.align_max_yaw)
    if args.lift and "lift" in res:
        rep = res["lift"]
        print(f"GROUND LIFT  {rep['lines_lifted']} of {rep['lines']} lines lifted   {rep['stations_without_ground']} of "
              f"{rep['stations']} stations without ground")
    if args.align and "align" in res:
        rep = res["align"]
        yaw = ""
        if args.align_max_yaw > 0.0:
            a = np.abs(rep["yaws"]) if rep["frames"] else np.zeros(1)
            yaw = f"   |yaw| median {float(np.median(a)) * 1e3:.1f} mrad   max {float(a.max()) * 1e3:.1f} mrad"
        print(f"PAINT ALIGN  {rep['frames_aligned']} of {rep['frames']} frames aligned{yaw}")
    if args.evaluate is None:
        return
    import torch
    from pointnet_refine_amd.model import LineRefineNet
    model = LineRefineNet()
    if args.evaluate == "procedural":
        from oracle import procedural as P
        model.load_state_dict(P.linerefine_state_dict(0))
    else:
        model.load_state_dict(torch.load(args.evaluate, map_location="cpu"))
    model = model.cuda().eval()
    keep = {k: [] for k in ("ade_noisy", "ade_refined", "lat_noisy", "lat_refined")}
    rows = bad = 0
    if args.batched:
        from pointnet_refine_amd import pcd
        scenes = [(pcd.read_pcd(os.path.join(args.out_dir, f"{ts}.pcd"), device="cuda"),
                   io.load_scene_items(os.path.join(args.out_dir, f"{ts}.json"))) for ts in res["written"]]
        evaluated = iter(metrics.evaluate_scenes(model, scenes))
    for ts in res["written"]:
        if args.batched:
            ev = next(evaluated)
        else:
            items = io.load_scene_items(os.path.join(args.out_dir, f"{ts}.json"))
            ev = metrics.evaluate_scene(model, io.load_pcd_data(os.path.join(args.out_dir, f"{ts}.pcd")), items)
        use = ev["valid"] & ~ev["bad_match"]
        rows, bad = rows + len(use), bad + int(ev["bad_match"].sum())
        for k in keep:
            keep[k] += ev[k][use].tolist()
    mean = {k: (float(np.mean(v)) if v else float("nan")) for k, v in keep.items()}
    print(f"EVALUATION over {len(res['written'])} scenes, {rows} predictions, {len(keep['ade_noisy'])} scored, "
          f"{bad} bad matches: ADE {mean['ade_noisy']:.3f}->{mean['ade_refined']:.3f} | "
          f"Lat {mean['lat_noisy']:.3f}->{mean['lat_refined']:.3f}")


if __name__ == "__main__":
    main()
