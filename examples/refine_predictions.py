"""A detector run in, one refined lane map out, with no ground truth in between: every camera
frame's BEV-pixel polylines are refined in their ego frame, the refined pieces are linked across
frames into lanes and fused into one polyline per lane in the drive frame
(pointnet_refine_amd/link.py).

    python examples/refine_predictions.py DRIVE_DIR RESULTS_JSON --checkpoint CKPT --out MAP.json
                                          [--gt GT_JSON] [--png DIR] [--batched] [--device-sync]
                                          [--support [--intensity-floor F|auto]] [--lift [--lift-radius R]]
                                          [--align [--align-max-shift M] [--align-scope frame|drive] [--align-max-yaw RAD]]

DRIVE_DIR holds pose/*.json and merged.pcd; RESULTS_JSON is the detector's output
(predictions.load_results); MAP.json gets the fused map in the drive file layout
(items[].category / attributes / position), one item per polyline with its cluster as 'source_line'.
With --gt every fused cluster is attributed to the ground-truth line of smallest mean distance
(fuse.project_to_lines) and the map's distance to those lines is printed (fuse.map_error).
--support scores the fused map against the cloud itself (pointnet_refine_amd/support.py): one MAP
SUPPORT line with the share of the map's 0.5 m stations that have lidar points under them, the
intensity-weighted lateral offset of those points (--intensity-floor F is subtracted from the
intensity first) and the markings counted by type; every cluster's figures and its marking (solid /
dashed / none) go into MAP.json's attributes.
--device-sync runs the linking's edges, clusters and arc synchronisation on the GPU as well
(link.link_sync): the same map, without copying the candidate pairs' statistics to the host.
--lift puts the detector's lines (z = 0) on the road before they are refined: the road height under
every metre of every line is read from the frame's own cloud points within --lift-radius R
(pointnet_refine_amd/ground.py), and one GROUND LIFT line says how many lines and stations found ground.
--align then moves every frame's lines in x y onto the paint: the shift, up to --align-max-shift M per
component, under which the frame's bright cloud points lie closest to the lines
(pointnet_refine_amd/align.py), per frame or - --align-scope drive - one for the whole drive; one
PAINT ALIGN line says how many frames were aligned and the median and largest shift.
--align-max-yaw RAD sweeps a yaw of up to RAD radians about each frame's ego origin together with the
shift (a heading error of the extrinsic turns the lines about the sensor, and no shift takes that
out); the PAINT ALIGN line then carries the median and largest yaw as well.
--png DIR draws the fused map over a BEV intensity map of the merged cloud (bev.py).

Without --checkpoint the model carries deterministic procedural weights (the run then exercises the
path and says nothing about accuracy).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PNG_RESOLUTION = 0.1         # metres per pixel of the --png picture


def load_model(checkpoint):
    from pointnet_refine_amd.model import LineRefineNet
    model = LineRefineNet()
    if checkpoint:
        model.load_state_dict(torch.load(checkpoint, map_location="cpu"))
        print(f"Loaded model from {checkpoint}")
    else:
        from oracle import procedural as P
        model.load_state_dict(P.linerefine_state_dict(0))
        print("No checkpoint: procedural weights")
    return model.cuda().eval()


def attribute(fused, gt):
    """Per fused cluster the GT line of smallest mean distance over the cluster's vertices."""
    from pointnet_refine_amd import fuse
    owner = []
    for parts in fused:
        pts = np.concatenate(parts) if parts else np.zeros((0, 3))
        if len(pts) == 0 or not gt:
            owner.append(-1)
            continue
        means = [float(fuse.project_to_lines(pts, np.full(len(pts), l), gt)[1].mean()) if len(gt[l]) else np.inf
                 for l in range(len(gt))]
        owner.append(int(np.argmin(means)))
    return owner


def report_map(res, args):
    """The map, support and map_error lines, MAP.json and the --png picture: what this tool and
    examples/refine_cloud.py print once the drive is refined.  args: out, drive_dir, support, gt, png."""
    from pointnet_refine_amd import drive, fuse
    rep = res["report"]
    print(f"{rep['slices']} frames, {rep['pieces']} pieces ({rep['pieces_sparse']} left out: sparse tube), "
          f"{rep['candidates']} candidate pairs, {rep['edges']} edges, {rep['clusters']} clusters, "
          f"{rep['clusters_kept']} kept ({rep['pieces_unlinked']} pieces unlinked), "
          f"{rep['nodes_used']} of {rep['nodes']} nodes used, {rep['fused_polylines']} polylines")
    fused = res["fused"]
    attributes = None
    if args.support:
        sup = res["support"]
        attributes = [{k: None if v != v else v for k, v in a.items()} for a in sup["attributes"]]   # nan has no JSON form
        kinds = [a["marking"] for a in attributes]
        counted = ", ".join(f"{kinds.count(k)} {k}" for k in ("solid", "dashed", "none", "unknown") if kinds.count(k))
        print(f"MAP SUPPORT  {100.0 * sup['fused']['supported_share']:.1f} % of {sup['fused']['nodes']} stations supported   "
              f"offset_w mean {sup['fused']['offset_w_mean']:+.4f} m   markings: {counted or 'no lines'}")
    n = fuse.write_map_json(args.out, fused, categories=["lane_line"] * len(fused), attributes=attributes)
    print(f"Wrote {n} polylines to {args.out}")
    if args.gt is not None:
        gt = [it["points"] for it in drive.load_gt_items(args.gt)]
        owner = attribute(fused, gt)
        by_line = [[p for c, parts in enumerate(fused) if owner[c] == l for p in parts] for l in range(len(gt))]
        e = fuse.map_error(by_line, gt)
        print(f"Distance to {args.gt} (clusters attributed to lines {owner}):")
        print(f"  fused map        mean {e['mean']:.4f} m   max {e['max']:.4f} m   coverage {100.0 * e['coverage']:.1f} %   "
              f"({e['vertices']} vertices)")
    if args.png is not None:
        from pointnet_refine_amd import bev
        cloud = drive.load_merged_cloud(args.drive_dir).astype(np.float32)
        image, extent = bev.bev_map(cloud, resolution=PNG_RESOLUTION)
        norm, _ = bev.tone_map(image)
        rgba = bev.colorize(norm, image).contiguous()
        parts = [p for f in fused for p in f]
        bev.draw_lines(rgba, np.array([float(v) for v in extent]), parts, np.zeros(len(parts), dtype=np.int64),
                       [bev.STYLE_REFINED] * len(parts), resolution=PNG_RESOLUTION)
        os.makedirs(args.png, exist_ok=True)
        path = os.path.join(args.png, os.path.basename(os.path.normpath(args.drive_dir)) + "_map.png")
        bev.write_png(path, rgba)
        print(f"Saved {path}")


def main():
    from pointnet_refine_amd import paintfloor
    ap = argparse.ArgumentParser()
    ap.add_argument("drive_dir")
    ap.add_argument("results_json")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gt", default=None)
    ap.add_argument("--png", default=None)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--gate", type=float, default=1.0)
    ap.add_argument("--min-pieces", type=int, default=2)
    ap.add_argument("--batched", action="store_true", help="contexts of all frames in one ragged GPU pass")
    ap.add_argument("--device-sync", action="store_true", help="piece linking steps 5-6 on the GPU (the same map)")
    ap.add_argument("--support", action="store_true", help="score the map against the cloud (no GT needed)")
    ap.add_argument("--intensity-floor", type=paintfloor.floor_argument, default=0.0,
                    help="a number, or auto: read from the road surface of the frames' slices (one PAINT FLOOR line)")
    ap.add_argument("--lift", action="store_true", help="put the detector's lines on the road read from the cloud")
    ap.add_argument("--lift-radius", type=float, default=0.5)
    ap.add_argument("--align", action="store_true", help="move the detector's lines in x y onto the paint of the cloud")
    ap.add_argument("--align-max-shift", type=float, default=1.0)
    ap.add_argument("--align-scope", choices=("frame", "drive"), default="frame")
    ap.add_argument("--align-max-yaw", type=float, default=0.0, metavar="RAD",
                    help="with --align: also sweep a yaw of up to RAD radians about each frame's ego origin")
    args = ap.parse_args()

    from pointnet_refine_amd import link
    res = link.refine_predictions(load_model(args.checkpoint), args.drive_dir, args.results_json, seed=args.seed,
                                  step=args.step, gate=args.gate, min_pieces=args.min_pieces, batched=args.batched,
                                  support=args.support, intensity_floor=args.intensity_floor,
                                  device_sync=args.device_sync, lift=args.lift, lift_radius=args.lift_radius,
                                  align=args.align, align_max_shift=args.align_max_shift, align_scope=args.align_scope,
                                  align_max_yaw=args.align_max_yaw)
    rep = res["report"]
    if args.intensity_floor == "auto":
        print(paintfloor.floor_line(rep))
    if args.lift:
        print(f"GROUND LIFT  {rep['lift_lines_lifted']} of {rep['lift_lines']} lines lifted "
              f"({rep['lift_lines_unlifted']} left at the detector's z)   {rep['lift_stations_without_ground']} of "
              f"{rep['lift_stations']} stations without ground")
    if args.align:
        norm = np.hypot(rep["align_shifts"][:, 0], rep["align_shifts"][:, 1]) if rep["align_frames"] else np.zeros(1)
        yaw = ""
        if args.align_max_yaw > 0.0:
            a = np.abs(rep["align_yaws"]) if rep["align_frames"] else np.zeros(1)
            yaw = f"   |yaw| median {float(np.median(a)) * 1e3:.1f} mrad   max {float(a.max()) * 1e3:.1f} mrad"
        print(f"PAINT ALIGN  {rep['align_frames_aligned']} of {rep['align_frames']} frames aligned   |shift| median "
              f"{float(np.median(norm)):.3f} m   max {float(norm.max()):.3f} m{yaw}   ({rep['align_candidates']} bright points)")
    report_map(res, args)


if __name__ == "__main__":
    main()
