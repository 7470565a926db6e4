"""A whole drive in, one refined lane map out: the drive is cut into 50 m ego-frame slices, every
slice's lines are refined by the model, and the refined pieces are fused into one polyline per
input line in the drive frame (pointnet_refine_amd/fuse.py).

    python examples/refine_drive.py DRIVE_DIR LINES_JSON --checkpoint CKPT --out MAP.json
                                    [--noise S] [--seed N] [--gt GT_JSON] [--png DIR] [--batched]
                                    [--support [--intensity-floor F|auto]]

DRIVE_DIR holds pose/*.json and merged.pcd; LINES_JSON the lines to refine in the drive file layout
(items[].category / attributes / position); MAP.json gets the fused map in the same layout.
--noise S perturbs the lines at drive level first (drive.noisy_candidates, one scale, seeded) - the
way to try the pipeline on a drive that only has ground truth.  With --gt (default: LINES_JSON when
--noise is given) three map_error figures against the ground truth are printed: the input lines,
the refined pieces before fusion, and the fused map; GT_JSON must list the same lines in the same
order.  --support scores the input lines and the fused map against the cloud itself, with no GT
(pointnet_refine_amd/support.py): one MAP SUPPORT line with the share of the map's 0.5 m stations
that have lidar points under them, the intensity-weighted lateral offset of those points from the
input lines and from the fused map (where the paint lies; --intensity-floor F is subtracted from
the intensity first, so asphalt weighs nothing) and the markings counted by type; every line's
figures and its marking (solid / dashed / none) go into MAP.json's attributes.  --png DIR draws the fused map over the merged cloud (view3d.render_cloud3d).

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


def show(label, e):
    print(f"  {label:<16} mean {e['mean']:.4f} m   max {e['max']:.4f} m   coverage {100.0 * e['coverage']:.1f} %   "
          f"({e['vertices']} vertices)")


def show_support(fused, before, attributes):
    kinds = [a["marking"] for a in attributes]
    counted = ", ".join(f"{kinds.count(k)} {k}" for k in ("solid", "dashed", "none", "unknown") if kinds.count(k))
    move = f"{fused['offset_w_mean']:+.4f} m" if before is None else \
        f"{before['offset_w_mean']:+.4f} m -> {fused['offset_w_mean']:+.4f} m"
    print(f"MAP SUPPORT  {100.0 * fused['supported_share']:.1f} % of {fused['nodes']} stations supported   "
          f"offset_w mean {move}   markings: {counted or 'no lines'}")


def main():
    from pointnet_refine_amd import paintfloor
    ap = argparse.ArgumentParser()
    ap.add_argument("drive_dir")
    ap.add_argument("lines_json")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--noise", type=float, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--gt", default=None)
    ap.add_argument("--png", default=None)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--batched", action="store_true", help="contexts of all slices in one ragged GPU pass")
    ap.add_argument("--support", action="store_true", help="score the map against the cloud (no GT needed)")
    ap.add_argument("--intensity-floor", type=paintfloor.floor_argument, default=0.0,
                    help="a number, or auto: read from the road surface of the slices (one PAINT FLOOR line)")
    args = ap.parse_args()

    from pointnet_refine_amd import drive, fuse
    items = drive.load_gt_items(args.lines_json)
    lines = [it["points"] for it in items]
    gt_path = args.gt if args.gt is not None else (args.lines_json if args.noise is not None else None)
    if args.noise is not None:
        lines = [c[0] for c in drive.noisy_candidates(lines, (args.noise,), seed=args.seed)]
        print(f"Perturbed {len(lines)} lines at scale {args.noise} (seed {args.seed})")
    res = fuse.refine_drive(load_model(args.checkpoint), args.drive_dir, None, lines, seed=args.seed, step=args.step,
                            batched=args.batched, support=args.support, intensity_floor=args.intensity_floor)
    rep = res["report"]
    if args.intensity_floor == "auto":
        print(paintfloor.floor_line(rep))
    print(f"{rep['slices']} slices, {rep['pieces']} pieces ({rep['pieces_sparse']} left out: sparse tube), "
          f"{rep['nodes_used']} of {rep['nodes']} nodes used, {rep['fused_polylines']} polylines")
    attributes = [dict(it["attributes"]) for it in items]
    if args.support:
        sup = res["support"]
        show_support(sup["fused"], sup["input"], sup["attributes"])
        for attr, marking in zip(attributes, sup["attributes"]):
            attr.update({k: None if v != v else v for k, v in marking.items()})      # nan has no JSON form
    n = fuse.write_map_json(args.out, res["fused"], categories=[it["category"] for it in items], attributes=attributes)
    print(f"Wrote {n} polylines to {args.out}")
    if gt_path is not None:
        gt = [it["points"] for it in drive.load_gt_items(gt_path)]
        if len(gt) != len(lines):
            raise SystemExit(f"{gt_path} lists {len(gt)} lines, {args.lines_json} {len(lines)}: they must correspond")
        world = res["nodes"]["world"]
        pieces = [[world[p] for p in np.flatnonzero(res["piece_line"] == l)] for l in range(len(lines))]
        print(f"Distance to {gt_path}:")
        show("input lines", fuse.map_error([[l] for l in lines], gt))
        show("refined pieces", fuse.map_error(pieces, gt))
        show("fused map", fuse.map_error(res["fused"], gt))
    if args.png is not None:
        from pointnet_refine_amd import view3d
        cloud = drive.load_merged_cloud(args.drive_dir)
        parts = [(p, items[l]["category"]) for l, f in enumerate(res["fused"]) for p in f]
        name = os.path.basename(os.path.normpath(args.drive_dir)) + "_map"
        view3d.render_cloud3d(cloud, [p for p, _ in parts], categories=[c for _, c in parts], out_dir=args.png, name=name)
        print(f"Saved {os.path.join(args.png, name + '.png')}")


if __name__ == "__main__":
    main()
