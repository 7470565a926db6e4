"""3-D pictures of scenes (the reference's inference_whole_scene.py figure, tools/visualize_data.py,
check_global_align.py and visualize_sampled_pointcloud.py, without Plotly or matplotlib and without
their point caps): every point of the cloud is drawn, PNG and JSON files come out.

    python examples/render_3d.py scenes SCENE_DIR --out DIR [--checkpoint CKPT] [--closeups] [--max-scenes 50]
        for every NAME.json / NAME.pcd pair: NAME_view_K.png (the overview, then one close-up per
        item with --closeups) and NAME.json with the cameras and the legend labels (context GT
        orange, GT green, noisy dashed red, refined magenta with markers)
    python examples/render_3d.py clouds SCENE_DIR --out DIR [--max-scenes 50]
        the data viewer: NAME.png with the cloud, the GT lines and the three noisy candidates of the
        first item that has them (no model needed)
    python examples/render_3d.py drive DRIVE_DIR GT_JSON --out DIR [--max-slices 8]
        a drive directory (pose/*.json, merged.pcd): NAME_merged.png, the whole merged cloud against
        its GT (check_global_align.py's picture), and NAME_slice_POSE.png per slice the slicer cuts,
        all slices drawn from one pass over the sliced cloud
    python examples/render_3d.py sample --out DIR [--checkpoint CKPT]
        what the network sees: one synthetic training sample, context points, noisy line and GT

Without --checkpoint the model carries deterministic procedural weights (the run then exercises the
path and says nothing about accuracy).
"""
import argparse
import os
import sys

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


def scene_pairs(scene_dir, max_scenes):
    names = sorted(f for f in os.listdir(scene_dir) if f.endswith(".json"))
    for name in names[:max_scenes]:
        json_path = os.path.join(scene_dir, name)
        pcd_path = json_path.replace(".json", ".pcd")
        if os.path.exists(pcd_path):
            yield os.path.splitext(name)[0], json_path, pcd_path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tool", choices=("scenes", "clouds", "drive", "sample"))
    ap.add_argument("scene_dir", nargs="?", help="SCENE_DIR, or DRIVE_DIR for the drive tool")
    ap.add_argument("gt_json", nargs="?", help="drive tool: the drive's GT polylines")
    ap.add_argument("--max-slices", type=int, default=8)
    ap.add_argument("--out", required=True)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--closeups", action="store_true")
    ap.add_argument("--max-scenes", type=int, default=50)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=960)
    args = ap.parse_args()

    from pointnet_refine_amd import io, view3d
    if args.tool == "sample":
        from pointnet_refine_amd.synth import synthetic_batch
        ctx, noisy, target = synthetic_batch(1, 1024, torch.device("cuda"), seed=0)
        view3d.render_sample3d(ctx, noisy, target, out_dir=args.out, name="sample3d")
        print(f"Saved {os.path.join(args.out, 'sample3d.png')}")
        return
    if not args.scene_dir:
        ap.error("scenes, clouds and drive need a directory")
    if args.tool == "drive":
        name = os.path.basename(os.path.normpath(args.scene_dir))
        res = view3d.render_drive3d(args.scene_dir, args.gt_json, out_dir=args.out, name=name, max_slices=args.max_slices,
                                    height=args.height, width=args.width)
        print(f"Saved {name}_merged.png and {len(res['names'])} slice view(s)")
        return
    model = load_model(args.checkpoint) if args.tool == "scenes" else None
    found = False
    for stem, json_path, pcd_path in scene_pairs(args.scene_dir, args.max_scenes):
        found = True
        print(f"Processing {stem}...")
        cloud = io.load_pcd_data(pcd_path)
        if len(cloud) == 0:
            print("  empty cloud, skipping")
            continue
        items = io.load_scene_items(json_path)
        if args.tool == "scenes":
            res = view3d.render_scene3d(model, cloud, items, out_dir=args.out, name=stem, closeups=args.closeups,
                                        height=args.height, width=args.width)
            for label in res["labels"]:
                if label.startswith("Noisy"):
                    print("  " + label.replace("<br>", " | "))
            print(f"Saved {len(res['cameras'])} view(s) of {stem}")
        else:
            gts = [it["position"] for it in items if it["position"] is not None and len(it["position"]) > 1]
            cands = next((it["noisy_candidates"][:3] for it in items if it["noisy_candidates"]), [])
            view3d.render_cloud3d(cloud, gts, candidates=cands, out_dir=args.out, name=stem, height=args.height,
                                  width=args.width)
            print(f"Saved {stem}.png")
    if not found:
        print("No data found.")


if __name__ == "__main__":
    main()
