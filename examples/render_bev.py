"""BEV pictures of refined scenes (the reference's tools/vis_inference_bev.py main(), without
matplotlib): for every NAME.json / NAME.pcd pair of SCENE_DIR, one NAME_item_K.png per item - the
scene's intensity image zoomed on the item, GT lime, the first noisy candidate dashed red, the
refined line cyan - and one NAME.json with the windows and the legend labels (`Noisy (E=..m)`,
`Refined (E=..m)`).

    python examples/render_bev.py SCENE_DIR --out DIR [--checkpoint CKPT] [--max-scenes 50]

Without --checkpoint the model carries deterministic procedural weights (the run then exercises the
path and says nothing about accuracy).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scene_dir")
    ap.add_argument("--out", required=True)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--max-scenes", type=int, default=50)          # NUM_VIS_SAMPLES of the reference
    args = ap.parse_args()

    from pointnet_refine_amd import bev, io
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

    json_files = sorted(f for f in os.listdir(args.scene_dir) if f.endswith(".json"))
    if not json_files:
        print("No data found.")
        return
    for name in json_files[:args.max_scenes]:
        json_path = os.path.join(args.scene_dir, name)
        pcd_path = json_path.replace(".json", ".pcd")
        if not os.path.exists(pcd_path):
            continue
        print(f"Processing {name}...")
        cloud = io.load_pcd_data(pcd_path)
        if len(cloud) == 0:
            print(f"  empty cloud, skipping")
            continue
        stem = os.path.splitext(name)[0]
        res = bev.render_scene(model, cloud, io.load_scene_items(json_path), out_dir=args.out, name=stem)
        for k, idx in enumerate(res["items"]):
            label = ""
            if res["refined"][k] is not None:
                label = f": Noisy (E={res['err_noisy'][k]:.2f}m) Refined (E={res['err_refined'][k]:.2f}m)"
            print(f"Saved {stem}_item_{idx}.png{label}")


if __name__ == "__main__":
    main()
