"""Drive slicer (the reference's tools/generate_train_data.py, and with --candidates its
tools/augment_train_data.py): DRIVE_DIR holds pose/*.json and merged.pcd, GT_JSON the drive's GT
polylines; OUT_DIR receives one NAME.pcd / NAME.json scene per 25 m step, the files
SceneSampleStream reads.  Every slice of the drive comes out of one slice_cloud and one
clip_lines call on the GPU.

    python examples/slice_drive.py DRIVE_DIR GT_JSON OUT_DIR [--candidates] [--seed 0]

Without --candidates the scenes hold GT only; train on them with
SceneSampleStream(OUT_DIR, augment=(0.1, 0.25, 0.4)), which draws fresh candidates every epoch.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("drive_dir")
    ap.add_argument("gt_json")
    ap.add_argument("out_dir")
    ap.add_argument("--candidates", action="store_true", help="store three noisy candidates per GT line")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from pointnet_refine_amd import drive
    print(f"\nProcessing Dataset:\n  Raw: {args.drive_dir}\n  GT: {args.gt_json}")
    drive.slice_drive(args.drive_dir, args.gt_json, args.out_dir, candidates=args.candidates, seed=args.seed)


if __name__ == "__main__":
    main()
