"""A lidar drive in, one refined lane map out, with no detector and no ground truth: the paint is
traced from every slice of the cloud (pointnet_refine_amd/trace.py), the traced lines are refined in
their ego frame, the refined pieces are linked across slices into lanes and fused into one polyline
per lane in the drive frame (pointnet_refine_amd/link.py).

    python examples/refine_cloud.py DRIVE_DIR --checkpoint CKPT --out MAP.json --intensity-floor F|auto
                                    [--half-width W] [--surface [--surface-band B]] [--support]
                                    [--gt GT_JSON] [--png DIR] [--batched] [--device-sync]

DRIVE_DIR holds pose/*.json and merged.pcd; MAP.json gets the fused map in the drive file layout.
--intensity-floor F separates paint from asphalt: F is subtracted from every point's intensity and
only what stays above 0 counts; without a floor that does, the tracer follows asphalt texture.
--intensity-floor auto reads F from the road surface of the slices (pointnet_refine_amd/paintfloor.py)
and prints one PAINT FLOOR line: the floor, the surface points it was read from, the share above it.
--half-width W is the half width, in metres, of the strip beside the ego x axis that is traced.
--surface traces the road surface only: a bright point counts where it lies within B metres (0.15) of
the road height of its 1 m cell, so the trail of a followed vehicle, reflectors and signs are left out;
the PAINT TRACE line then ends with the number of bright points off the surface.
One PAINT TRACE line says how many slices, bright points, peaks and lines the tracer found; the map,
--support, --gt, --png, --batched and --device-sync lines are those of examples/refine_predictions.py.

Without --checkpoint the model carries deterministic procedural weights (the run then exercises the
path and says nothing about accuracy).
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from refine_predictions import load_model, report_map  # noqa: E402


def main():
    from pointnet_refine_amd import paintfloor
    ap = argparse.ArgumentParser()
    ap.add_argument("drive_dir")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--out", required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--intensity-floor", type=paintfloor.floor_argument, required=True, help="a number, or auto")
    ap.add_argument("--half-width", type=float, default=12.8)
    ap.add_argument("--surface", action="store_true", help="trace only points on the road surface")
    ap.add_argument("--surface-band", type=float, default=paintfloor.BAND, help="metres from the road height, with --surface")
    ap.add_argument("--gt", default=None)
    ap.add_argument("--png", default=None)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--gate", type=float, default=1.0)
    ap.add_argument("--min-pieces", type=int, default=2)
    ap.add_argument("--batched", action="store_true", help="contexts of all slices in one ragged GPU pass")
    ap.add_argument("--device-sync", action="store_true", help="piece linking steps 5-6 on the GPU (the same map)")
    ap.add_argument("--support", action="store_true", help="score the map against the cloud (no GT needed)")
    args = ap.parse_args()

    from pointnet_refine_amd import trace
    surface = dict(surface=True, surface_band=args.surface_band) if args.surface else {}
    res = trace.refine_cloud(load_model(args.checkpoint), args.drive_dir, seed=args.seed, step=args.step, gate=args.gate,
                             min_pieces=args.min_pieces, batched=args.batched, support=args.support,
                             device_sync=args.device_sync, intensity_floor=args.intensity_floor,
                             half_width=args.half_width, **surface)
    rep = res["report"]
    if args.intensity_floor == "auto":
        print(paintfloor.floor_line(rep))
    print(f"PAINT TRACE  {rep['trace_slices']} slices   {rep['trace_bright_points']} bright points   "
          f"{rep['trace_peaks']} peaks   {rep['trace_lines']} lines ({rep['trace_lines_dropped_short']} short chains left out)"
          + (f"   {rep['trace_off_surface_points']} bright points off the surface" if args.surface else ""))
    report_map(res, args)


if __name__ == "__main__":
    main()
