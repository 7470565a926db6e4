"""Times the surface gate of paint tracing (csrc/prh_trace.hpp trace_hist_surface_kernel,
pointnet_refine_amd/trace.py) and writes a report (default profiles/r23_trace_surface_bench.txt) that ends
in one JSON line:

  kernels   prh_trace_hist and prh_trace_hist_surface (their memsets included) in the same process over
            the slices of a generated drive - paint_floor_bench.py's: --slices x --points-per-slice
            float64 points, 3 % of them paint at 40-60, intensity_floor 20 - with the ground table
            paintfloor.surface_ground builds for them, next to the bytes both must read (every row
            once) at 5 TB/s; the same with a third of the paint lifted 0.6 m off the road, where the
            gate has something to leave out; device events, median of --reps after one warm-up call
  drive     trace.refine_cloud whole on one generated drive directory (paint_trace_bench.py's, about
            2 M points), wall clock, median of --reps after one warm-up call: at the default, with
            surface=True, with intensity_floor="auto", and with both, where the floor and the gate share
            one ground table

Without --step every step runs in a child process of its own, under its own time limit, and the first
that fails ends the run; --step report writes the report from the parts that have run and names the others.

    python scripts/trace_surface_bench.py [--slices 40] [--points-per-slice 500000] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

HBM_BYTES_PER_S = 5e12
TRACE_FLOOR = 20.0
STEPS = ("kernels", "drive")
STEP_LIMIT_S = {"kernels": 300, "drive": 420}


def stat(runs):
    return {"ms": float(np.median(runs)), "runs": [round(v, 3) for v in runs]}


def step_kernels(args):
    import torch
    from link_bench import events_ms
    from paint_floor_bench import generated_slices
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    from pointnet_refine_amd import paintfloor as PF
    from pointnet_refine_amd import trace as T
    dev = G.device("trace")
    lib = L.lib()
    n_s, n_pts = args.slices, args.points_per_slice
    pts = generated_slices(n_s, n_pts, args.lanes, dev, torch)
    off = np.arange(n_s + 1, dtype=np.int64) * n_pts
    off_t = torch.from_numpy(off).to(dev)
    tp = T._params("bench", intensity_floor=TRACE_FLOOR)
    sp = T._surface_params("bench", tp)
    ground = PF.surface_ground(pts, off)
    nb = lib.prh_trace_workspace_bytes(n_s, tp["nx"], tp["ny"])
    ws = G.workspace(nb, dev)
    off_surface = torch.empty((n_s,), dtype=torch.int64, device=dev)

    def hist(p, gated):
        a = (G.ptr(p), 1, G.ptr(off_t), n_s, 0, p.shape[0], tp["half_length"], tp["col"], tp["nx"], tp["half_width"],
             tp["cell"], tp["ny"], TRACE_FLOOR, G.ptr(ws), nb)
        if gated:
            L.check(lib.prh_trace_hist_surface(*a, sp["half_length"], sp["half_width"], sp["ground_cell"], sp["gx"], sp["gy"],
                                               G.ptr(ground), sp["band"], G.ptr(off_surface), dev.index, G.stream(dev)),
                    "prh_trace_hist_surface")
        else:
            L.check(lib.prh_trace_hist(*a, dev.index, G.stream(dev)), "prh_trace_hist")

    def bright():
        return int(ws[:4 * n_s * tp["nx"] * tp["ny"]].view(torch.int32).sum(dtype=torch.int64).item())

    res, counts = {}, {}
    lifted = pts.clone()                                         # a third of the paint 0.6 m up: what the gate is for
    up = (lifted[:, 3] > TRACE_FLOOR) & (torch.arange(lifted.shape[0], device=dev) % 3 == 0)
    lifted[up, 2] += 0.6
    for name, p in (("flat", pts), ("lifted", lifted)):
        # ungated, gated, and each once more: the order of the rows must not decide the comparison
        for key, gated in (("plain", False), ("surface", True), ("plain_again", False), ("surface_again", True)):
            res[f"{name}_{key}"] = stat(events_ms(lambda: hist(p, gated), args.reps))
            counts[f"{name}_{key}"] = bright()
        counts[f"{name}_off_surface"] = int(off_surface.sum().item())
    return {"device": torch.cuda.get_device_name(0), "slices": n_s, "points_per_slice": n_pts, "lanes": args.lanes,
            "reps": args.reps, "gx": sp["gx"], "gy": sp["gy"], "band": sp["band"],
            "cells_without_ground": int(torch.isnan(ground).sum().item()), "results": res, "counts": counts}


def step_drive(args):
    import torch
    from link_bench import wall_ms
    from oracle import procedural as P
    from paint_trace_bench import write_drive
    from pointnet_refine_amd import trace as T
    from pointnet_refine_amd.model import LineRefineNet
    model = LineRefineNet()
    model.load_state_dict(P.linerefine_state_dict(0))
    model = model.cuda().eval()

    def median_wall(fn):
        fn()
        return stat([wall_ms(fn)[0] for _ in range(args.reps)])

    modes = {"default": dict(intensity_floor=TRACE_FLOOR), "surface": dict(intensity_floor=TRACE_FLOOR, surface=True),
             "auto": dict(intensity_floor="auto"), "auto_surface": dict(intensity_floor="auto", surface=True)}
    with tempfile.TemporaryDirectory() as root:
        drive, _, n_cloud = write_drive(root, args.drive_length, 500.0, 300.0)
        runs = {k: T.refine_cloud(model, drive, batched=True, **kw) for k, kw in modes.items()}
        res = {k: median_wall(lambda: T.refine_cloud(model, drive, batched=True, **kw)) for k, kw in modes.items()}
    rep = {k: r["report"] for k, r in runs.items()}
    return {"device": torch.cuda.get_device_name(0), "cloud_points": n_cloud, "drive_length": args.drive_length,
            "reps": args.reps, "results": res, "slices": rep["default"]["slices"],
            "trace_lines": {k: r["trace_lines"] for k, r in rep.items()}, "clusters": {k: r["clusters_kept"] for k, r in rep.items()},
            "off_surface": {k: r["trace_off_surface_points"] for k, r in rep.items() if "trace_off_surface_points" in r},
            "floor": {k: r["floor"] for k, r in rep.items() if "floor" in r},
            "same_pieces_default_surface": bool(runs["default"]["pieces"].tobytes() == runs["surface"]["pieces"].tobytes()),
            "same_pieces_auto_auto_surface": bool(runs["auto"]["pieces"].tobytes() == runs["auto_surface"]["pieces"].tobytes())}


def report(args, parts):
    lines = ["Surface gate of paint tracing: the tracer sees the road surface only (prh_trace_hist_surface; trace.paint_peaks with a",
             "ground table, trace.refine_cloud with surface=True).",
             f"Command: python scripts/trace_surface_bench.py   (--slices {args.slices} --points-per-slice {args.points_per_slice} "
             f"--lanes {args.lanes} --drive-length {args.drive_length:g} --reps {args.reps})",
             f"Written {time.strftime('%Y-%m-%d')}; every step one child process under its own time limit.", ""]
    not_run = [s for s in STEPS if s not in parts]
    if not_run:
        lines += [f"NOT RUN: {', '.join(not_run)} - no numbers for {'these steps' if len(not_run) > 1 else 'this step'} below.", ""]
    if "kernels" in parts:
        k = parts["kernels"]
        n = k["slices"] * k["points_per_slice"]
        floor_ms = n * 32 / HBM_BYTES_PER_S * 1e3
        lines += [f"Machine: 1 x MI355X (reported as \"{k['device']}\"), one process.  Device events around the call (memsets included), median "
                  f"of {k['reps']} after one warm-up call.",
                  f"Generated slices: {k['slices']} x {k['points_per_slice']} = {n} float64 points, 3 % of them paint in {k['lanes']} bands, "
                  f"intensity_floor {TRACE_FLOOR:g}; ground table {k['gx']} x {k['gy']} cells of 1 m per slice ({k['cells_without_ground']} "
                  f"of {k['slices'] * k['gx'] * k['gy']} without ground), band {k['band']:g}.",
                  f"Both kernels must read {n * 32 / 1e6:.0f} MB: {floor_ms:.3f} ms at 5 TB/s."]
        for name, label in (("flat", "all paint on the road"), ("lifted", "a third of the paint 0.6 m above the road")):
            c = k["counts"]
            lines.append(f"{label}: {c[name + '_plain']} bright points ungated; gated {c[name + '_surface']} kept, {c[name + '_off_surface']} off the surface")
            for key, what in (("plain", "prh_trace_hist"), ("surface", "prh_trace_hist_surface"), ("plain_again", "prh_trace_hist, again"),
                              ("surface_again", "prh_trace_hist_surface, again")):
                v = k["results"][f"{name}_{key}"]
                lines.append(f"  {what:<34} runs (ms) {v['runs']} median {v['ms']:.3f}   {100.0 * floor_ms / v['ms']:.1f} % of 5 TB/s")
            a, b = k["results"][name + "_plain"]["ms"], k["results"][name + "_surface"]["ms"]
            a2, b2 = k["results"][name + "_plain_again"]["ms"], k["results"][name + "_surface_again"]["ms"]
            lines.append(f"  gated / ungated: {b / a:.3f} (first pair), {b2 / a2:.3f} (second pair)")
        lines.append("")
    if "drive" in parts:
        d = parts["drive"]
        r = d["results"]
        lines += [f"Whole, one generated drive directory ({d['cloud_points']} points, {d['drive_length']:g} m, poses 25 m apart, {d['slices']} slices), "
                  f"batched contexts, wall clock (ms), median of {d['reps']} after one warm-up call,",
                  "merged.pcd read and parsed inside every call; procedural weights, so the maps say nothing about accuracy:"]
        for key, what in (("default", f"intensity_floor={TRACE_FLOOR:g}"), ("surface", f"intensity_floor={TRACE_FLOOR:g}, surface=True"),
                          ("auto", 'intensity_floor="auto"'), ("auto_surface", 'intensity_floor="auto", surface=True')):
            tail = f"   {d['trace_lines'][key]} traced lines, {d['clusters'][key]} clusters"
            if key in d["off_surface"]:
                tail += f", {d['off_surface'][key]} bright points off the surface"
            if key in d["floor"]:
                tail += f", floor {d['floor'][key]:g}"
            lines.append(f"  trace.refine_cloud, {what:<44} runs {r[key]['runs']} median {r[key]['ms']:.1f}{tail}")
        lines += [f"  surface=True over the default: {r['surface']['ms'] - r['default']['ms']:+.1f} ms (the ground table); over \"auto\": "
                  f"{r['auto_surface']['ms'] - r['auto']['ms']:+.1f} ms (the table \"auto\" builds anyway is shared)",
                  f"  the same pieces with and without the gate: {d['same_pieces_default_surface']} (fixed floor), "
                  f"{d['same_pieces_auto_auto_surface']} (\"auto\")", ""]
    text = "\n".join(lines) + json.dumps(parts) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=STEPS + ("report",), default=None)
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--points-per-slice", type=int, default=500000)
    ap.add_argument("--lanes", type=int, default=6)
    ap.add_argument("--drive-length", type=float, default=400.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts-dir", default=os.path.join(ROOT, "results", "trace_surface_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_trace_surface_bench.txt"))
    args = ap.parse_args()
    os.makedirs(args.parts_dir, exist_ok=True)
    part = lambda name: os.path.join(args.parts_dir, name + ".json")
    if args.step in STEPS:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("trace_surface_bench.py needs a GPU")
        out = step_kernels(args) if args.step == "kernels" else step_drive(args)
        print(json.dumps(out))
        with open(part(args.step), "w") as f:
            json.dump(out, f)
        return
    if args.step is None:
        for name in STEPS:                                       # one process and one time limit per GPU step; stop at the first failure
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name] + sys.argv[1:],
                                timeout=STEP_LIMIT_S[name]).returncode
            if rc != 0:
                raise SystemExit(f"step {name} ended with status {rc}: nothing more is started")
    parts = {name: json.load(open(part(name))) for name in STEPS if os.path.exists(part(name))}
    report(args, parts)


if __name__ == "__main__":
    main()
