"""Times a data-set evaluation per scene (metrics.evaluate_scene in a loop) against one
metrics.evaluate_scenes call in the same process, clouds already on the device, and writes a report
(default profiles/r13_ragged_evaluation_bench.txt) that ends in one JSON line per step:

  detector   --frames frames of --lanes predictions against --lanes - 1 GT lines (the generated run
             of link_bench.py / ragged_contexts_bench.py as candidates, the clean lanes as GT, a cloud
             of --detector-points points along its path cut into one ego-frame scene per frame)
  reference  the reference's own evaluation size: --scenes scenes of --lines lines
             (scene_eval_bench.py's generator, a cloud of --scene-points points generated on the device)

Per step: the whole evaluation in both modes (the loop three times, for its spread), then the three
phases of each mode on the same inputs - contexts + model, line metrics, calibration - and the
library calls each mode makes.  Nothing is read from outside the tree.

Without --step every step runs in a child process of its own, under its own time limit, and the
first failure ends the run; the report is written from the steps' JSON files.

    python scripts/evaluate_scenes_bench.py [--step detector|reference|report] [--frames 2000] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STEP_LIMIT_S = {"detector": 540, "reference": 420}
LOOP_RUNS = 3


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def procedural_model():
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    model = LineRefineNet()
    model.load_state_dict(P.linerefine_state_dict(0))
    return model.cuda().eval()


class Calls:
    """Counts the library calls of the metric stage while a block runs."""
    NAMES = ("prh_line_metrics", "prh_shift_sweep", "prh_shift_sweep_ragged", "prh_context_build",
             "prh_context_ragged_count", "prh_context_ragged_select")

    def __init__(self):
        from pointnet_refine_amd import _lib as L
        self.lib, self.counts, self.saved = L.lib(), {}, {}

    def __enter__(self):
        for name in self.NAMES:
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def counted(*a, _fn=fn, _name=name):
                self.counts[_name] = self.counts.get(_name, 0) + 1
                return _fn(*a)
            setattr(self.lib, name, counted)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)


def compare(model, scenes, kw):
    """Both modes on resident scenes: whole evaluation, phases, call counts."""
    import torch
    from pointnet_refine_amd import metrics as MT
    from pointnet_refine_amd.context import resample_polylines_device
    from pointnet_refine_amd.io import scene_offsets, scene_offsets_ragged
    m = 32
    plans = [MT.scene_rows(items) for _, items in scenes]
    used = [s for s, p in enumerate(plans) if p[0]]

    def loop():
        return [MT.evaluate_scene(model, cloud, items, **kw) for cloud, items in scenes]

    def batched():
        return MT.evaluate_scenes(model, scenes, **kw)

    MT.evaluate_scenes(model, scenes[:4], **kw)                       # warm-up of both modes
    [MT.evaluate_scene(model, c, it, **kw) for c, it in scenes[:4]]
    loop_ms = []
    for _ in range(LOOP_RUNS):
        ms, per_scene = wall_ms(loop)
        loop_ms.append(round(ms, 1))
        print(f"loop: {ms:.1f} ms", file=sys.stderr, flush=True)
    with Calls() as loop_calls:
        loop()
    batched_ms, ragged = wall_ms(batched)
    batched_ms2, _ = wall_ms(batched)
    print(f"one call: {batched_ms:.1f} ms, {batched_ms2:.1f} ms", file=sys.stderr, flush=True)
    with Calls() as batched_calls:
        batched()
    worst = max((float(np.abs(a["refined"] - b["refined"]).max()) for a, b in zip(per_scene, ragged) if len(a["refined"])),
                default=0.0)
    same_cal = all(a["calibration"] == b["calibration"] for a, b in zip(per_scene, ragged))

    # ---- phases, each mode on the inputs the whole call builds
    def model_loop():
        for s in used:
            off, _, _ = scene_offsets(model, scenes[s][0], plans[s][1], m, **kw)
            (resample_polylines_device(plans[s][1], m, off.device) + off.double()).cpu()

    def model_batched():
        so = np.concatenate([[0], np.cumsum([scenes[s][0].shape[0] for s in used])]).astype(np.int64)
        points = torch.empty((int(so[-1]), 4), dtype=torch.float32, device="cuda")
        for k, s in enumerate(used):
            points[so[k]:so[k + 1]].copy_(scenes[s][0][:, :4])
        raw = [line for s in used for line in plans[s][1]]
        ls = np.repeat(np.arange(len(used)), [len(plans[s][0]) for s in used])
        off, _, _ = scene_offsets_ragged(model, points, so, raw, ls, [kw.get("seed", 0)] * len(used), m,
                                         **{k: v for k, v in kw.items() if k != "seed"})
        (resample_polylines_device(raw, m, off.device) + off.double()).cpu()

    def index(gts, base=0):
        return np.array([-1 if g is None else base + r for r, g in enumerate(gts)], dtype=np.int64)

    def lines_loop():
        for s in used:
            MT.line_metrics(per_scene[s]["noisy"], per_scene[s]["refined"], plans[s][2], index(plans[s][2]))

    noisy_all = np.concatenate([per_scene[s]["noisy"] for s in used])
    refined_all = np.concatenate([per_scene[s]["refined"] for s in used])
    gts_all, gi_all = [], []
    for s in used:
        gi_all.append(index(plans[s][2], len(gts_all)))
        gts_all += plans[s][2]

    def lines_batched():
        MT.line_metrics(noisy_all, refined_all, gts_all, np.concatenate(gi_all))

    cal = [s for s in used if plans[s][3]]

    def cal_loop():
        for s in cal:
            MT.calibrate_alignment(plans[s][1], plans[s][3])
            MT.calibrate_alignment(list(per_scene[s]["refined"]), plans[s][3])

    def cal_batched():
        MT.calibrate_alignments([x for s in cal for x in (plans[s][1], per_scene[s]["refined"])],
                                [plans[s][3] for s in cal], np.repeat(np.arange(len(cal)), 2))

    phases = {}
    for name, fn in (("model_loop", model_loop), ("model_batched", model_batched), ("lines_loop", lines_loop),
                     ("lines_batched", lines_batched), ("calibration_loop", cal_loop), ("calibration_batched", cal_batched)):
        phases[name + "_ms"] = round(wall_ms(fn)[0], 1)
        print(f"{name}: {phases[name + '_ms']:.1f} ms", file=sys.stderr, flush=True)
    return {"scenes": len(scenes), "scenes_with_rows": len(used), "rows": int(sum(len(p[0]) for p in plans)),
            "cloud_points": int(sum(c.shape[0] for c, _ in scenes)),
            "loop_ms": loop_ms, "batched_ms": [round(batched_ms, 1), round(batched_ms2, 1)],
            "speedup": round(float(np.median(loop_ms)) / min(batched_ms, batched_ms2), 2),
            "loop_calls": loop_calls.counts, "batched_calls": batched_calls.counts,
            "refined_max_abs_diff_m": worst, "calibration_equal": bool(same_cal), **phases}


def step_detector(args):
    import torch
    import _fuse_oracle as O
    from link_bench import make_run, path_y
    from pointnet_refine_amd import drive
    rng = np.random.default_rng(0)
    model = procedural_model()
    pieces, _, poses = make_run(args.frames, args.lanes, rng)
    x = rng.uniform(0.0, poses[-1, 0] + 30.0, args.detector_points)
    cloud = np.column_stack([x, path_y(x) + rng.uniform(-21.0, 21.0, len(x)), 0.2 * np.sin(x / 45.0) + rng.normal(0.0, 0.03, len(x)),
                             rng.uniform(0.0, 60.0, len(x))]).astype(np.float32)
    pts, offs, _ = drive.slice_cloud(torch.from_numpy(cloud).cuda(), poses, 50.0, 60.0)
    pts, oh = pts.to(torch.float32), offs.cpu().numpy()
    n_gt = args.lanes - 1
    scenes = []
    for f in range(args.frames):
        gx = poses[f, 0] + np.linspace(-30.0, 30.0, 61)
        items = []
        for l in range(n_gt):                     # GT: the clean lane; the last GT line is matched by two predictions
            w = np.column_stack([gx, path_y(gx) + 3.5 * (l - (args.lanes - 1) / 2), 0.2 * np.sin(gx / 45.0)])
            cands = [pieces[f * args.lanes + l]] + ([pieces[f * args.lanes + args.lanes - 1]] if l == n_gt - 1 else [])
            items.append({"position": O.to_ego(w, poses[f]), "noisy_candidates": cands, "context_lines": []})
        scenes.append((pts[oh[f]:oh[f + 1]], items))
    out = {"step": "detector", "device": torch.cuda.get_device_name(0), "frames": args.frames, "lanes": args.lanes,
           "gt_lines": n_gt, "detector_points": args.detector_points}
    out.update(compare(model, scenes, {}))
    return out


def step_reference(args):
    import torch
    from scene_eval_bench import scene
    model = procedural_model()
    origin = np.array([4.0e5, 5.0e6, 30.0])
    g = torch.Generator(device="cuda").manual_seed(0)
    scenes = []
    for s in range(args.scenes):
        gts, raws = scene(args.lines, 64, 200, seed=s)
        rows = -(-args.lines // 16)
        u = torch.rand((args.scene_points, 4), generator=g, device="cuda")
        cloud = torch.stack([u[:, 0] * 1920.0, u[:, 1] * (3.5 * rows + 4.0) - 2.0, (u[:, 2] - 0.5) * 0.1, u[:, 3] * 60.0], 1)
        items = [{"position": gt - origin, "noisy_candidates": [raw - origin], "context_lines": []}
                 for gt, raw in zip(gts, raws)]
        scenes.append((cloud.contiguous(), items))
    out = {"step": "reference", "device": torch.cuda.get_device_name(0), "lines": args.lines, "scene_points": args.scene_points}
    out.update(compare(model, scenes, {}))
    return out


def report(args, parts):
    first = parts.get("detector") or parts.get("reference")
    lines = [f"""Data-set evaluation per scene (metrics.evaluate_scene in a loop) against one metrics.evaluate_scenes call, same process.
Command: python scripts/evaluate_scenes_bench.py   (--frames {args.frames} --lanes {args.lanes} --detector-points {args.detector_points} --scenes {args.scenes} --lines {args.lines} --scene-points {args.scene_points})
Machine: 1 x MI355X (reported as "{first['device']}"), one run, {time.strftime('%Y-%m-%d')}; each step in a process of its own.
Timing: wall clock around synchronised calls after a warm-up of both modes on the first four scenes, clouds resident on the
device; the loop is timed {LOOP_RUNS} times (its spread is the yardstick), the one call twice; the phases are timed once each on
the inputs the whole call builds.  Procedural weights.
"""]
    for name in ("detector", "reference"):
        r = parts.get(name)
        if r is None:
            continue
        lines.append(json.dumps(r))
        lines.append("")
        lines.append(f"{name}: {r['scenes']} scenes, {r['rows']} rows, {r['cloud_points']} cloud points: loop {r['loop_ms']} ms, "
                     f"one call {r['batched_ms']} ms (median loop / best call {r['speedup']:.2f}x).")
        lines.append(f"{name}: contexts + model {r['model_loop_ms']:.1f} -> {r['model_batched_ms']:.1f} ms, line metrics "
                     f"{r['lines_loop_ms']:.1f} -> {r['lines_batched_ms']:.1f} ms, calibration {r['calibration_loop_ms']:.1f} -> "
                     f"{r['calibration_batched_ms']:.1f} ms.")
        lines.append(f"{name}: library calls, loop {json.dumps(r['loop_calls'])}; one call {json.dumps(r['batched_calls'])} "
                     "(a sweep call is 2 launches, an upload and a read-back; a ragged sweep call 2 launches, 3 table "
                     "uploads, a stream sync and a read-back).")
        lines.append(f"{name}: refined lines of the two modes differ by at most {r['refined_max_abs_diff_m']:.3e} m; "
                     f"calibration equal: {r['calibration_equal']}.")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("detector", "reference", "report"), default=None)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--lanes", type=int, default=12)
    ap.add_argument("--detector-points", type=int, default=4_000_000)
    ap.add_argument("--scenes", type=int, default=50)
    ap.add_argument("--lines", type=int, default=256)
    ap.add_argument("--scene-points", type=int, default=200_000)
    ap.add_argument("--parts-dir", default=os.path.join(ROOT, "results", "evaluate_scenes_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_ragged_evaluation_bench.txt"))
    args = ap.parse_args()
    os.makedirs(args.parts_dir, exist_ok=True)
    part = lambda name: os.path.join(args.parts_dir, name + ".json")
    if args.step in ("detector", "reference"):
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("evaluate_scenes_bench.py needs a GPU")
        out = step_detector(args) if args.step == "detector" else step_reference(args)
        print(json.dumps(out))
        with open(part(args.step), "w") as f:
            json.dump(out, f)
        return
    if args.step is None:
        for name in ("detector", "reference"):           # one process and one time limit per GPU step; stop at the first failure
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name] + sys.argv[1:],
                                timeout=STEP_LIMIT_S[name]).returncode
            if rc != 0:
                raise SystemExit(f"step {name} ended with status {rc}: nothing more is started")
    parts = {name: json.load(open(part(name))) for name in ("detector", "reference") if os.path.exists(part(name))}
    if not parts:
        raise SystemExit("no step has run yet")
    report(args, parts)


if __name__ == "__main__":
    main()
