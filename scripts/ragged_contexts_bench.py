"""Times the contexts-plus-model part of fuse.refine_drive and link.refine_predictions per slice
(io.scene_offsets in a loop) and batched (one io.scene_offsets_ragged call) in the same run, and
writes a report (default profiles/r12_ragged_contexts_bench.txt) that ends in one JSON line per step:

  drive     fuse.refine_drive on the generated 80-slice drive of map_fusion_bench.py (4 M points,
            6 lines, procedural weights), whole, per slice and batched; the model side of both
            modes on the slices of one slice_cloud call; the ragged build split into resampling,
            count pass (prh_context_ragged_count + the read-back), select pass
            (prh_context_ragged_select) and the forward
  detector  the same model-side comparison at --frames frames of --lanes lines (the generated run of
            link_bench.py as candidates, a cloud of --detector-points points along its path).
            Reading the files and fuse_unmatched are the same code in both modes and are not timed.

Without --step every step runs in a child process of its own, under its own time limit, and the
first failure ends the run; the report is written from the steps' JSON files.

    python scripts/ragged_contexts_bench.py [--step drive|detector|report] [--frames 2000] [--lanes 12] [--out FILE]
"""
import argparse
import ctypes as C
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

STEP_LIMIT_S = {"drive": 240, "detector": 420}


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


def model_side(model, pts, oh, cands, seed=0):
    """Both modes of the contexts-plus-model part on resident slices.  Returns a dict of wall-clock ms
    (after a warm-up of each mode on the first slices) and the ragged build's phases."""
    import torch
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    from pointnet_refine_amd import context as CX
    from pointnet_refine_amd import fuse
    from pointnet_refine_amd.io import scene_offsets
    used = [si for si, c in enumerate(cands) if c and oh[si + 1] > oh[si]]

    def loop(which):
        n = 0
        for si in which:
            out = scene_offsets(model, pts[oh[si]:oh[si + 1]].to(torch.float32), cands[si], seed=seed * 1000003 + si,
                                return_counts=True)
            (out[1] + out[2][:, None, :] + out[0]).to(torch.float64).cpu()
            out[3].cpu()
            n += len(cands[si])
        return n

    def batched(which_cands):
        return fuse.refine_slices(model, pts, oh, which_cands, 32, 1024, 0.3, 2.0, seed, None, fuse.MIN_TUBE_POINTS, batched=True)

    loop(used[:4])
    batched([c if si in used[:4] else [] for si, c in enumerate(cands)])
    loop_ms, n_lines = wall_ms(lambda: loop(used))
    batched_ms, res = wall_ms(lambda: batched(cands))

    # ---- the ragged build in phases, on the same inputs refine_slices(batched=True) builds
    dev = pts.device
    lib = L.lib()
    points = pts.to(torch.float32)
    raw = [v for si in used for v in cands[si]]
    ls = np.repeat(np.asarray(used, dtype=np.int32), [len(cands[si]) for si in used])
    so = np.ascontiguousarray(oh, dtype=np.int64)
    seeds = np.array([(seed * 1000003 + si) & 0xFFFFFFFFFFFFFFFF for si in range(len(so) - 1)], dtype=np.uint64)
    resample_ms, (dense, line) = wall_ms(lambda: (CX.resample_polylines_device(raw, CX.DENSE_POINTS, dev).float(),
                                                  CX.resample_polylines_device(raw, 32, dev).float()))
    n_l, n_s = len(raw), len(so) - 1
    items = int(CX.ragged_block_offsets(so, ls)[-1])
    nb = lib.prh_context_ragged_workspace_bytes(n_l, items)
    ws = G.workspace(nb, dev)
    counts = torch.empty((n_l,), dtype=torch.int32, device=dev)
    co = torch.empty((n_l + 1,), dtype=torch.int64, device=dev)
    out = torch.empty((n_l, 1024, 4), dtype=torch.float32, device=dev)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    p = G.ptr

    def count():
        L.check(lib.prh_context_ragged_count(p(points), hp(so), n_s, p(dense), 200, hp(ls), hp(seeds), n_l, 0.3, p(counts),
                                             p(co), p(ws), nb, dev.index, G.stream(dev)), "prh_context_ragged_count")
        return int(co[-1].item())

    count_ms, total = wall_ms(count)
    cand = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)
    keys = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)

    def select():
        L.check(lib.prh_context_ragged_select(p(points), hp(so), n_s, p(dense), 200, p(line), 32, hp(ls), n_l, 0.3, 2.0, 1024,
                                              p(counts), p(co), 0, n_l, p(cand), p(keys), total, p(out), p(ws), nb,
                                              dev.index, G.stream(dev)), "prh_context_ragged_select")

    select_ms, _ = wall_ms(select)
    centres = line.mean(dim=1)
    noisy_c = line - centres[:, None, :]

    def forward():
        with torch.no_grad():
            return torch.cat([model(out[s:s + 2048], noisy_c[s:s + 2048])[-1] for s in range(0, n_l, 2048)])

    forward_ms, _ = wall_ms(forward)
    return {"slices_used": len(used), "lines": n_lines, "points_in_slices": int(oh[-1]), "work_items": items,
            "candidates": total, "candidate_bytes_csr": total * CX.CANDIDATE_BYTES,
            "candidate_bytes_fixed_slots": n_l * 8192 * 8, "pieces": int(len(res[0])),
            "per_slice_ms": round(loop_ms, 1), "batched_ms": round(batched_ms, 1),
            "speedup": round(loop_ms / batched_ms, 2), "ragged_resample_ms": round(resample_ms, 2),
            "ragged_count_ms": round(count_ms, 2), "ragged_select_ms": round(select_ms, 2),
            "ragged_forward_ms": round(forward_ms, 2)}


def step_drive(args):
    import torch
    from map_fusion_bench import make_drive
    from pointnet_refine_amd import drive, fuse
    rng = np.random.default_rng(0)
    model = procedural_model()
    cloud, dposes, dlines = make_drive(args.cloud_points, args.slices, 6, rng)
    cl = torch.from_numpy(cloud).cuda()
    out = {"step": "drive", "device": torch.cuda.get_device_name(0), "cloud_points": args.cloud_points}
    for mode in (False, True):
        fuse.refine_drive(model, cl, dposes, dlines, batched=mode)                 # warm-up
        ms, res = wall_ms(lambda: fuse.refine_drive(model, cl, dposes, dlines, batched=mode))
        out["refine_drive_batched_ms" if mode else "refine_drive_per_slice_ms"] = round(ms, 1)
        out["report_batched" if mode else "report_per_slice"] = res["report"]
    chosen = drive.plan_slices(dposes)
    pq = dposes[chosen]
    pts, offs, _ = drive.slice_cloud(cl, pq)
    clipped = drive.clip_lines(dlines, pq)
    out.update(model_side(model, pts, offs.cpu().numpy(), [[v for _, v in kept] for kept in clipped]))
    out["slices"] = len(chosen)
    return out


def step_detector(args):
    import torch
    from link_bench import make_run, path_y
    from pointnet_refine_amd import drive
    rng = np.random.default_rng(0)
    model = procedural_model()
    pieces, frame, poses = make_run(args.frames, args.lanes, rng)
    x = rng.uniform(0.0, poses[-1, 0] + 30.0, args.detector_points)
    cloud = np.column_stack([x, path_y(x) + rng.uniform(-21.0, 21.0, len(x)), 0.2 * np.sin(x / 45.0) + rng.normal(0.0, 0.03, len(x)),
                             rng.uniform(0.0, 60.0, len(x))]).astype(np.float32)
    pts, offs, _ = drive.slice_cloud(torch.from_numpy(cloud).cuda(), poses, 50.0, 60.0)
    cands = [[pieces[f * args.lanes + l] for l in range(args.lanes)] for f in range(args.frames)]
    out = {"step": "detector", "device": torch.cuda.get_device_name(0), "frames": args.frames, "lanes": args.lanes,
           "cloud_points": args.detector_points}
    out.update(model_side(model, pts, offs.cpu().numpy(), cands))
    return out


def report(args, parts):
    d, t = parts.get("drive"), parts.get("detector")
    lines = [f"""Contexts + model per slice (io.scene_offsets in a loop) against batched (one io.scene_offsets_ragged call), same run.
Command: python scripts/ragged_contexts_bench.py   (--slices {args.slices} --cloud-points {args.cloud_points} --frames {args.frames} --lanes {args.lanes} --detector-points {args.detector_points})
Machine: 1 x MI355X (reported as "{(d or t)['device']}"), one run, {time.strftime('%Y-%m-%d')}; each step in a process of its own.
Timing: wall clock around synchronised calls, one timed run after a warm-up (of the whole for refine_drive, of both modes
on the first four slices for the model side); the phases of the ragged build are timed one by one on the same inputs.
"""]
    for name, r in (("drive", d), ("detector", t)):
        if r is None:
            continue
        lines.append(json.dumps(r))
        lines.append("")
        if name == "drive":
            lines.append(f"refine_drive whole, {r['slices']} slices, {r['cloud_points']} cloud points: per slice "
                         f"{r['refine_drive_per_slice_ms']:.1f} ms, batched {r['refine_drive_batched_ms']:.1f} ms.")
        lines.append(f"{name}: contexts + model, {r['slices_used']} slices, {r['lines']} lines: per slice {r['per_slice_ms']:.1f} ms, "
                     f"batched {r['batched_ms']:.1f} ms ({r['speedup']:.2f}x).")
        lines.append(f"{name}: ragged build in phases: resampling {r['ragged_resample_ms']:.2f} ms, count pass + read-back "
                     f"{r['ragged_count_ms']:.2f} ms ({r['work_items']} work items), select pass {r['ragged_select_ms']:.2f} ms "
                     f"({r['candidates']} candidates), forward {r['ragged_forward_ms']:.2f} ms.")
        lines.append(f"{name}: candidate memory {r['candidate_bytes_csr'] / 1e6:.1f} MB in CSR against "
                     f"{r['candidate_bytes_fixed_slots'] / 1e6:.1f} MB at 8192 fixed slots per line.")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("drive", "detector", "report"), default=None)
    ap.add_argument("--slices", type=int, default=80)
    ap.add_argument("--cloud-points", type=int, default=4_000_000)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--lanes", type=int, default=12)
    ap.add_argument("--detector-points", type=int, default=4_000_000)
    ap.add_argument("--parts-dir", default=os.path.join(ROOT, "results", "ragged_contexts_bench"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_ragged_contexts_bench.txt"))
    args = ap.parse_args()
    os.makedirs(args.parts_dir, exist_ok=True)
    part = lambda name: os.path.join(args.parts_dir, name + ".json")
    if args.step in ("drive", "detector"):
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("ragged_contexts_bench.py needs a GPU")
        out = step_drive(args) if args.step == "drive" else step_detector(args)
        print(json.dumps(out))
        with open(part(args.step), "w") as f:
            json.dump(out, f)
        return
    if args.step is None:
        for name in ("drive", "detector"):               # one process and one time limit per GPU step; stop at the first failure
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name] + sys.argv[1:],
                                timeout=STEP_LIMIT_S[name]).returncode
            if rc != 0:
                raise SystemExit(f"step {name} ended with status {rc}: nothing more is started")
    parts = {name: json.load(open(part(name))) for name in ("drive", "detector") if os.path.exists(part(name))}
    if not parts:
        raise SystemExit("no step has run yet")
    report(args, parts)


if __name__ == "__main__":
    main()
