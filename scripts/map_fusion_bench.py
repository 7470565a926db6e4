"""Times map fusion (csrc/prh_fuse.hpp, pointnet_refine_amd/fuse.py) and writes a report
(default profiles/r10_map_fusion_bench.txt) that ends in one JSON line:

  project_ms        prh_fuse_project on resident buffers, device events: --pieces pieces of 32 points
                    (768 k points by default) of a prediction drive, spread over --lines carriers of
                    --vertices vertices each
  project_rate      (point, segment) pairs per second, and that rate as a share of the fp64 vector
                    rate: 30 fp64 add / mul instructions per pair by the source (9 differences, 12
                    products, 9 sums; the division runs only where the clamp does not decide)
                    against the spec 39.3e12 lane-instructions/s
  gather_ms         prh_fuse_gather of the same drive (range pass + gather), device events
  refine_drive_*    fuse.refine_drive on a generated --slices slice drive (procedural weights), wall
                    clock around synchronised calls, and its parts timed the way it calls them
  oracle_ms_scaled  tests/_fuse_oracle.py (plain Python loops) on one carrier with a few pieces,
                    SCALED by points to the size of the project + gather run - an estimate

    python scripts/map_fusion_bench.py [--pieces 24000] [--lines 12] [--vertices 2000] [--slices 80] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_LANE_RATE = 39.3e12        # MI355X spec fp64 vector rate, 78.6 TFLOP/s counting an FMA as 2
PAIR_INSTRUCTIONS = 30


def path_y(x):
    return 10.0 * np.sin(x / 80.0)


def make_carriers(n_lines, n_vertices, length, rng):
    lines = []
    for l in range(n_lines):
        x = np.sort(rng.uniform(0.0, length, n_vertices))
        x[0], x[-1] = 0.0, length
        lines.append(np.column_stack([x, path_y(x) + 3.5 * (l - n_lines / 2), 0.2 * np.sin(x / 45.0)]))
    return lines


def make_pieces(lines, n_pieces, m, rng):
    """Pieces of m points over 40 m stretches of their carrier, 5 cm noise, in an identity frame per
    25 m (the pose index only selects the translation here)."""
    import _fuse_oracle as O
    length = lines[0][-1, 0]
    n_poses = int(length // 25.0)
    poses = np.zeros((n_poses, 7))
    poses[:, 0] = 25.0 * np.arange(n_poses) + 12.5
    poses[:, 1] = path_y(poses[:, 0])
    yaw = np.arctan(np.cos(poses[:, 0] / 80.0) / 8.0)
    poses[:, 5], poses[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    piece_line = np.sort(rng.integers(0, len(lines), n_pieces))
    piece_pose = rng.integers(0, n_poses, n_pieces)
    pieces = np.empty((n_pieces, m, 3))
    for p in range(n_pieces):
        v = lines[piece_line[p]]
        x = np.clip(poses[piece_pose[p], 0] + np.linspace(-20.0, 20.0, m), 0.0, length)
        w = np.column_stack([x, np.interp(x, v[:, 0], v[:, 1]), np.interp(x, v[:, 0], v[:, 2])])
        pieces[p] = O.to_ego(w + rng.normal(0.0, 0.05, w.shape), poses[piece_pose[p]])
    return pieces, piece_line, piece_pose, poses


def make_drive(n_points, n_slices, n_lines, rng):
    length = 25.0 * (n_slices + 1)
    px = 25.0 * np.arange(0, n_slices + 2)
    yaw = np.arctan(np.cos(px / 80.0) / 8.0)
    poses = np.column_stack([px, path_y(px), np.zeros_like(px), np.zeros_like(px), np.zeros_like(px), np.sin(yaw / 2),
                             np.cos(yaw / 2)])
    x = rng.uniform(-10.0, length + 10.0, n_points)
    cloud = np.column_stack([x, path_y(x) + rng.uniform(-9.0, 9.0, n_points), rng.normal(0.0, 0.03, n_points),
                             rng.uniform(0.0, 60.0, n_points)]).astype(np.float32)
    lines = []
    for l in range(n_lines):
        xs = np.linspace(0.0, length, int(length / 2.0))
        lines.append(np.column_stack([xs, path_y(xs) + 3.5 * (l - (n_lines - 1) / 2), np.zeros_like(xs)]))
    return cloud, poses, lines


def events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pieces", type=int, default=24000)
    ap.add_argument("--lines", type=int, default=12)
    ap.add_argument("--vertices", type=int, default=2000)
    ap.add_argument("--slices", type=int, default=80)
    ap.add_argument("--cloud-points", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_map_fusion_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("map_fusion_bench.py needs a GPU")
    import _fuse_oracle as O
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    from pointnet_refine_amd import drive, fuse
    from pointnet_refine_amd.io import scene_offsets
    dev = G.device("fuse")
    lib = L.lib()
    rng = np.random.default_rng(0)
    m = 32

    # ---- the two kernels on resident buffers
    length = 25.0 * 2000 / 10                           # a 2,000-frame drive at 2.5 m per frame
    lines = make_carriers(args.lines, args.vertices, length, rng)
    pieces, piece_line, piece_pose, poses = make_pieces(lines, args.pieces, m, rng)
    cums = [fuse.carrier_cum(v) for v in lines]
    verts, off_t, _ = G.lines_csr(lines, dev)
    cum_t = torch.from_numpy(np.concatenate(cums)).to(dev)
    pc = torch.from_numpy(pieces).to(dev)
    pl = torch.from_numpy(piece_line.astype(np.int32)).to(dev)
    pp = torch.from_numpy(piece_pose.astype(np.int32)).to(dev)
    ps = torch.from_numpy(poses).to(dev)
    n_p = args.pieces
    world = torch.empty((n_p, m, 3), dtype=torch.float64, device=dev)
    s = torch.empty((n_p, m), dtype=torch.float64, device=dev)
    d = torch.empty((n_p, m), dtype=torch.float64, device=dev)
    seg = torch.empty((n_p, m), dtype=torch.int32, device=dev)
    nb = lib.prh_fuse_project_workspace_bytes(len(poses))
    ws = G.workspace(nb, dev)

    def project():
        L.check(lib.prh_fuse_project(G.ptr(pc), n_p, m, G.ptr(pl), G.ptr(pp), G.ptr(ps), len(poses), G.ptr(verts),
                                     G.ptr(off_t), G.ptr(cum_t), len(lines), G.ptr(world), G.ptr(s), G.ptr(d), G.ptr(seg),
                                     G.ptr(ws), nb, dev.index, G.stream(dev)), "prh_fuse_project")

    project_all = events_ms(project, args.reps)
    counts = np.array([int(np.floor(c[-1] / 0.5)) + 1 for c in cums], dtype=np.int64)
    node_off = np.concatenate(([0], np.cumsum(counts)))
    piece_off = np.concatenate(([0], np.cumsum(np.bincount(piece_line, minlength=len(lines)))))
    n_nodes = int(node_off[-1])
    no_t, po_t = torch.from_numpy(node_off).to(dev), torch.from_numpy(piece_off).to(dev)
    X = torch.empty((n_nodes, 3), dtype=torch.float64, device=dev)
    W = torch.empty((n_nodes,), dtype=torch.float64, device=dev)
    C = torch.empty((n_nodes,), dtype=torch.int32, device=dev)
    spread = torch.empty((n_nodes,), dtype=torch.float64, device=dev)
    nb2 = lib.prh_fuse_gather_workspace_bytes(n_p)
    ws2 = G.workspace(nb2, dev)

    def gather():
        L.check(lib.prh_fuse_gather(G.ptr(world), G.ptr(s), n_p, m, G.ptr(po_t), len(lines), G.ptr(no_t), n_nodes, 0.5,
                                    G.ptr(X), G.ptr(W), G.ptr(C), G.ptr(spread), G.ptr(ws2), nb2, dev.index, G.stream(dev)),
                "prh_fuse_gather")

    gather_all = events_ms(gather, args.reps)
    project_ms, gather_ms = float(np.median(project_all)), float(np.median(gather_all))
    pairs = float(n_p) * m * (args.vertices - 1)
    pair_rate = pairs / (project_ms * 1e-3)
    used = int((C > 0).sum().item())
    mean_c = float(C.double().mean().item())
    mean_d = float(d.mean().item())

    # ---- the numpy restatement on one carrier, scaled by points
    k = 4
    sel = np.flatnonzero(piece_line == 0)[:k]
    t = time.perf_counter()
    O.fuse([lines[0]], pieces[sel], np.zeros(k, dtype=np.int64), piece_pose[sel], poses, origin=np.zeros(3))
    oracle_ms = (time.perf_counter() - t) * 1e3
    oracle_scaled = oracle_ms * n_p / k

    # ---- refine_drive on a generated drive, whole and in parts
    from pointnet_refine_amd.model import LineRefineNet
    from oracle import procedural as P
    model = LineRefineNet()
    model.load_state_dict(P.linerefine_state_dict(0))
    model = model.cuda().eval()
    cloud, dposes, dlines = make_drive(args.cloud_points, args.slices, 6, rng)
    cl = torch.from_numpy(cloud).to(dev)
    fuse.refine_drive(model, cl, dposes, dlines)                      # warm-up
    whole_ms, res = wall_ms(lambda: fuse.refine_drive(model, cl, dposes, dlines))
    chosen = drive.plan_slices(dposes)
    pq = dposes[chosen]
    slice_ms, (pts, offs, _) = wall_ms(lambda: drive.slice_cloud(cl, pq))
    clip_ms, clipped = wall_ms(lambda: drive.clip_lines(dlines, pq))
    oh = offs.cpu().numpy()

    def model_side():
        for si, kept in enumerate(clipped):
            if kept and oh[si + 1] > oh[si]:
                out = scene_offsets(model, pts[oh[si]:oh[si + 1]].to(torch.float32), [v for _, v in kept], seed=si,
                                    return_counts=True)
                (out[1] + out[2][:, None, :] + out[0]).to(torch.float64).cpu()

    model_ms, _ = wall_ms(model_side)
    fuse_ms, _ = wall_ms(lambda: fuse.fuse_pieces(dlines, res["pieces"], res["piece_line"], res["piece_slice"], res["poses"],
                                                  return_nodes=True))
    err = fuse.map_error(res["fused"], dlines)

    out = {"device": torch.cuda.get_device_name(0), "pieces": n_p, "points": n_p * m, "lines": args.lines,
           "vertices_per_line": args.vertices, "pairs": pairs, "reps": args.reps,
           "project_ms": round(project_ms, 3), "project_ms_all": [round(v, 3) for v in project_all],
           "project_pairs_per_s": pair_rate, "pair_instructions": PAIR_INSTRUCTIONS,
           "project_share_of_fp64_vector_rate": round(pair_rate * PAIR_INSTRUCTIONS / FP64_LANE_RATE, 3),
           "nodes": n_nodes, "nodes_used": used, "mean_contributions": round(mean_c, 2), "mean_d_m": round(mean_d, 4),
           "gather_ms": round(gather_ms, 3), "gather_ms_all": [round(v, 3) for v in gather_all],
           "oracle_ms_measured": round(oracle_ms, 1), "oracle_pieces_timed": k, "oracle_ms_scaled": round(oracle_scaled, 0),
           "drive_slices": len(chosen), "drive_cloud_points": args.cloud_points, "drive_lines": len(dlines),
           "drive_pieces": res["report"]["pieces"], "drive_pieces_sparse": res["report"]["pieces_sparse"],
           "refine_drive_ms": round(whole_ms, 1), "refine_drive_slice_cloud_ms": round(slice_ms, 2),
           "refine_drive_clip_lines_ms": round(clip_ms, 2), "refine_drive_model_ms": round(model_ms, 1),
           "refine_drive_fuse_pieces_ms": round(fuse_ms, 2), "drive_map_mean_d_m": round(err["mean"], 4),
           "drive_map_coverage": round(err["coverage"], 4)}
    text = f"""Map fusion: prh_fuse_project / prh_fuse_gather on a prediction-drive-sized input, fuse.refine_drive on a generated drive.
Command: python scripts/map_fusion_bench.py   (--pieces {n_p} --lines {args.lines} --vertices {args.vertices} --slices {args.slices} --cloud-points {args.cloud_points} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, {time.strftime('%Y-%m-%d')}.
Timing: device events around the library calls on resident buffers, median of {args.reps} after one warm-up call;
refine_drive and its parts by wall clock around synchronised calls after one warm-up run of the whole.
Algorithmic work of fuse_project: points x carrier segments = {pairs:.3g} pairs, {PAIR_INSTRUCTIONS} fp64 add / mul instructions per
pair by the source (FMA contraction is off by the rule), against the spec fp64 vector rate of 39.3e12
lane-instructions/s (78.6 TFLOP/s counting an FMA as 2; a spec figure, not measured here).

{json.dumps(out)}

fuse_project runs (ms): {[round(v, 3) for v in project_all]}
fuse_gather runs (ms):  {[round(v, 3) for v in gather_all]}
fuse_project: {n_p * m} points x {args.vertices - 1} segments in {project_ms:.3f} ms = {pair_rate:.3g} pairs/s = {out['project_share_of_fp64_vector_rate']:.2f} of the fp64 vector rate.
fuse_gather: {n_nodes} nodes ({used} used, {mean_c:.2f} contributions per node) from {n_p} pieces in {gather_ms:.3f} ms.
numpy restatement (plain Python loops): {oracle_ms:.0f} ms for {k} pieces on one carrier; SCALED by points to {n_p} pieces:
{oracle_scaled / 1e3:.0f} s (an estimate, not a measurement of that size).
refine_drive, {len(chosen)} slices, {args.cloud_points} cloud points, {len(dlines)} lines, {res['report']['pieces']} pieces: {whole_ms:.1f} ms, of which
slice_cloud {slice_ms:.2f} ms, clip_lines {clip_ms:.2f} ms, contexts + model per slice {model_ms:.1f} ms, fuse_pieces {fuse_ms:.2f} ms
(the parts are timed in separate calls after the whole; procedural weights, so the map's distance to the
input, {err['mean']:.4f} m mean, says nothing about accuracy).
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
