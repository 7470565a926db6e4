"""Times piece linking (csrc/prh_link.hpp, pointnet_refine_amd/link.py) on a detector-run-sized
input and writes a report (default profiles/r11_piece_links_bench.txt) that ends in one JSON line:

  pairs_ms          prh_link_pairs_count + prh_link_pairs_write on resident buffers, device events:
                    --frames frames x --lanes lines of 32 points on generated lanes (24,000 pieces
                    by default), all-pairs box tests
  stats_ms          prh_link_stats over every candidate, device events, and its rate in
                    (point, segment) tests per second: candidates x 2 x 32 x 31
  host_ms           steps 5-6 on the host (edges_of, sync_pieces, arc_positions), wall clock
  fuse_unmatched_ms the whole of link.fuse_unmatched from ego-frame pieces, wall clock around a
                    synchronised call after one warm-up call
  oracle_ms_scaled  tests/_link_oracle.py (plain Python loops) on the first --oracle-frames frames,
                    SCALED by candidate pairs to the size of the run - an estimate

    python scripts/link_bench.py [--frames 2000] [--lanes 12] [--oracle-frames 12] [--out FILE]
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
TEST_INSTRUCTIONS = 30          # fp64 add / mul per (point, segment) test, as in map_fusion_bench.py
M = 32


def path_y(x):
    return 10.0 * np.sin(x / 80.0)


def make_run(n_frames, n_lanes, rng, spacing=2.5):
    """n_frames poses `spacing` m apart along a winding path, n_lanes lanes 3.5 m apart; per frame
    every lane over ego |x| <= 25 as 32 points with 5 cm noise, every third piece reversed."""
    import _fuse_oracle as O
    px = 30.0 + spacing * np.arange(n_frames)
    yaw = np.arctan(np.cos(px / 80.0) / 8.0)
    poses = np.column_stack([px, path_y(px), np.zeros_like(px), np.zeros_like(px), np.zeros_like(px), np.sin(yaw / 2),
                             np.cos(yaw / 2)])
    pieces = np.empty((n_frames * n_lanes, M, 3))
    for f in range(n_frames):
        x = px[f] + np.linspace(-25.0, 25.0, M)
        for l in range(n_lanes):
            w = np.column_stack([x, path_y(x) + 3.5 * (l - (n_lanes - 1) / 2), 0.2 * np.sin(x / 45.0)])
            pieces[f * n_lanes + l] = O.to_ego(w + rng.normal(0.0, 0.05, w.shape), poses[f])
    pieces[::3] = pieces[::3, ::-1].copy()
    return pieces, np.repeat(np.arange(n_frames), n_lanes), poses


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
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--lanes", type=int, default=12)
    ap.add_argument("--oracle-frames", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_piece_links_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("link_bench.py needs a GPU")
    import _link_oracle as K
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    from pointnet_refine_amd import fuse, link
    dev = G.device("link")
    lib = L.lib()
    rng = np.random.default_rng(0)
    pieces, frame, poses = make_run(args.frames, args.lanes, rng)
    n_p = len(pieces)
    org = fuse.default_origin(poses)
    ps = poses.copy()
    ps[:, :3] -= org
    world_t, _, _, _ = fuse._project(dev, pieces, None, frame, ps, None, None)
    world = world_t.cpu().numpy()
    cum_ms, cum = wall_ms(lambda: link.piece_cums(world))
    cum_t = torch.from_numpy(cum).to(dev)
    fr_t = torch.from_numpy(frame.astype(np.int32)).to(dev)
    offsets = torch.zeros((n_p + 1,), dtype=torch.int64, device=dev)
    nb = lib.prh_link_pairs_workspace_bytes(n_p)
    ws = G.workspace(nb, dev)

    def count():
        L.check(lib.prh_link_pairs_count(G.ptr(world_t), n_p, M, G.ptr(fr_t), 1.0, G.ptr(offsets), G.ptr(ws), nb, dev.index,
                                         G.stream(dev)), "prh_link_pairs_count")

    count()
    n_pairs = int(offsets[-1].item())
    pair_j = torch.empty((n_pairs,), dtype=torch.int32, device=dev)
    cnt = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
    sums = torch.empty((n_pairs, 4), dtype=torch.float64, device=dev)

    def pairs():
        count()
        L.check(lib.prh_link_pairs_write(G.ptr(world_t), n_p, M, G.ptr(fr_t), 1.0, G.ptr(offsets), G.ptr(pair_j), G.ptr(ws),
                                         nb, dev.index, G.stream(dev)), "prh_link_pairs_write")

    def stats():
        L.check(lib.prh_link_stats(G.ptr(world_t), G.ptr(cum_t), n_p, M, G.ptr(offsets), G.ptr(pair_j), n_pairs, 1.0,
                                   G.ptr(cnt), G.ptr(sums), dev.index, G.stream(dev)), "prh_link_stats")

    pairs_all = events_ms(pairs, args.reps)
    stats_all = events_ms(stats, args.reps)
    pairs_ms, stats_ms = float(np.median(pairs_all)), float(np.median(stats_all))
    tests = float(n_pairs) * 2 * M * (M - 1)
    rate = tests / (stats_ms * 1e-3)

    links = link._link(dev, world_t, frame, cum, 1.0, link.MIN_IN, link.OUT_RATIO)

    def host():
        link.edges_of(links["n_in"], links["n_out"], links["sum_self"], links["sum_other"], links["sum_dot"])
        s = link.sync_pieces(n_p, links)
        link.arc_positions(cum, s)
        return s

    host_ms, sync = wall_ms(host)
    link.fuse_unmatched(pieces, frame, poses)                          # warm-up
    whole_ms, (fused, nodes) = wall_ms(lambda: link.fuse_unmatched(pieces, frame, poses, return_nodes=True))

    # ---- the Python restatement on the first frames, scaled by candidate pairs
    k = args.oracle_frames * args.lanes
    t = time.perf_counter()
    small = K.link(world[:k], frame[:k])
    oracle_ms = (time.perf_counter() - t) * 1e3
    oracle_scaled = oracle_ms * n_pairs / max(len(small["edge"]), 1)

    out = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "lanes": args.lanes, "pieces": n_p,
           "points_per_piece": M, "box_tests": n_p * (n_p - 1) // 2, "candidates": n_pairs,
           "candidates_per_piece": round(2.0 * n_pairs / n_p, 1), "edges": int(links["edge"].sum()), "reps": args.reps,
           "pairs_ms": round(pairs_ms, 3), "pairs_ms_all": [round(v, 3) for v in pairs_all],
           "stats_ms": round(stats_ms, 3), "stats_ms_all": [round(v, 3) for v in stats_all],
           "point_segment_tests": tests, "tests_per_s": rate, "test_instructions": TEST_INSTRUCTIONS,
           "stats_share_of_fp64_vector_rate": round(rate * TEST_INSTRUCTIONS / FP64_LANE_RATE, 3),
           "piece_cums_ms": round(cum_ms, 1), "host_ms": round(host_ms, 1), "clusters": int(sync["cluster"].max()) + 1,
           "tree_levels": int(sync["level"].max()), "fuse_unmatched_ms": round(whole_ms, 1), "clusters_kept": len(fused),
           "fused_polylines": int(sum(len(f) for f in fused)), "oracle_ms_measured": round(oracle_ms, 1),
           "oracle_pieces_timed": k, "oracle_pairs_timed": int(len(small["edge"])), "oracle_ms_scaled": round(oracle_scaled, 0)}
    text = f"""Piece linking: prh_link_pairs_count / _write and prh_link_stats on a detector-run-sized input, link.fuse_unmatched whole.
Command: python scripts/link_bench.py   (--frames {args.frames} --lanes {args.lanes} --oracle-frames {args.oracle_frames} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, {time.strftime('%Y-%m-%d')}.
Timing: device events around the library calls on resident buffers, median of {args.reps} after one warm-up call;
the host steps and fuse_unmatched by wall clock around synchronised calls (fuse_unmatched after one warm-up call).
Algorithmic work of link_stats: candidates x 2 directions x {M} points x {M - 1} segments = {tests:.3g} (point, segment)
tests, {TEST_INSTRUCTIONS} fp64 add / mul instructions per test by the source (FMA contraction is off by the rule), against
the spec fp64 vector rate of 39.3e12 lane-instructions/s (a spec figure, not measured here).

{json.dumps(out)}

pairs count + write runs (ms): {[round(v, 3) for v in pairs_all]}
link_stats runs (ms):          {[round(v, 3) for v in stats_all]}
pairs: {n_p} pieces, {out['box_tests']:.3g} box tests, {n_pairs} candidates ({out['candidates_per_piece']} per piece) in {pairs_ms:.3f} ms.
link_stats: {tests:.3g} tests in {stats_ms:.3f} ms = {rate:.3g} tests/s = {out['stats_share_of_fp64_vector_rate']:.2f} of the fp64 vector rate.
host: piece_cums {cum_ms:.1f} ms; steps 5-6 {host_ms:.1f} ms ({out['edges']} edges, {out['clusters']} clusters, {out['tree_levels']} tree levels).
fuse_unmatched, steps 1-8 from ego pieces: {whole_ms:.1f} ms, {len(fused)} clusters kept, {out['fused_polylines']} polylines.
Python restatement (plain loops), steps 1-5: {oracle_ms:.0f} ms for {k} pieces / {len(small['edge'])} candidates; SCALED by candidates to
{n_pairs}: {oracle_scaled / 1e3:.0f} s (an estimate, not a measurement of that size).
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
