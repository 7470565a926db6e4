"""Times steps 5-6 of piece linking (edges, clusters, arc synchronisation) and the cum of the inputs
on the host against the device path (csrc/prh_link_sync.hpp, link.link_sync) on the detector-run-
sized input of scripts/link_bench.py, in one process, and writes a report (default
profiles/r16_link_sync_bench.txt) that ends in one JSON line:

  host_*_ms           link.piece_cums, link.edges_of and link.sync_pieces, wall clock, and the copy
                      of the candidates' statistics to the host that they need (pair_j, pair_count,
                      pair_sum: 44 B per candidate)
  device_*_ms         prh_link_cum, prh_link_edges + _compact, the component rounds and the tree
                      levels (with their counts), wall clock around synchronised calls: the rounds
                      and levels read a flag each, so the host is part of them
  fuse_unmatched_*    link.fuse_unmatched whole, default and device_sync=True, wall clock
  pairs_ms_*          prh_link_pairs_count + prh_link_pairs_write alone (device events) at the run's
                      size and at --big-frames frames (100,008 pieces by default), next to
                      prh_link_stats at the run's size: what the all-pairs box test costs

    python scripts/link_sync_bench.py [--frames 2000] [--lanes 12] [--big-frames 8334] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

M = 32
BYTES_PER_CANDIDATE = 4 + 2 * 4 + 4 * 8          # pair_j, pair_count, pair_sum


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--lanes", type=int, default=12)
    ap.add_argument("--big-frames", type=int, default=8334)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_link_sync_bench.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("link_sync_bench.py needs a GPU")
    from link_bench import events_ms, make_run, wall_ms
    from pointnet_refine_amd import _gpu as G
    from pointnet_refine_amd import _lib as L
    from pointnet_refine_amd import fuse, link
    dev = G.device("link")
    lib = L.lib()

    def median_wall(fn):
        fn()
        runs = [wall_ms(fn)[0] for _ in range(args.reps)]
        return float(np.median(runs)), [round(v, 3) for v in runs]

    def project(pieces, frame, poses):
        ps = poses.copy()
        ps[:, :3] -= fuse.default_origin(poses)
        return fuse._project(dev, pieces, None, frame, ps, None, None)[0]

    def pairs_ms(world_t, frame):
        n_p = world_t.shape[0]
        fr_t = torch.from_numpy(frame.astype(np.int32)).to(dev)
        offsets = torch.zeros((n_p + 1,), dtype=torch.int64, device=dev)
        nb = lib.prh_link_pairs_workspace_bytes(n_p)
        ws = G.workspace(nb, dev)

        def count():
            L.check(lib.prh_link_pairs_count(G.ptr(world_t), n_p, M, G.ptr(fr_t), 1.0, G.ptr(offsets), G.ptr(ws), nb,
                                             dev.index, G.stream(dev)), "prh_link_pairs_count")

        count()
        n_pairs = int(offsets[-1].item())
        pair_j = torch.empty((n_pairs,), dtype=torch.int32, device=dev)

        def both():
            count()
            L.check(lib.prh_link_pairs_write(G.ptr(world_t), n_p, M, G.ptr(fr_t), 1.0, G.ptr(offsets), G.ptr(pair_j),
                                             G.ptr(ws), nb, dev.index, G.stream(dev)), "prh_link_pairs_write")

        runs = events_ms(both, args.reps)
        return float(np.median(runs)), [round(v, 3) for v in runs], n_pairs, offsets, pair_j

    # ---- the run of link_bench.py
    pieces, frame, poses = make_run(args.frames, args.lanes, np.random.default_rng(0))
    n_p = len(pieces)
    world_t = project(pieces, frame, poses)
    world = world_t.cpu().numpy()
    p_ms, p_all, n_pairs, offsets, pair_j = pairs_ms(world_t, frame)
    cum_t = link.device_cums(dev, world_t)
    count = torch.zeros((n_pairs, 2), dtype=torch.int32, device=dev)
    sums = torch.zeros((n_pairs, 4), dtype=torch.float64, device=dev)

    def stats():
        L.check(lib.prh_link_stats(G.ptr(world_t), G.ptr(cum_t), n_p, M, G.ptr(offsets), G.ptr(pair_j), n_pairs, 1.0,
                                   G.ptr(count), G.ptr(sums), dev.index, G.stream(dev)), "prh_link_stats")

    stats_all = events_ms(stats, args.reps)
    stats_ms = float(np.median(stats_all))

    # ---- host: the copy, then cum, step 5, step 6
    def copy_down():
        return pair_j.cpu().numpy(), count.cpu().numpy(), sums.cpu().numpy()

    copy_ms, copy_all = median_wall(copy_down)
    host_cum_ms, host_cum_all = median_wall(lambda: link.piece_cums(world))
    cum = link.piece_cums(world)
    links = link._link(dev, world_t, frame, cum, 1.0, link.MIN_IN, link.OUT_RATIO)
    host_edges_ms, host_edges_all = median_wall(
        lambda: link.edges_of(links["n_in"], links["n_out"], links["sum_self"], links["sum_other"], links["sum_dot"]))
    host_sync_ms, host_sync_all = median_wall(lambda: link.sync_pieces(n_p, links))
    want = link.sync_pieces(n_p, links)

    # ---- device: cum, step 5, components, trees
    dev_cum_ms, dev_cum_all = median_wall(lambda: link.device_cums(dev, world_t))
    dev_edges_ms, dev_edges_all = median_wall(
        lambda: link.device_edges(dev, n_p, offsets, pair_j, count, sums, link.MIN_IN, link.OUT_RATIO))
    per, edges = link.device_edges(dev, n_p, offsets, pair_j, count, sums, link.MIN_IN, link.OUT_RATIO)
    dev_comp_ms, dev_comp_all = median_wall(lambda: link.device_components(dev, n_p, edges))
    label, rounds = link.device_components(dev, n_p, edges)
    dev_tree_ms, dev_tree_all = median_wall(lambda: link.device_tree(dev, n_p, edges, label))
    tree, levels = link.device_tree(dev, n_p, edges, label)
    got = link.link_sync(world, frame, origin=np.zeros(3))
    same = all(got[k].tobytes() == want[k].tobytes() for k in want) and got["cum"].tobytes() == cum.tobytes()
    n_edges = int(edges["ij"].shape[0])

    # ---- fuse_unmatched whole, both ways
    whole_host_ms, whole_host_all = median_wall(lambda: link.fuse_unmatched(pieces, frame, poses))
    whole_dev_ms, whole_dev_all = median_wall(lambda: link.fuse_unmatched(pieces, frame, poses, device_sync=True))
    fa = link.fuse_unmatched(pieces, frame, poses)
    fb = link.fuse_unmatched(pieces, frame, poses, device_sync=True)
    same_map = len(fa) == len(fb) and all(x.tobytes() == y.tobytes() for p, q in zip(fa, fb) for x, y in zip(p, q))

    # ---- the all-pairs box test at a map's size
    del count, sums, links, per
    big_pieces, big_frame, big_poses = make_run(args.big_frames, args.lanes, np.random.default_rng(1))
    big_world_t = project(big_pieces, big_frame, big_poses)
    big_ms, big_all, big_pairs, _, _ = pairs_ms(big_world_t, big_frame)
    n_big = len(big_pieces)

    host_total = copy_ms + host_cum_ms + host_edges_ms + host_sync_ms
    dev_total = dev_cum_ms + dev_edges_ms + dev_comp_ms + dev_tree_ms
    d2h_device = n_p * (8 + 4 + 4 + 4 + 8) + n_p * M * 8 + 8 + 4 * (rounds + levels + 1)
    out = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "lanes": args.lanes, "pieces": n_p,
           "points_per_piece": M, "candidates": n_pairs, "edges": n_edges, "clusters": int(want["cluster"].max()) + 1,
           "reps": args.reps, "bitwise_equal_sync": bool(same), "bitwise_equal_map": bool(same_map),
           "host_copy_ms": round(copy_ms, 3), "host_cum_ms": round(host_cum_ms, 3), "host_edges_ms": round(host_edges_ms, 3),
           "host_sync_ms": round(host_sync_ms, 3), "host_total_ms": round(host_total, 3),
           "device_cum_ms": round(dev_cum_ms, 3), "device_edges_ms": round(dev_edges_ms, 3),
           "device_components_ms": round(dev_comp_ms, 3), "component_rounds": rounds,
           "device_tree_ms": round(dev_tree_ms, 3), "tree_levels": levels, "device_total_ms": round(dev_total, 3),
           "d2h_bytes_avoided": n_pairs * BYTES_PER_CANDIDATE, "d2h_bytes_device_path": d2h_device,
           "fuse_unmatched_host_ms": round(whole_host_ms, 1), "fuse_unmatched_device_ms": round(whole_dev_ms, 1),
           "pairs_ms": round(p_ms, 3), "stats_ms": round(stats_ms, 3), "big_pieces": n_big,
           "big_box_tests": n_big * (n_big - 1) // 2, "big_candidates": big_pairs, "big_pairs_ms": round(big_ms, 3)}
    text = f"""Piece linking, steps 5-6 and cum: host (numpy) against the device path (prh_link_cum, prh_link_edges, prh_link_label_round,
prh_link_tree_level), and the all-pairs box test at a map's size.
Command: python scripts/link_sync_bench.py   (--frames {args.frames} --lanes {args.lanes} --big-frames {args.big_frames} --reps {args.reps})
Machine: 1 x MI355X (reported as "{out['device']}"), one run, one process, {time.strftime('%Y-%m-%d')}.
Timing: wall clock around synchronised calls, median of {args.reps} after one warm-up call, for everything but the pairs and
stats kernels (device events).  The component rounds and tree levels read one flag each, so their host time is in the figure.

host, runs (ms): copy of pair_j / pair_count / pair_sum {copy_all}; piece_cums {host_cum_all};
  edges_of {host_edges_all}; sync_pieces {host_sync_all}
device, runs (ms): cum {dev_cum_all}; edges + compact {dev_edges_all};
  components {dev_comp_all} ({rounds} rounds); trees {dev_tree_all} ({levels} levels)
{n_p} pieces, {n_pairs} candidates, {n_edges} edges, {out['clusters']} clusters.
host:   copy {copy_ms:.2f} + piece_cums {host_cum_ms:.2f} + edges_of {host_edges_ms:.2f} + sync_pieces {host_sync_ms:.2f} = {host_total:.2f} ms
device: cum {dev_cum_ms:.2f} + edges {dev_edges_ms:.2f} + components {dev_comp_ms:.2f} + trees {dev_tree_ms:.2f} = {dev_total:.2f} ms
device results bitwise equal to the host's: sync {same}, fused map {same_map}.
D2H avoided: {n_pairs * BYTES_PER_CANDIDATE} B ({BYTES_PER_CANDIDATE} B per candidate); the device path copies {d2h_device} B (per-piece arrays, cum, flags).
fuse_unmatched whole (ms): default {whole_host_all} median {whole_host_ms:.1f}; device_sync {whole_dev_all} median {whole_dev_ms:.1f}
pairs count + write: {n_p} pieces ({n_p * (n_p - 1) // 2:.3g} box tests) {p_all} median {p_ms:.3f} ms;
  {n_big} pieces ({out['big_box_tests']:.3g} box tests, {big_pairs} candidates) {big_all} median {big_ms:.3f} ms;
  prh_link_stats at {n_p} pieces {[round(v, 3) for v in stats_all]} median {stats_ms:.3f} ms.

{json.dumps(out)}
"""
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
