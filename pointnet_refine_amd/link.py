"""Carrier-free map fusion: which refined pieces of a drive are the same lane, when nothing says so.
``fuse.fuse_pieces`` takes pieces matched to a carrier line; a detector run gives a dozen unlabelled
polylines per camera frame.  This module links the refined pieces across frames
(``csrc/prh_link.hpp``; the rule is in ``include/pointnet_refine_hip.h``, "Piece linking - the rule",
and restated in ``tests/_link_oracle.py``), puts every cluster on one arc coordinate, drafts a carrier
per cluster from the pieces themselves and hands them to the standard fusion.

  link_pieces         HIP: candidate pairs from boxes (steps 1-2), two-way projection statistics of
                      every candidate (steps 3-4); host: which candidates are edges (step 5)
  sync_pieces         host: clusters, a spanning tree per cluster, sign and arc offset per piece (step 6)
  fuse_unmatched      steps 1-8 from ego-frame pieces: pieces_to_world, link_pieces, sync_pieces,
                      prh_fuse_gather for the draft carriers, fuse_pieces for the map
  refine_predictions  a detector run to a map: load_results, slice_cloud, io.scene_offsets per frame,
                      fuse_unmatched

    res = refine_predictions(model, "DRIVE_annotation_raw_data", "results.json")
    fuse.write_map_json("map.json", res["fused"])

Candidates come from an all-pairs box test, O(P^2): right for a drive (2.9e8 tests at 24,000 pieces);
a spatial grid for maps beyond about 1e5 pieces is not built.  The GPU functions have no CPU
fallback: without a GPU they raise RuntimeError.
"""
import os

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L
from . import fuse as F

GATE = 1.0                   # metres: a point within this distance of the other piece is in
MIN_IN = 4
OUT_RATIO = 4
MIN_PIECES = 2


# ------------------------------------------------------------------ host side
def piece_cums(world):
    """(P,M) cumulative arc length of every piece: fuse.carrier_cum per piece."""
    w = np.asarray(world, dtype=np.float64)
    return np.stack([F.carrier_cum(p) for p in w]) if len(w) else np.zeros(w.shape[:2])


def _check_params(gate, min_in, out_ratio, what):
    if not float(gate) >= 0.0:
        raise ValueError(f"{what}: gate must not be negative")
    if int(min_in) < 1 or int(out_ratio) < 0:
        raise ValueError(f"{what}: min_in >= 1 and out_ratio >= 0")


def edges_of(n_in, n_out, sum_self, sum_other, sum_dot, min_in=MIN_IN, out_ratio=OUT_RATIO):
    """Step 5 for arrays of candidates: (edge bool, rho int8, delta float64).  delta is 0 where n_in is 0."""
    n_in, n_out = np.asarray(n_in, dtype=np.int64), np.asarray(n_out, dtype=np.int64)
    edge = (n_in >= int(min_in)) & (int(out_ratio) * n_out <= n_in)
    rho = np.where(np.asarray(sum_dot) >= 0.0, 1, -1).astype(np.int8)
    delta = np.zeros(len(n_in))
    has = n_in > 0
    delta[has] = (np.asarray(sum_self)[has] - rho[has] * np.asarray(sum_other)[has]) / n_in[has].astype(np.float64)
    return edge, rho, delta


def _ranges(start, count):
    """The concatenation of arange(start[k], start[k] + count[k])."""
    total = int(count.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    first = np.cumsum(count) - count
    return np.repeat(start - first, count) + np.arange(total, dtype=np.int64)


def sync_pieces(n_pieces, links):
    """Step 6: clusters and one arc coordinate per cluster from link_pieces' result (the rows with
    'edge' are used; 'pairs', 'n_in', 'rho', 'delta' are read).  Host only.  Returns {'cluster' (P,)
    int64 numbered by ascending smallest member, 'level' (P,) int64, 'parent' (P,) int64 (-1 for
    roots), 'sign' (P,) int8, 'offset' (P,) float64}: point k of piece p sits at offset[p] + sign[p]
    * cum_p[k] on its cluster's arc.  Level-synchronous and vectorised: the work is a few numpy
    passes over the edges per tree level."""
    n = int(n_pieces)
    pairs = np.asarray(links["pairs"], dtype=np.int64).reshape(-1, 2)
    sel = np.flatnonzero(np.asarray(links["edge"], dtype=bool))
    if len(sel) and (pairs[sel].min() < 0 or pairs[sel].max() >= n):
        raise ValueError(f"sync_pieces: an edge refers to a piece outside 0..{n - 1}")
    ei, ej = pairs[sel, 0], pairs[sel, 1]
    e_in = np.asarray(links["n_in"], dtype=np.int64)[sel]
    e_rho = np.asarray(links["rho"], dtype=np.int64)[sel]
    e_delta = np.asarray(links["delta"], dtype=np.float64)[sel]
    # components: every piece takes the smallest label among its neighbours, then labels are chased
    # to their own label, until nothing moves; the label is the component's smallest member
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, ei, label[ej])
        np.minimum.at(new, ej, label[ei])
        while True:
            hop = new[new]
            if np.array_equal(hop, new):
                break
            new = hop
        if np.array_equal(new, label):
            break
        label = new
    roots = np.flatnonzero(label == np.arange(n))
    cluster = np.searchsorted(roots, label)
    # both directions of every edge, grouped by source: src -> (dst, edge number, src is the edge's i)
    src, dst = np.concatenate([ei, ej]), np.concatenate([ej, ei])
    num = np.concatenate([np.arange(len(ei)), np.arange(len(ei))])
    src_is_i = np.concatenate([np.ones(len(ei), dtype=bool), np.zeros(len(ei), dtype=bool)])
    order = np.argsort(src, kind="stable")
    src, dst, num, src_is_i = src[order], dst[order], num[order], src_is_i[order]
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(np.bincount(src, minlength=n)[:n]) if n else 0
    level = np.full(n, -1, dtype=np.int64)
    parent = np.full(n, -1, dtype=np.int64)
    sign = np.ones(n, dtype=np.int8)
    offset = np.zeros(n)
    level[roots] = 0
    front, depth = roots, 0
    while len(front):
        rows = _ranges(ptr[front], ptr[front + 1] - ptr[front])
        rows = rows[level[dst[rows]] < 0]
        if len(rows) == 0:
            break
        # per child the neighbour with the largest n_in, then the smallest index
        pick = np.lexsort((src[rows], -e_in[num[rows]], dst[rows]))
        rows = rows[pick]
        rows = rows[np.concatenate(([True], dst[rows][1:] != dst[rows][:-1]))]
        a, b, e = src[rows], dst[rows], num[rows]
        depth += 1
        level[b], parent[b] = depth, a
        sign[b] = (e_rho[e] * sign[a]).astype(np.int8)
        offset[b] = np.where(src_is_i[rows], offset[a] + sign[a] * e_delta[e], offset[a] - sign[b] * e_delta[e])
        front = b
    return {"cluster": cluster, "level": level, "parent": parent, "sign": sign, "offset": offset}


def arc_positions(cum, sync):
    """Step 6's last sentences: g (P,M) = offset + sign * cum, reversed where sign < 0 so it ascends
    along every piece, minus the cluster's smallest g.  Returns (g, flip (P,) bool)."""
    cum = np.asarray(cum, dtype=np.float64)
    g = sync["offset"][:, None] + sync["sign"][:, None].astype(np.float64) * cum
    flip = sync["sign"] < 0
    g[flip] = g[flip, ::-1]
    if len(g):
        low = np.full(int(sync["cluster"].max()) + 1, np.inf)
        np.minimum.at(low, sync["cluster"], g.min(axis=1))
        g = g - low[sync["cluster"]][:, None]
    return g, flip


# ------------------------------------------------------------------ GPU side
def _link(dev, world_t, frame, cum, gate, min_in, out_ratio):
    """Steps 1-5 on a CUDA (P,M,3) float64 tensor of shifted drive-frame points."""
    n_p, m = world_t.shape[:2]
    lib = L.lib()
    fr = torch.from_numpy(frame.astype(np.int32)).to(dev)
    offsets = torch.zeros((n_p + 1,), dtype=torch.int64, device=dev)
    nb = lib.prh_link_pairs_workspace_bytes(n_p)
    ws = G.workspace(nb, dev)
    L.check(lib.prh_link_pairs_count(G.ptr(world_t), n_p, m, G.ptr(fr), float(gate), G.ptr(offsets), G.ptr(ws), nb,
                                     dev.index, G.stream(dev)), "prh_link_pairs_count")
    off = offsets.cpu().numpy()
    n_pairs = int(off[-1])
    pair_j = torch.empty((n_pairs,), dtype=torch.int32, device=dev)
    count = torch.zeros((n_pairs, 2), dtype=torch.int32, device=dev)
    sums = torch.zeros((n_pairs, 4), dtype=torch.float64, device=dev)
    if n_pairs:
        L.check(lib.prh_link_pairs_write(G.ptr(world_t), n_p, m, G.ptr(fr), float(gate), G.ptr(offsets), G.ptr(pair_j),
                                         G.ptr(ws), nb, dev.index, G.stream(dev)), "prh_link_pairs_write")
        cum_t = torch.from_numpy(np.ascontiguousarray(cum)).to(dev)
        L.check(lib.prh_link_stats(G.ptr(world_t), G.ptr(cum_t), n_p, m, G.ptr(offsets), G.ptr(pair_j), n_pairs,
                                   float(gate), G.ptr(count), G.ptr(sums), dev.index, G.stream(dev)), "prh_link_stats")
    count, sums = count.cpu().numpy(), sums.cpu().numpy()
    pairs = np.stack([np.repeat(np.arange(n_p, dtype=np.int64), np.diff(off)), pair_j.cpu().numpy().astype(np.int64)], 1)
    edge, rho, delta = edges_of(count[:, 0], count[:, 1], sums[:, 1], sums[:, 2], sums[:, 3], min_in, out_ratio)
    return {"pairs": pairs, "n_in": count[:, 0].copy(), "n_out": count[:, 1].copy(), "sum_d": sums[:, 0].copy(),
            "sum_self": sums[:, 1].copy(), "sum_other": sums[:, 2].copy(), "sum_dot": sums[:, 3].copy(), "edge": edge,
            "rho": rho, "delta": delta}


def link_pieces(world, piece_frame, gate=GATE, min_in=MIN_IN, out_ratio=OUT_RATIO, origin=None):
    """Steps 1-5: world (P,M,3) pieces in the drive frame, 2 <= M <= 64 (pieces_to_world's result),
    piece_frame (P,) the frame each was seen in.  origin (default: the first point rounded down to
    1000 m) is subtracted before the upload.  Returns, for all candidates in the rule's order,
    {'pairs' (E,2) int64, 'n_in', 'n_out' (E,) int32, 'sum_d', 'sum_self', 'sum_other', 'sum_dot'
    (E,) float64, 'edge' (E,) bool, 'rho' (E,) int8, 'delta' (E,) float64}.  Bitwise reproducible."""
    w = F._check_pieces(world, "link_pieces")
    fr = F._check_index(piece_frame, len(w), np.iinfo(np.int32).max, "piece_frame", "link_pieces")
    _check_params(gate, min_in, out_ratio, "link_pieces")
    dev = G.device("link")
    if origin is None:
        org = np.floor(w[0, 0] / 1000.0) * 1000.0 if len(w) else np.zeros(3)
    else:
        org = np.asarray(origin, dtype=np.float64).reshape(3)
    shifted = np.ascontiguousarray(w - org)
    return _link(dev, torch.from_numpy(shifted).to(dev), fr, piece_cums(shifted), gate, min_in, out_ratio)


def _draft_carriers(dev, world, g, line, n_lines, step):
    """Step 7: prh_fuse_gather with s := g over pieces grouped by line (already in line order).
    world (K,M,3), g (K,M) numpy.  Returns per line the (k,3) nodes with C >= 1, shifted frame."""
    lib = L.lib()
    n_k, m = g.shape
    top = np.zeros(n_lines)
    np.maximum.at(top, line, g.max(axis=1))
    counts = np.floor(top / float(step)).astype(np.int64) + 1
    node_off = np.zeros(n_lines + 1, dtype=np.int64)
    node_off[1:] = np.cumsum(counts)
    piece_off = np.zeros(n_lines + 1, dtype=np.int64)
    piece_off[1:] = np.cumsum(np.bincount(line, minlength=n_lines)[:n_lines])
    n_nodes = int(node_off[-1])
    X = torch.zeros((n_nodes, 3), dtype=torch.float64, device=dev)
    W = torch.zeros((n_nodes,), dtype=torch.float64, device=dev)
    C = torch.zeros((n_nodes,), dtype=torch.int32, device=dev)
    spread = torch.zeros((n_nodes,), dtype=torch.float64, device=dev)
    w_t, g_t = torch.from_numpy(np.ascontiguousarray(world)).to(dev), torch.from_numpy(np.ascontiguousarray(g)).to(dev)
    po_t, no_t = torch.from_numpy(piece_off).to(dev), torch.from_numpy(node_off).to(dev)
    nb = lib.prh_fuse_gather_workspace_bytes(n_k)
    ws = G.workspace(nb, dev)
    L.check(lib.prh_fuse_gather(G.ptr(w_t), G.ptr(g_t), n_k, m, G.ptr(po_t), n_lines, G.ptr(no_t), n_nodes, float(step),
                                G.ptr(X), G.ptr(W), G.ptr(C), G.ptr(spread), G.ptr(ws), nb, dev.index, G.stream(dev)),
            "prh_fuse_gather")
    Xh, Ch = X.cpu().numpy(), C.cpu().numpy()
    return [Xh[node_off[l]:node_off[l + 1]][Ch[node_off[l]:node_off[l + 1]] >= 1] for l in range(n_lines)]


def fuse_unmatched(pieces, piece_pose, poses_xyzq, gate=GATE, min_in=MIN_IN, out_ratio=OUT_RATIO,
                   min_pieces=MIN_PIECES, step=F.STEP, min_count=F.MIN_COUNT, max_gap=F.MAX_GAP, origin=None,
                   return_nodes=False):
    """Unlabelled refined pieces fused into one map (steps 1-8 of the rule).

    pieces (P,M,3), 2 <= M <= 64, piece p in the ego frame of poses_xyzq[piece_pose[p]]; the frame of
    a piece is its pose index.  Pieces are linked across frames, every cluster of at least
    min_pieces pieces gets a draft carrier from its own pieces, and fuse_pieces merges the kept
    pieces on those carriers.  Returns fused: per kept cluster the list of (k,3) polylines, as
    fuse_pieces does.  return_nodes=True also returns fuse_pieces' node dict (over the kept pieces,
    in the caller's order) plus 'cluster' (P,) the kept cluster of every piece, -1 for pieces of
    dropped clusters, 'sign' (P,), 'offset' (P,), 'g' (P,M), 'kept' (the kept pieces' indices),
    'carriers' [per kept cluster (k,3)], 'links' (link_pieces' dict) and sync_pieces' 'level',
    'parent' and, as 'clusters_all', its cluster numbers before any was dropped.  Bitwise reproducible."""
    pc = F._check_pieces(pieces, "fuse_unmatched")
    poses = F._check_poses(poses_xyzq, "fuse_unmatched")
    n_p, m = pc.shape[:2]
    pp = F._check_index(piece_pose, n_p, len(poses), "piece_pose", "fuse_unmatched")
    _check_params(gate, min_in, out_ratio, "fuse_unmatched")
    if not float(step) > 0.0:
        raise ValueError("fuse_unmatched: step must be positive")
    dev = G.device("link")
    org = F._origin(origin, poses)
    ps = poses.copy()
    ps[:, :3] -= org
    if n_p:
        world_t, _, _, _ = F._project(dev, pc, None, pp, ps, None, None)
    else:
        world_t = torch.zeros((0, m, 3), dtype=torch.float64, device=dev)
    world = world_t.cpu().numpy()
    cum = piece_cums(world)
    links = _link(dev, world_t, pp, cum, gate, min_in, out_ratio)
    sync = sync_pieces(n_p, links)
    g, flip = arc_positions(cum, sync)
    size = np.bincount(sync["cluster"], minlength=0)
    big = np.flatnonzero(size >= int(min_pieces))
    # draft carriers of the clusters that are large enough, pieces grouped by cluster in their order
    rank = np.full(len(size), -1, dtype=np.int64)
    rank[big] = np.arange(len(big))
    line = rank[sync["cluster"]] if n_p else np.zeros(0, dtype=np.int64)
    sel = np.flatnonzero(line >= 0)
    sel = sel[np.argsort(line[sel], kind="stable")]
    turned = world.copy()
    turned[flip] = turned[flip, ::-1]
    drafts = _draft_carriers(dev, turned[sel], g[sel], line[sel], len(big), step) if len(big) else []
    good = np.array([len(d) >= 2 for d in drafts], dtype=bool)
    final = np.full(len(big), -1, dtype=np.int64)
    final[good] = np.arange(int(good.sum()))
    cluster = np.where(line >= 0, final[np.maximum(line, 0)], -1) if len(big) else np.full(n_p, -1, dtype=np.int64)
    kept = np.flatnonzero(cluster >= 0)
    carriers = [d + org for d, ok in zip(drafts, good) if ok]
    ego = pc.copy()
    ego[flip] = ego[flip, ::-1]
    fused, nodes = F.fuse_pieces(carriers, ego[kept], cluster[kept], pp[kept], poses, step, min_count, max_gap, org,
                                 return_nodes=True)
    if not return_nodes:
        return fused
    nodes.update(cluster=cluster, sign=sync["sign"], offset=sync["offset"], g=g, kept=kept, carriers=carriers,
                 links=links, level=sync["level"], parent=sync["parent"], clusters_all=sync["cluster"])
    return fused, nodes


@torch.no_grad()
def refine_predictions(model, drive_dir, results_json, num_line_points=32, num_context_points=1024, crop_radius=0.3,
                       decay_scale=2.0, seed=0, precision=None, segment_len=None, radius=None, max_pose_gap=None,
                       min_tube_points=F.MIN_TUBE_POINTS, gate=GATE, min_in=MIN_IN, out_ratio=OUT_RATIO,
                       min_pieces=MIN_PIECES, step=F.STEP, min_count=F.MIN_COUNT, max_gap=F.MAX_GAP, origin=None,
                       batched=False, support=False, support_radius=None, intensity_floor=0.0):
    """A detector run refined into one drive-frame map, with no GT.

    drive_dir holds pose/*.json and merged.pcd; results_json is the detector's output
    (predictions.load_results).  A chain of the project's calls: load_frame_poses, load_results and
    match_poses pick a pose per camera frame; one drive.slice_cloud cuts the cloud of every frame
    that has a pose; per frame, io.scene_offsets runs the model on that frame's device-resident slice
    with the pixel_to_ego lines as candidates, exactly what refine_drive does per slice; a piece
    whose tube held fewer than min_tube_points cloud points is left out and counted; fuse_unmatched
    links and fuses the rest.  batched=True replaces the per-frame loop by one
    io.scene_offsets_ragged call over all frames (fuse.refine_slices_batched), as in refine_drive.

    Returns {'fused' [per kept cluster], 'pieces' (P,M,3) float64 ego frame, 'piece_frame' (P,) the
    row of 'poses' each piece was seen from, 'piece_slice' (the same), 'pose_index' (per used frame
    the pose's number), 'poses' (S,7), 'nodes' (fuse_unmatched's dict), 'report': {'slices',
    'pieces', 'pieces_sparse', 'nodes', 'nodes_used', 'fused_polylines', 'candidates', 'edges',
    'clusters', 'clusters_kept', 'pieces_unlinked'}}."""
    from . import drive as D
    from . import predictions as PR
    from .io import load_pcd_data, scene_offsets
    G.device("link")
    m = int(num_line_points)
    if not 2 <= m <= F.MAX_POINTS:
        raise ValueError(f"refine_predictions: 2..{F.MAX_POINTS} points per line, got {num_line_points}")
    segment_len = PR.SEGMENT_LEN if segment_len is None else segment_len
    poses = PR.load_frame_poses(os.path.join(drive_dir, "pose"))
    frames = PR.load_results(results_json)
    chosen = PR.match_poses([fr["ts"] for fr in frames], [p["ts"] for p in poses],
                            PR.MAX_POSE_GAP_NS if max_pose_gap is None else max_pose_gap)
    with_pose = np.flatnonzero(chosen >= 0)
    pq = D.poses_xyzq(poses, chosen[with_pose]) if len(with_pose) else np.zeros((0, 7))
    pieces, piece_frame, sparse = [], [], 0
    cloud = None
    if len(with_pose):
        cloud = np.atleast_2d(load_pcd_data(os.path.join(drive_dir, "merged.pcd")))[:, :4]
        points, offsets, _ = D.slice_cloud(np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4), pq, segment_len,
                                           PR.RADIUS if radius is None else radius)
        off = offsets.cpu().numpy()
        if batched:
            pieces, piece_frame, _, sparse = F.refine_slices_batched(
                model, points, off, [[PR.pixel_to_ego(px) for px in frames[n]["pixels"]] for n in with_pose], m,
                num_context_points, crop_radius, decay_scale, seed, precision, min_tube_points)
        else:
            for si, n in enumerate(with_pose):
                cands = [PR.pixel_to_ego(px) for px in frames[n]["pixels"]]
                if not cands:
                    continue
                if off[si + 1] == off[si]:
                    sparse += len(cands)                   # no cloud at all in this frame's slice
                    continue
                pts = points[off[si]:off[si + 1]].to(torch.float32)
                offset, noisy_c, centres, counts = scene_offsets(model, pts, cands, m, num_context_points, crop_radius,
                                                                 decay_scale, seed=int(seed) * 1000003 + si,
                                                                 precision=precision, return_counts=True)
                refined = (noisy_c + centres[:, None, :] + offset).to(torch.float64).cpu().numpy()
                keep = counts.cpu().numpy() >= int(min_tube_points)
                sparse += int((~keep).sum())
                for r in np.flatnonzero(keep):
                    pieces.append(refined[r])
                    piece_frame.append(si)
    pieces = np.stack(pieces) if len(pieces) else np.zeros((0, m, 3))
    piece_frame = np.asarray(piece_frame, dtype=np.int64)
    fused, nodes = fuse_unmatched(pieces, piece_frame, pq, gate, min_in, out_ratio, min_pieces, step, min_count, max_gap,
                                  origin, return_nodes=True)
    all_clusters = nodes["clusters_all"]
    report = {"slices": int(len(with_pose)), "pieces": int(len(pieces)), "pieces_sparse": int(sparse),
              "nodes": int(len(nodes["C"])), "nodes_used": int((nodes["C"] >= min_count).sum()),
              "fused_polylines": int(sum(len(f) for f in fused)), "candidates": int(len(nodes["links"]["edge"])),
              "edges": int(nodes["links"]["edge"].sum()),
              "clusters": int(all_clusters.max()) + 1 if len(all_clusters) else 0, "clusters_kept": len(fused),
              "pieces_unlinked": int((nodes["cluster"] < 0).sum())}
    res = {"fused": fused, "pieces": pieces, "piece_frame": piece_frame, "piece_slice": piece_frame.copy(),
           "pose_index": [int(c) for c in chosen[with_pose]], "poses": pq, "nodes": nodes, "report": report}
    if support:
        if cloud is None:
            cloud = np.atleast_2d(load_pcd_data(os.path.join(drive_dir, "merged.pcd")))[:, :4]
        res["support"] = F.cloud_support(np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4), fused, None, step,
                                         crop_radius if support_radius is None else support_radius, intensity_floor,
                                         nodes["origin"])
    return res
