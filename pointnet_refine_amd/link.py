"""Carrier-free map fusion: which refined pieces of a drive are the same lane, when nothing says so.
``fuse.fuse_pieces`` takes pieces matched to a carrier line; a detector run gives a dozen unlabelled
polylines per camera frame.  This module links the refined pieces across frames
(``csrc/prh_link.hpp``; the rule is in ``include/pointnet_refine_hip.h``, "Piece linking - the rule",
and restated in ``tests/_link_oracle.py``), puts every cluster on one arc coordinate, drafts a carrier
per cluster from the pieces themselves and hands them to the standard fusion.

  link_pieces         HIP: candidate pairs from boxes (steps 1-2), two-way projection statistics of
                      every candidate (steps 3-4); host: which candidates are edges (step 5)
  sync_pieces         host: clusters, a spanning tree per cluster, sign and arc offset per piece (step 6)
  link_sync           HIP: steps 1-6 and cum on the device (csrc/prh_link_sync.hpp), the bits of
                      piece_cums, link_pieces and sync_pieces; fuse_unmatched(device_sync=True) and
                      refine_predictions(device_sync=True) go through it (default off)
  fuse_unmatched      steps 1-8 from ego-frame pieces: pieces_to_world, link_pieces, sync_pieces,
                      prh_fuse_gather for the draft carriers, fuse_pieces for the map
  refine_predictions  a detector run to a map: load_results, slice_cloud, fuse.refine_slices, fuse_unmatched

    res = refine_predictions(model, "DRIVE_annotation_raw_data", "results.json")
    fuse.write_map_json("map.json", res["fused"])

Candidates come from an all-pairs box test, O(P^2): measured at 2.0 ms for 24,000 pieces (2.9e8 tests)
and 11.5 ms for 100,008 pieces (5.0e9 tests) on one MI355X, next to 5.2 ms of prh_link_stats at 24,000
(profiles/r16_link_sync_bench.txt), so a spatial grid is not built and is not needed at 1e5 pieces.
The GPU functions have no CPU fallback: without a GPU they raise RuntimeError.
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
    ptr = G.csr_offsets(np.bincount(src, minlength=n)[:n])
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
def _link_stats(dev, world_t, frame, cum_t, gate):
    """Steps 1-4 on a CUDA (P,M,3) float64 tensor of shifted drive-frame points; cum_t (P,M) on the
    device, or a callable that gives it (asked only when there are candidates).  Returns (offsets
    (P+1,) numpy, offsets, pair_j, count, sums on the device)."""
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
        if callable(cum_t):
            cum_t = cum_t()
        L.check(lib.prh_link_stats(G.ptr(world_t), G.ptr(cum_t), n_p, m, G.ptr(offsets), G.ptr(pair_j), n_pairs,
                                   float(gate), G.ptr(count), G.ptr(sums), dev.index, G.stream(dev)), "prh_link_stats")
    return off, offsets, pair_j, count, sums


def _link(dev, world_t, frame, cum, gate, min_in, out_ratio):
    """Steps 1-5 on a CUDA (P,M,3) float64 tensor of shifted drive-frame points."""
    n_p = world_t.shape[0]
    off, _, pair_j, count, sums = _link_stats(dev, world_t, frame,
                                              lambda: torch.from_numpy(np.ascontiguousarray(cum)).to(dev), gate)
    count, sums = count.cpu().numpy(), sums.cpu().numpy()
    pairs = np.stack([np.repeat(np.arange(n_p, dtype=np.int64), np.diff(off)), pair_j.cpu().numpy().astype(np.int64)], 1)
    edge, rho, delta = edges_of(count[:, 0], count[:, 1], sums[:, 1], sums[:, 2], sums[:, 3], min_in, out_ratio)
    return {"pairs": pairs, "n_in": count[:, 0].copy(), "n_out": count[:, 1].copy(), "sum_d": sums[:, 0].copy(),
            "sum_self": sums[:, 1].copy(), "sum_other": sums[:, 2].copy(), "sum_dot": sums[:, 3].copy(), "edge": edge,
            "rho": rho, "delta": delta}


# ------------------------------------------------------------------ steps 5-6 on the device
KEY_LOW = 0xFFFFFFFF


def parent_key(n_in, a):
    """The 64-bit key a neighbour a with n_in points in offers a piece it could be the parent of:
    (n_in << 32) | (2^32 - 1 - a).  The largest key is the largest n_in, ties to the smallest a; 0
    means no offer.  0 <= n_in < 2^31, 0 <= a < 2^32."""
    n_in, a = int(n_in), int(a)
    if not (0 <= n_in < 1 << 31 and 0 <= a <= KEY_LOW):
        raise ValueError("parent_key: 0 <= n_in < 2^31 and 0 <= a < 2^32")
    return (n_in << 32) | (KEY_LOW - a)


def parent_of_key(key):
    """parent_key's inverse: (n_in, a)."""
    key = int(key)
    return key >> 32, KEY_LOW - (key & KEY_LOW)


def device_cums(dev, world_t):
    """(P,M) float64 on the device: piece_cums' bits from prh_link_cum."""
    n_p, m = world_t.shape[:2]
    cum_t = torch.zeros((n_p, m), dtype=torch.float64, device=dev)
    L.check(L.lib().prh_link_cum(G.ptr(world_t), n_p, m, G.ptr(cum_t), dev.index, G.stream(dev)), "prh_link_cum")
    return cum_t


def device_edges(dev, n_p, offsets, pair_j, count, sums, min_in, out_ratio):
    """Step 5 on the device.  Returns ({'pair_i' int32, 'edge' uint8, 'rho' int8, 'delta' float64}
    per candidate, {'ij' (E,2) int32, 'w' (E,2) int32 = n_in rho, 'delta' (E,) float64} the edges in
    candidate order), all CUDA tensors; one 8-byte read sizes the second."""
    lib = L.lib()
    n_pairs = int(pair_j.shape[0])
    per = {"pair_i": torch.zeros((n_pairs,), dtype=torch.int32, device=dev),
           "edge": torch.zeros((n_pairs,), dtype=torch.uint8, device=dev),
           "rho": torch.zeros((n_pairs,), dtype=torch.int8, device=dev),
           "delta": torch.zeros((n_pairs,), dtype=torch.float64, device=dev)}
    blocks = int(lib.prh_link_edges_blocks(n_pairs))
    scan = torch.zeros((2 * blocks + 1,), dtype=torch.int64, device=dev)
    L.check(lib.prh_link_edges(G.ptr(offsets), n_p, G.ptr(count), G.ptr(sums), n_pairs, int(min_in), int(out_ratio),
                               G.ptr(per["pair_i"]), G.ptr(per["edge"]), G.ptr(per["rho"]), G.ptr(per["delta"]),
                               G.ptr(scan), dev.index, G.stream(dev)), "prh_link_edges")
    n_edges = int(scan[blocks].item())
    edges = {"ij": torch.zeros((n_edges, 2), dtype=torch.int32, device=dev),
             "w": torch.zeros((n_edges, 2), dtype=torch.int32, device=dev),
             "delta": torch.zeros((n_edges,), dtype=torch.float64, device=dev)}
    L.check(lib.prh_link_edges_compact(G.ptr(per["pair_i"]), G.ptr(pair_j), G.ptr(count), G.ptr(per["edge"]),
                                       G.ptr(per["rho"]), G.ptr(per["delta"]), n_pairs, G.ptr(scan), n_edges,
                                       G.ptr(edges["ij"]), G.ptr(edges["w"]), G.ptr(edges["delta"]), dev.index,
                                       G.stream(dev)), "prh_link_edges_compact")
    return per, edges


def device_components(dev, n_p, edges):
    """Step 6's clusters on the device: (label (P,) int32 CUDA, the component's smallest member;
    rounds run).  One 4-byte read per round."""
    lib = L.lib()
    label = torch.arange(n_p, dtype=torch.int32, device=dev)
    changed = torch.zeros((1,), dtype=torch.int32, device=dev)
    n_edges, rounds = int(edges["ij"].shape[0]), 0
    while n_edges and n_p:
        L.check(lib.prh_link_label_round(G.ptr(edges["ij"]), n_edges, n_p, G.ptr(label), G.ptr(changed), dev.index,
                                         G.stream(dev)), "prh_link_label_round")
        rounds += 1
        if int(changed.item()) == 0:
            break
        if rounds > n_p + 1:
            raise RuntimeError("link: the component rounds did not settle")
    return label, rounds


def device_tree(dev, n_p, edges, label):
    """Step 6's spanning trees on the device: ({'level', 'parent', 'sign' int32, 'offset' float64}
    CUDA, levels run).  One 4-byte read per level."""
    lib = L.lib()
    t = {"level": torch.zeros((n_p,), dtype=torch.int32, device=dev),
         "parent": torch.zeros((n_p,), dtype=torch.int32, device=dev),
         "sign": torch.zeros((n_p,), dtype=torch.int32, device=dev),
         "offset": torch.zeros((n_p,), dtype=torch.float64, device=dev)}
    key = torch.zeros((n_p,), dtype=torch.int64, device=dev)           # the library reads it as uint64
    placed = torch.zeros((1,), dtype=torch.int32, device=dev)
    L.check(lib.prh_link_tree_init(G.ptr(label), n_p, G.ptr(t["level"]), G.ptr(t["parent"]), G.ptr(t["sign"]),
                                   G.ptr(t["offset"]), G.ptr(key), dev.index, G.stream(dev)), "prh_link_tree_init")
    n_edges, n = int(edges["ij"].shape[0]), 0
    while n_edges and n < n_p:
        L.check(lib.prh_link_tree_level(G.ptr(edges["ij"]), G.ptr(edges["w"]), G.ptr(edges["delta"]), n_edges, n_p, n,
                                        G.ptr(t["level"]), G.ptr(t["parent"]), G.ptr(t["sign"]), G.ptr(t["offset"]),
                                        G.ptr(key), G.ptr(placed), dev.index, G.stream(dev)), "prh_link_tree_level")
        if int(placed.item()) == 0:
            break
        n += 1
    return t, n


def _link_sync(dev, world_t, frame, gate, min_in, out_ratio, return_links):
    """Steps 1-6 on a CUDA (P,M,3) float64 tensor of shifted drive-frame points: link_sync's result."""
    n_p = int(world_t.shape[0])
    cum_t = device_cums(dev, world_t)
    off, offsets, pair_j, count, sums = _link_stats(dev, world_t, frame, cum_t, gate)
    per, edges = device_edges(dev, n_p, offsets, pair_j, count, sums, min_in, out_ratio)
    label, _ = device_components(dev, n_p, edges)
    tree, _ = device_tree(dev, n_p, edges, label)
    root = label == torch.arange(n_p, dtype=torch.int32, device=dev)
    rank = torch.cumsum(root.to(torch.int64), 0) - 1                   # integers: exact in any order
    cluster = rank[label.to(torch.int64)] if n_p else rank
    res = {"cluster": cluster.cpu().numpy(), "level": tree["level"].cpu().numpy().astype(np.int64),
           "parent": tree["parent"].cpu().numpy().astype(np.int64), "sign": tree["sign"].cpu().numpy().astype(np.int8),
           "offset": tree["offset"].cpu().numpy(), "cum": cum_t.cpu().numpy(), "candidates": int(pair_j.shape[0]),
           "edges": int(edges["ij"].shape[0])}
    if return_links:
        cnt, sm = count.cpu().numpy(), sums.cpu().numpy()
        res["links"] = {"pairs": np.stack([per["pair_i"].cpu().numpy().astype(np.int64),
                                           pair_j.cpu().numpy().astype(np.int64)], 1),
                        "n_in": cnt[:, 0].copy(), "n_out": cnt[:, 1].copy(), "sum_d": sm[:, 0].copy(),
                        "sum_self": sm[:, 1].copy(), "sum_other": sm[:, 2].copy(), "sum_dot": sm[:, 3].copy(),
                        "edge": per["edge"].cpu().numpy().astype(bool), "rho": per["rho"].cpu().numpy(),
                        "delta": per["delta"].cpu().numpy()}
    return res


def _origin_of(w, origin):
    if origin is None:
        return F.floor_km(w[0, 0]) if len(w) else np.zeros(3)
    return np.asarray(origin, dtype=np.float64).reshape(3)


def link_sync(world, piece_frame, gate=GATE, min_in=MIN_IN, out_ratio=OUT_RATIO, origin=None, return_links=False):
    """Steps 1-6 on the device: link_pieces' inputs; the candidates' statistics stay on the device.
    Returns sync_pieces' five arrays ('cluster', 'level', 'parent' int64, 'sign' int8, 'offset'
    float64, bitwise what sync_pieces(link_pieces(..)) gives) plus 'cum' (P,M) float64 (piece_cums'
    bits), 'candidates' and 'edges' (two ints); return_links=True adds 'links', link_pieces' dict,
    copied to the host only then.  Bitwise reproducible: csrc/prh_link_sync.hpp says why."""
    w = F._check_pieces(world, "link_sync")
    fr = F._check_index(piece_frame, len(w), np.iinfo(np.int32).max, "piece_frame", "link_sync")
    _check_params(gate, min_in, out_ratio, "link_sync")
    dev = G.device("link")
    shifted = np.ascontiguousarray(w - _origin_of(w, origin))
    return _link_sync(dev, torch.from_numpy(shifted).to(dev), fr, gate, min_in, out_ratio, return_links)


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
    shifted = np.ascontiguousarray(w - _origin_of(w, origin))
    return _link(dev, torch.from_numpy(shifted).to(dev), fr, piece_cums(shifted), gate, min_in, out_ratio)


def _draft_carriers(dev, world, g, line, n_lines, step):
    """Step 7: prh_fuse_gather with s := g over pieces grouped by line (already in line order).
    world (K,M,3), g (K,M) numpy.  Returns per line the (k,3) nodes with C >= 1, shifted frame."""
    top = np.zeros(n_lines)
    np.maximum.at(top, line, g.max(axis=1))
    node_off = F.node_offsets(top, step)
    w_t, g_t = torch.from_numpy(np.ascontiguousarray(world)).to(dev), torch.from_numpy(np.ascontiguousarray(g)).to(dev)
    X, _, C, _ = F.gather_nodes(dev, w_t, g_t, G.csr_offsets(np.bincount(line, minlength=n_lines)[:n_lines]), node_off, step)
    Xh, Ch = X.cpu().numpy(), C.cpu().numpy()
    return [Xh[node_off[l]:node_off[l + 1]][Ch[node_off[l]:node_off[l + 1]] >= 1] for l in range(n_lines)]


def fuse_unmatched(pieces, piece_pose, poses_xyzq, gate=GATE, min_in=MIN_IN, out_ratio=OUT_RATIO,
                   min_pieces=MIN_PIECES, step=F.STEP, min_count=F.MIN_COUNT, max_gap=F.MAX_GAP, origin=None,
                   return_nodes=False, device_sync=False, return_links=False):
    """Unlabelled refined pieces fused into one map (steps 1-8 of the rule).

    pieces (P,M,3), 2 <= M <= 64, piece p in the ego frame of poses_xyzq[piece_pose[p]]; the frame of
    a piece is its pose index.  Pieces are linked across frames, every cluster of at least
    min_pieces pieces gets a draft carrier from its own pieces, and fuse_pieces merges the kept
    pieces on those carriers.  Returns fused: per kept cluster the list of (k,3) polylines, as
    fuse_pieces does.  return_nodes=True also returns fuse_pieces' node dict (over the kept pieces,
    in the caller's order) plus 'cluster' (P,) the kept cluster of every piece, -1 for pieces of
    dropped clusters, 'sign' (P,), 'offset' (P,), 'g' (P,M), 'kept' (the kept pieces' indices),
    'carriers' [per kept cluster (k,3)], 'links' (link_pieces' dict) and sync_pieces' 'level',
    'parent' and, as 'clusters_all', its cluster numbers before any was dropped, and 'n_candidates'
    and 'n_edges' (two ints).  Bitwise reproducible.

    device_sync=True runs steps 1-6 through the device path (link_sync's: cum, edges, clusters and the
    spanning trees on the GPU, the candidates' statistics never copied to the host); arc_positions
    stays on the host.  'links' is then in the dict only with return_links=True; every other key and
    the map are bitwise the default's."""
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
    if device_sync:
        sync = _link_sync(dev, world_t, pp, gate, min_in, out_ratio, return_links)
        cum, links = sync["cum"], sync.get("links")
    else:
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
                 level=sync["level"], parent=sync["parent"], clusters_all=sync["cluster"])
    if links is not None:
        nodes["links"] = links
    if device_sync:
        nodes.update(n_candidates=sync["candidates"], n_edges=sync["edges"])
    else:
        nodes.update(n_candidates=int(len(links["edge"])), n_edges=int(links["edge"].sum()))
    return fused, nodes


@torch.no_grad()
def refine_predictions(model, drive_dir, results_json, num_line_points=32, num_context_points=1024, crop_radius=0.3,
                       decay_scale=2.0, seed=0, precision=None, segment_len=None, radius=None, max_pose_gap=None,
                       min_tube_points=F.MIN_TUBE_POINTS, gate=GATE, min_in=MIN_IN, out_ratio=OUT_RATIO,
                       min_pieces=MIN_PIECES, step=F.STEP, min_count=F.MIN_COUNT, max_gap=F.MAX_GAP, origin=None,
                       batched=False, support=False, support_radius=None, intensity_floor=0.0, device_sync=False,
                       return_links=False, lift=False, lift_radius=0.5, lift_step=1.0, align=False, align_max_shift=1.0,
                       align_radius=0.15, align_scope="frame", align_max_yaw=0.0):
    """A detector run refined into one drive-frame map, with no GT.

    drive_dir holds pose/*.json and merged.pcd; results_json is the detector's output
    (predictions.load_results).  A chain of the project's calls: load_frame_poses, load_results and
    match_poses pick a pose per camera frame; one drive.slice_cloud cuts the cloud of every frame
    that has a pose; fuse.refine_slices runs the model on every frame's device-resident slice with the
    pixel_to_ego lines as candidates, exactly what refine_drive does per slice (one io.scene_offsets
    call per frame, or with batched=True one io.scene_offsets_ragged call over all frames); a piece
    whose tube held fewer than min_tube_points cloud points is left out and counted; fuse_unmatched
    links and fuses the rest.
    device_sync and return_links go to fuse_unmatched: the same map and report, steps 5-6 on the device.
    lift=True puts the pixel_to_ego lines (z = 0) on the road first: one ground.lift_lines call over
    all frames' slices (stations every lift_step metres, cloud points within lift_radius in xy), and
    the lifted lines are the candidates; the report gains 'lift_lines', 'lift_lines_lifted',
    'lift_lines_unlifted', 'lift_stations' and 'lift_stations_without_ground'.
    align=True then moves every frame's lines in x y onto the paint: one align.align_lines call over
    all frames' slices (shifts up to align_max_shift per component, cloud points within align_radius
    of a shifted line, one shift per frame or - align_scope='drive' - one for the drive); it runs
    after the lift, because its distances are 3-D, and before the candidates are refined; the report
    gains 'align_frames', 'align_frames_aligned', 'align_frames_unaligned', 'align_shifts' (S,2),
    'align_score_zero', 'align_score_best' and 'align_candidates'.  align_max_yaw above 0 makes that
    one align.align_lines_rigid call: a yaw of up to align_max_yaw radians about each frame's ego
    origin is swept with the shift, for the heading error a shift cannot take out, and the report
    gains 'align_yaws' (S,); at 0.0 the shift-only path runs untouched.
    intensity_floor (the floor of support=True's scores) may be "auto": paintfloor.paint_floor reads it
    from the frames' slices, once, as soon as they are cut, and the report gains 'floor',
    'floor_surface_points', 'floor_paint_share' and 'floor_contrast'.

    Returns {'fused' [per kept cluster], 'pieces' (P,M,3) float64 ego frame, 'piece_frame' (P,) the
    row of 'poses' each piece was seen from, 'piece_slice' (the same), 'pose_index' (per used frame
    the pose's number), 'poses' (S,7), 'nodes' (fuse_unmatched's dict), 'report': {'slices',
    'pieces', 'pieces_sparse', 'nodes', 'nodes_used', 'fused_polylines', 'candidates', 'edges',
    'clusters', 'clusters_kept', 'pieces_unlinked'}}."""
    from . import drive as D
    from . import paintfloor as PF
    from . import predictions as PR
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
    pieces, piece_frame, sparse = np.zeros((0, m, 3)), np.zeros(0, dtype=np.int64), 0
    cloud = None
    lift_report = {"lines": 0, "lines_lifted": 0, "lines_unlifted": 0, "stations": 0, "stations_without_ground": 0}
    align_report = {"frames": 0, "frames_aligned": 0, "frames_unaligned": 0, "shifts": np.zeros((0, 2)),
                    "score_zero": np.zeros(0, dtype=np.int64), "score_best": np.zeros(0, dtype=np.int64), "candidates": 0}
    if len(with_pose):
        cloud = np.ascontiguousarray(D.load_merged_cloud(drive_dir), dtype=np.float32).reshape(-1, 4)
        points, offsets, _ = D.slice_cloud(cloud, pq, segment_len, PR.RADIUS if radius is None else radius)
        off = offsets.cpu().numpy()
        intensity_floor, floor_report = PF.resolve(intensity_floor, points, off, "refine_predictions")
        cands_all = [[PR.pixel_to_ego(px) for px in frames[n]["pixels"]] for n in with_pose]
        if lift:
            from . import ground as GR
            cands_all, lift_report = GR.lift_lines(points, off, cands_all, step=lift_step, radius=lift_radius)
        if align:
            from . import align as AL
            cands_all, align_report = AL.align(points, off, cands_all, align_max_yaw, max_shift=align_max_shift,
                                               radius=align_radius, scope=align_scope)
        pieces, piece_frame, _, sparse = F.refine_slices(model, points, off, cands_all, m, num_context_points, crop_radius,
                                                         decay_scale, seed, precision, min_tube_points, batched)
    else:
        intensity_floor, floor_report = PF.resolve(intensity_floor, None, None, "refine_predictions")   # "auto" without a slice raises
    fused, nodes = fuse_unmatched(pieces, piece_frame, pq, gate, min_in, out_ratio, min_pieces, step, min_count, max_gap,
                                  origin, return_nodes=True, device_sync=device_sync, return_links=return_links)
    all_clusters = nodes["clusters_all"]
    report = F.refine_report(len(with_pose), pieces, sparse, nodes, fused, min_count)
    report.update({"candidates": int(nodes["n_candidates"]), "edges": int(nodes["n_edges"]),
                   "clusters": int(all_clusters.max()) + 1 if len(all_clusters) else 0, "clusters_kept": len(fused),
                   "pieces_unlinked": int((nodes["cluster"] < 0).sum())})
    if lift:
        report.update({"lift_" + k: v for k, v in lift_report.items()})
    if align:
        if float(align_max_yaw) > 0.0:
            align_report.setdefault("yaws", np.zeros(0))
        report.update({"align_" + k: v for k, v in align_report.items()})
    if floor_report is not None:
        report.update(PF.report_keys(floor_report))
    res = {"fused": fused, "pieces": pieces, "piece_frame": piece_frame, "piece_slice": piece_frame.copy(),
           "pose_index": [int(c) for c in chosen[with_pose]], "poses": pq, "nodes": nodes, "report": report}
    if support:
        if cloud is None:
            cloud = np.ascontiguousarray(D.load_merged_cloud(drive_dir), dtype=np.float32).reshape(-1, 4)
        res["support"] = F.cloud_support(cloud, fused, None, step, crop_radius if support_radius is None else support_radius,
                                         intensity_floor, nodes["origin"])
    return res
