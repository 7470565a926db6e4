"""Map fusion: the last stage the reference does not have.  The refiner works on 50 m ego-frame
slices cut at a 25 m stride (``drive.py``), so every stretch of a line is refined twice, in two
frames; this module brings the refined pieces back to the drive frame and merges them into one
polyline per input line (``csrc/prh_fuse.hpp``; the rule is in ``include/pointnet_refine_hip.h``,
"Map fusion - the rule", and restated in ``tests/_fuse_oracle.py``).

  pieces_to_world    HIP: ego -> drive frame, w = R(q) p + t (step 1)
  project_to_lines   HIP: nearest point of a polyline for every point: arc position s, distance d,
                     segment (step 2)
  fuse_pieces        HIP: steps 1-5 (project, then one thread per 0.5 m node gathers the piece
                     segments that pass it) and the host's step 6 (nodes -> polylines)
  map_error          distance of a fused map to its lines and the share of their length it covers
  refine_slices      the slice refinement refine_drive and link.refine_predictions share: io.scene_offsets
                     per slice or one io.scene_offsets_ragged call, the sparse count, the tube cut
  refine_drive       plan_slices, slice_cloud, clip_lines, refine_slices, fuse_pieces
  cloud_support      refine_drive(support=True): support.map_support of the input lines and the fused map
  write_map_json     the drive file layout drive.load_gt_items reads

    res = refine_drive(model, "DRIVE_annotation_raw_data", None, [it["points"] for it in items])
    write_map_json("map.json", res["fused"])

The GPU functions have no CPU fallback: without a GPU they raise RuntimeError.
"""
import json
import os

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L

MAX_POINTS = 64              # points per piece (prh_fuse_max_points())
STEP = 0.5                   # node spacing in metres
MIN_COUNT = 1
MAX_GAP = 5.0
MIN_TUBE_POINTS = 32


# ------------------------------------------------------------------ host side
def floor_km(p):
    """p with each component rounded down to a multiple of 1000 m: the default origin of every tool
    that shifts world coordinates before an upload."""
    return np.floor(np.asarray(p, dtype=np.float64) / 1000.0) * 1000.0


def default_origin(poses_xyzq):
    """The first pose's translation with each component rounded down to a multiple of 1000 m."""
    p = np.asarray(poses_xyzq, dtype=np.float64).reshape(-1, 7)
    return floor_km(p[0, :3]) if len(p) else np.zeros(3)


def inverse_permutation(order):
    """back with back[order] = 0 .. n-1: rows taken in order go back to where they were with [back]."""
    back = np.empty_like(order)
    back[order] = np.arange(len(order))
    return back


def node_offsets(cums_or_lengths, step):
    """The node layout of fusion, support and the draft carriers: a line of arc length c has the
    nodes 0 .. floor(c / step).  cums_or_lengths: a list with every line's carrier_cum (a line
    without a vertex has no node) or an array of the lines' lengths.  Returns (L+1,) int64 offsets."""
    if isinstance(cums_or_lengths, np.ndarray):
        return G.csr_offsets(np.floor(cums_or_lengths / float(step)).astype(np.int64) + 1)
    return G.csr_offsets([int(np.floor(c[-1] / float(step))) + 1 if len(c) else 0 for c in cums_or_lengths])


def carrier_cum(verts):
    """Cumulative 3-D arc length of a polyline: cum[0] = 0, cum[k+1] = cum[k] + sqrt(|V[k+1] - V[k]|^2)."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    if len(v) == 0:
        return np.zeros(0)
    e = np.diff(v, axis=0)
    return np.concatenate(([0.0], np.cumsum(np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]))))


def _check_poses(poses_xyzq, what):
    from .predictions import _check_unit
    p = np.asarray(poses_xyzq.detach().cpu().numpy() if torch.is_tensor(poses_xyzq) else poses_xyzq, dtype=np.float64)
    if p.size % 7:
        raise ValueError(f"{what}: poses must be (S,7) x y z qx qy qz qw")
    p = p.reshape(-1, 7)
    _check_unit(p, what)
    return p


def _check_pieces(pieces, what, lo=2):
    a = np.asarray(pieces.detach().cpu().numpy() if torch.is_tensor(pieces) else pieces, dtype=np.float64)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{what}: pieces must be (P,M,3), got {a.shape}")
    if not lo <= a.shape[1] <= MAX_POINTS:
        raise ValueError(f"{what}: {lo}..{MAX_POINTS} points per piece, got {a.shape[1]}")
    return np.ascontiguousarray(a)


def _check_index(idx, n_rows, n_targets, name, what):
    a = np.asarray(idx)
    if a.ndim != 1 or len(a) != n_rows or (a.size and a.dtype.kind not in "iu"):
        raise ValueError(f"{what}: {name} must be {n_rows} integers")
    a = a.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() >= n_targets):
        raise ValueError(f"{what}: {name} outside 0..{n_targets - 1}")
    return a


def _origin(origin, poses):
    return default_origin(poses) if origin is None else np.asarray(origin, dtype=np.float64).reshape(3)


def _lines(lines, origin):
    """Polylines shifted by the origin, and their arc lengths."""
    shifted = [np.asarray(l, dtype=np.float64).reshape(-1, 3) - origin for l in lines]
    return shifted, [carrier_cum(v) for v in shifted]


def node_polylines(X, C, step=STEP, min_count=MIN_COUNT, max_gap=MAX_GAP):
    """Step 6 for the nodes of one line: the nodes with C >= min_count in node order, cut where two
    consecutive used nodes are more than max_gap metres of arc apart; runs of fewer than 2 nodes
    are dropped.  Returns a list of (k,3) arrays."""
    used = np.flatnonzero(np.asarray(C) >= min_count)
    if len(used) == 0:
        return []
    cuts = np.flatnonzero(np.diff(used) * float(step) > max_gap) + 1
    return [np.asarray(X)[r].copy() for r in np.split(used, cuts) if len(r) >= 2]


def write_map_json(json_path, fused, categories=None, attributes=None):
    """A fused map as a drive GT file (items[].category / attributes / position of {x,y,z}), the
    layout drive.load_gt_items reads.  fused: per line a list of (k,3) polylines; every polyline
    becomes one item with its line's category (default 'unknown') and attributes plus
    'source_line' (the line's index) and 'part' (the polyline's number within the line)."""
    from .drive import xyz_dicts
    items = []
    for l, parts in enumerate(fused):
        for k, pts in enumerate(parts):
            attr = dict(attributes[l]) if attributes is not None else {}
            attr.update(source_line=l, part=k)
            items.append({"category": categories[l] if categories is not None else "unknown", "attributes": attr,
                          "position": xyz_dicts(np.asarray(pts, dtype=np.float64).reshape(-1, 3))})
    with open(json_path, "w") as f:
        json.dump({"items": items}, f, indent=4)
    return len(items)


# ------------------------------------------------------------------ GPU side
def _project(dev, pieces, piece_line, piece_pose, poses, shifted, cums):
    """prh_fuse_project on (P,M,3) numpy pieces.  piece_pose None: pieces are in the (shifted) drive
    frame; piece_line None: transform only.  Returns CUDA (world (P,M,3), s, d (P,M), seg (P,M) int32);
    the last three are None without piece_line."""
    n_p, m = pieces.shape[:2]
    lib = L.lib()
    pc = torch.from_numpy(pieces).to(dev)
    world = torch.empty((n_p, m, 3), dtype=torch.float64, device=dev)
    pl = pp = ps = verts = off_t = cum_t = s = d = seg = None
    n_s = n_l = 0
    if piece_pose is not None:
        pp = torch.from_numpy(piece_pose.astype(np.int32)).to(dev)
        ps = G.poses(poses, dev, "fuse")
        n_s = ps.shape[0]
    if piece_line is not None:
        pl = torch.from_numpy(piece_line.astype(np.int32)).to(dev)
        verts, off_t, _ = G.lines_csr(shifted, dev)
        cum_t = torch.from_numpy(np.concatenate(cums) if len(cums) else np.zeros(0)).to(dev)
        n_l = len(shifted)
        s = torch.zeros((n_p, m), dtype=torch.float64, device=dev)
        d = torch.zeros((n_p, m), dtype=torch.float64, device=dev)
        seg = torch.full((n_p, m), -1, dtype=torch.int32, device=dev)
    nb = lib.prh_fuse_project_workspace_bytes(n_s)
    ws = G.workspace(nb, dev)
    L.check(lib.prh_fuse_project(G.ptr(pc), n_p, m, G.ptr(pl), G.ptr(pp), G.ptr(ps), n_s, G.ptr(verts), G.ptr(off_t),
                                 G.ptr(cum_t), n_l, G.ptr(world), G.ptr(s), G.ptr(d), G.ptr(seg), G.ptr(ws), nb, dev.index,
                                 G.stream(dev)), "prh_fuse_project")
    return world, s, d, seg


def gather_nodes(dev, world, s, piece_off, node_off, step):
    """prh_fuse_gather, the one driver of fuse_pieces and of link's draft carriers: world (P,M,3) and s
    (P,M) float64 CUDA with the pieces grouped by line, piece_off and node_off (L+1,) host offsets of
    every line's pieces and nodes (node_offsets), one node per step metres.  Returns CUDA (X (N,3),
    W (N,), C (N,) int32, spread (N,)), all 0 for a node nothing reaches."""
    n_p, m = world.shape[:2]
    n_l, n_nodes = len(node_off) - 1, int(node_off[-1])
    X = torch.zeros((n_nodes, 3), dtype=torch.float64, device=dev)
    W = torch.zeros((n_nodes,), dtype=torch.float64, device=dev)
    C = torch.zeros((n_nodes,), dtype=torch.int32, device=dev)
    spread = torch.zeros((n_nodes,), dtype=torch.float64, device=dev)
    if n_nodes:
        lib = L.lib()
        po_t, no_t = torch.from_numpy(piece_off).to(dev), torch.from_numpy(node_off).to(dev)
        nb = lib.prh_fuse_gather_workspace_bytes(n_p)
        ws = G.workspace(nb, dev)
        L.check(lib.prh_fuse_gather(G.ptr(world), G.ptr(s), n_p, m, G.ptr(po_t), n_l, G.ptr(no_t), n_nodes, float(step),
                                    G.ptr(X), G.ptr(W), G.ptr(C), G.ptr(spread), G.ptr(ws), nb, dev.index, G.stream(dev)),
                "prh_fuse_gather")
    return X, W, C, spread


def pieces_to_world(pieces, piece_pose, poses_xyzq, origin=None):
    """Step 1: pieces (P,M,3) in the ego frame of pose piece_pose[p] -> (P,M,3) float64 numpy in the
    drive frame, w = R(q) p + t in fp64 on the GPU (1 <= M <= 64).  The rotation runs on
    translations shifted by origin (default: default_origin(poses)), which is added back."""
    pc = _check_pieces(pieces, "pieces_to_world", lo=1)
    poses = _check_poses(poses_xyzq, "pieces_to_world")
    pp = _check_index(piece_pose, len(pc), len(poses), "piece_pose", "pieces_to_world")
    dev = G.device("fuse")
    org = _origin(origin, poses)
    if len(pc) == 0:
        return np.zeros(pc.shape)
    ps = poses.copy()
    ps[:, :3] -= org
    world, _, _, _ = _project(dev, pc, None, pp, ps, None, None)
    return world.cpu().numpy() + org


def project_to_lines(points, point_line, lines, origin=None):
    """Step 2: every point of points (N,3) projected onto the polyline lines[point_line[i]].
    Returns numpy (s (N,) arc position of the nearest point, d (N,) distance to it, seg (N,) int32
    the segment it lies on, -1 for a line without a segment of non-zero length, where s = 0 and d
    is the distance to the first vertex).  A line that points refer to needs at least one vertex.
    origin (default: the first vertex of the first line, rounded down to 1000 m) is subtracted
    from points and lines before the upload."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"project_to_lines: points must be (N,3), got {pts.shape}")
    pl = _check_index(point_line, len(pts), len(lines), "point_line", "project_to_lines")
    first = next((np.asarray(l, dtype=np.float64).reshape(-1, 3)[0] for l in lines if len(l)), np.zeros(3))
    org = floor_km(first) if origin is None else np.asarray(origin, dtype=np.float64).reshape(3)
    shifted, cums = _lines(lines, org)
    if any(len(shifted[l]) == 0 for l in np.unique(pl)):
        raise ValueError("project_to_lines: a line that points refer to has no vertex")
    dev = G.device("fuse")
    if len(pts) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int32)
    order = np.argsort(pl, kind="stable")
    _, s, d, seg = _project(dev, np.ascontiguousarray((pts - org)[order].reshape(-1, 1, 3)), pl[order], None, None,
                            shifted, cums)
    back = inverse_permutation(order)
    return s.cpu().numpy()[back, 0], d.cpu().numpy()[back, 0], seg.cpu().numpy()[back, 0]


def fuse_pieces(lines, pieces, piece_line, piece_pose, poses_xyzq, step=STEP, min_count=MIN_COUNT, max_gap=MAX_GAP,
                origin=None, return_nodes=False):
    """The refined pieces of a drive fused into one map (steps 1-6 of the rule).

    lines: list of (n,3) carrier polylines in the drive frame; pieces (P,M,3), 2 <= M <= 64, piece p
    in the ego frame of poses_xyzq[piece_pose[p]] and belonging to lines[piece_line[p]].  Pieces may
    come in any order: they are grouped by line with their order within a line kept.  Every node
    (one per step metres of a line's arc) is the taper-weighted mean of the piece segments that
    pass it.  Returns fused: per line the list of (k,3) float64 polylines made of its nodes with at
    least min_count contributions, cut at gaps longer than max_gap metres.  return_nodes=True also
    returns {'X' (N,3), 'W', 'C', 'spread' (N,), 'offsets' (n_lines+1,), 'world' (P,M,3), 's', 'd',
    'seg' (P,M), 'origin'}: the nodes line after line (X of an unused node is 0) and the pieces'
    drive-frame points and projections in the caller's piece order.  Bitwise reproducible."""
    pc = _check_pieces(pieces, "fuse_pieces")
    poses = _check_poses(poses_xyzq, "fuse_pieces")
    n_p, m = pc.shape[:2]
    pl = _check_index(piece_line, n_p, len(lines), "piece_line", "fuse_pieces")
    pp = _check_index(piece_pose, n_p, len(poses), "piece_pose", "fuse_pieces")
    if not float(step) > 0.0:
        raise ValueError("fuse_pieces: step must be positive")
    org = _origin(origin, poses)
    shifted, cums = _lines(lines, org)
    if any(len(shifted[l]) == 0 for l in np.unique(pl)):
        raise ValueError("fuse_pieces: a line that pieces refer to has no vertex")
    dev = G.device("fuse")
    n_l = len(lines)
    node_off = node_offsets(cums, step)
    order = np.argsort(pl, kind="stable")
    ps = poses.copy()
    ps[:, :3] -= org
    if n_p:
        world, s, d, seg = _project(dev, np.ascontiguousarray(pc[order]), pl[order], pp[order], ps, shifted, cums)
    else:
        world = torch.zeros((0, m, 3), dtype=torch.float64, device=dev)
        s, d, seg = world[:, :, 0], world[:, :, 0], world[:, :, 0].to(torch.int32)
    X, W, C, spread = gather_nodes(dev, world, s, G.csr_offsets(np.bincount(pl, minlength=n_l)[:n_l]), node_off, step)
    Xh, Ch = X.cpu().numpy(), C.cpu().numpy()
    Xh[Ch > 0] += org
    fused = [node_polylines(Xh[node_off[l]:node_off[l + 1]], Ch[node_off[l]:node_off[l + 1]], step, min_count, max_gap)
             for l in range(n_l)]
    if not return_nodes:
        return fused
    back = inverse_permutation(order)
    nodes = {"X": Xh, "W": W.cpu().numpy(), "C": Ch, "spread": spread.cpu().numpy(), "offsets": node_off, "origin": org,
             "world": world.cpu().numpy()[back] + org, "s": s.cpu().numpy()[back], "d": d.cpu().numpy()[back],
             "seg": seg.cpu().numpy()[back]}
    return fused, nodes


def map_error(fused, gt_lines):
    """How far a map is from its lines.  fused: per line a list of (k,3) polylines (fuse_pieces'
    result, or any polylines attributed to lines); gt_lines: the lines, same length.  Every vertex
    is projected onto its line with project_to_lines.  Returns {'mean', 'max': distance of the
    vertices in metres (nan without vertices), 'coverage': length of the union of the polylines' arc
    intervals [min s, max s] over the total length of the lines, 'vertices', 'covered_length',
    'line_length'}."""
    if len(fused) != len(gt_lines):
        raise ValueError("map_error: one list of polylines per line")
    parts = [(l, np.asarray(p, dtype=np.float64).reshape(-1, 3)) for l, ps in enumerate(fused) for p in ps]
    parts = [(l, p) for l, p in parts if len(p)]
    total = float(sum(carrier_cum(g)[-1] for g in gt_lines if len(g)))
    if not parts:
        G.device("fuse")
        return {"mean": float("nan"), "max": float("nan"), "coverage": 0.0, "vertices": 0, "covered_length": 0.0,
                "line_length": total}
    pts = np.concatenate([p for _, p in parts])
    pl = np.concatenate([np.full(len(p), l, dtype=np.int64) for l, p in parts])
    s, d, _ = project_to_lines(pts, pl, gt_lines)
    spans, at = {}, 0
    for l, p in parts:
        sp = s[at:at + len(p)]
        at += len(p)
        spans.setdefault(l, []).append((float(sp.min()), float(sp.max())))
    covered = 0.0
    for iv in spans.values():
        iv.sort()
        lo, hi = iv[0]
        for a, b in iv[1:]:
            if a > hi:
                covered += hi - lo
                lo, hi = a, b
            else:
                hi = max(hi, b)
        covered += hi - lo
    return {"mean": float(d.mean()), "max": float(d.max()), "coverage": covered / total if total > 0 else 0.0,
            "vertices": int(len(pts)), "covered_length": covered, "line_length": total}


def refine_slices(model, points, off, cands, num_line_points, num_context_points, crop_radius, decay_scale, seed,
                  precision, min_tube_points, batched=False):
    """The slice refinement of refine_drive and link.refine_predictions.  points (T,4) CUDA and off
    (S+1,) host offsets from drive.slice_cloud; cands: per slice the list of candidate polylines in
    that slice's frame.  One io.scene_offsets call per slice that has candidates and points, or,
    batched, one io.scene_offsets_ragged call over those slices: the same contexts byte for byte,
    other rows sharing a forward call.  Slice si draws with seed * 1000003 + si; the lines of a slice
    without points are counted as sparse and never reach the model; a piece whose tube held fewer
    than min_tube_points points is left out and counted.  Returns (pieces (P,M,3) float64 = noisy_c +
    centres + offset, piece_slice (P,), piece_row (P,) the row in cands[slice], both int64, sparse),
    pieces in slice order, then candidate order."""
    from .io import scene_offsets, scene_offsets_ragged
    off = np.asarray(off, dtype=np.int64)
    m = int(num_line_points)
    n_cand = np.array([len(c) for c in cands], dtype=np.int64)
    has_points = np.diff(off) > 0
    sparse = int(n_cand[~has_points].sum())
    used = np.flatnonzero(has_points & (n_cand > 0))
    if len(used) == 0:
        return np.zeros((0, m, 3)), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), sparse
    line_slice = np.repeat(used, n_cand[used])
    line_row = np.concatenate([np.arange(n_cand[si]) for si in used])
    seeds = [int(seed) * 1000003 + si for si in range(len(off) - 1)]
    kw = dict(precision=precision, return_counts=True)

    def to_host(offset, noisy_c, centres, counts):
        return (noisy_c + centres[:, None, :] + offset).to(torch.float64).cpu().numpy(), counts.cpu().numpy()

    if batched:
        parts = [to_host(*scene_offsets_ragged(model, points.to(torch.float32), off, [v for si in used for v in cands[si]],
                                               line_slice, seeds, m, num_context_points, crop_radius, decay_scale, **kw))]
    else:
        parts = [to_host(*scene_offsets(model, points[off[si]:off[si + 1]].to(torch.float32), cands[si], m,
                                        num_context_points, crop_radius, decay_scale, seed=seeds[si], **kw)) for si in used]
    refined = np.concatenate([r for r, _ in parts])
    keep = np.concatenate([c for _, c in parts]) >= int(min_tube_points)
    return refined[keep], line_slice[keep], line_row[keep], sparse + int((~keep).sum())


def refine_report(n_slices, pieces, sparse, nodes, fused, min_count):
    """What the 'report' of refine_drive and of link.refine_predictions have in common."""
    return {"slices": int(n_slices), "pieces": int(len(pieces)), "pieces_sparse": int(sparse),
            "nodes": int(len(nodes["C"])), "nodes_used": int((nodes["C"] >= min_count).sum()),
            "fused_polylines": int(sum(len(f) for f in fused))}


@torch.no_grad()
def refine_drive(model, drive_dir_or_cloud, poses, lines, num_line_points=32, num_context_points=1024, crop_radius=0.3,
                 decay_scale=2.0, seed=0, precision=None, segment_len=None, stride=None, radius=None, max_pose_gap=None,
                 step=STEP, min_count=MIN_COUNT, max_gap=MAX_GAP, min_tube_points=MIN_TUBE_POINTS, origin=None,
                 batched=False, support=False, support_radius=None, intensity_floor=0.0):
    """Refine the lines of a whole drive into one drive-frame map.

    drive_dir_or_cloud: a drive directory (merged.pcd and, when poses is None, pose/*.json) or the
    merged cloud itself, (P,4) float32 xyz + intensity (numpy or CUDA tensor).  poses: load_poses'
    list, an (S,7) array of x y z qx qy qz qw in file-name order, or None.  lines: list of (n,3)
    polylines in the drive frame (GT with noise, detector output matched to a carrier, ...).

    A chain of the project's calls: drive.plan_slices picks the slice poses; drive.slice_cloud cuts
    every slice's points; drive.clip_lines cuts the lines per slice; refine_slices runs the model,
    one io.scene_offsets call per slice, on the points taken straight from slice_cloud on the device - the
    points are rounded to float32 once, there is no PCD text round trip, so they are not rounded to
    the file format's 4 decimals the way a drive written by slice_drive and read back is; the
    refined pieces noisy_c + centres + offset are collected with their line and slice; fuse_pieces
    merges them with the input lines as carriers.  A piece whose tube held fewer than
    min_tube_points cloud points is left out and counted (the model saw padding, not a lane).
    batched=True makes that one io.scene_offsets_ragged call over all slices: the same contexts
    byte for byte, the same pieces in the same order up to which rows share a forward call.
    support=True scores the input lines and the fused map against the cloud (support.map_support
    with tube radius support_radius, default crop_radius, and intensity_floor): the lateral offset
    of the paint before and after refinement, with no GT.  intensity_floor may be "auto":
    paintfloor.paint_floor reads it from the slices, once, as soon as they are cut, and the report
    gains 'floor', 'floor_surface_points', 'floor_paint_share' and 'floor_contrast'.

    Returns {'fused', 'pieces' (P,M,3) float64 ego frame, 'piece_line', 'piece_slice' (P,),
    'pose_index' (plan_slices), 'poses' (S,7) of the slices, 'nodes' (fuse_pieces' node dict),
    'report': {'slices', 'pieces', 'pieces_sparse' (left out), 'nodes', 'nodes_used', 'fused_polylines'}}
    and, with support=True, 'support': {'input', 'fused' (map_support's dicts), 'attributes'
    (support.marking_attributes of the fused map, per line)}."""
    from . import drive as D
    from . import paintfloor as PF
    G.device("fuse")
    if not 2 <= int(num_line_points) <= MAX_POINTS:
        raise ValueError(f"refine_drive: 2..{MAX_POINTS} points per line, got {num_line_points}")
    kw = {k: v for k, v in (("segment_len", segment_len), ("stride", stride), ("max_pose_gap", max_pose_gap)) if v is not None}
    segment_len = D.SEGMENT_LEN if segment_len is None else segment_len
    if isinstance(drive_dir_or_cloud, (str, os.PathLike)):
        if poses is None:
            poses = D.load_poses(os.path.join(drive_dir_or_cloud, "pose"))
        cloud = D.load_merged_cloud(drive_dir_or_cloud).astype(np.float32, copy=False)
    else:
        cloud = drive_dir_or_cloud
    if poses is None:
        raise ValueError("refine_drive: poses are needed with a cloud")
    chosen = D.plan_slices(poses, **kw)
    if len(poses) and isinstance(poses[0], dict):
        pq = D.poses_xyzq(poses, chosen)
    else:
        pq = np.asarray(poses, dtype=np.float64).reshape(-1, 7)[chosen].reshape(-1, 7)
    lines = [np.asarray(l, dtype=np.float64).reshape(-1, 3) for l in lines]
    points, off, clipped = None, np.zeros(1, dtype=np.int64), []        # without a slice or a line: nothing to refine
    if len(chosen) and len(lines):
        points, offsets, _ = D.slice_cloud(cloud, pq, segment_len, D.RADIUS if radius is None else radius)
        clipped = D.clip_lines(lines, pq, segment_len)
        off = offsets.cpu().numpy()
    intensity_floor, floor_report = PF.resolve(intensity_floor, points, off, "refine_drive")      # "auto" without a slice raises
    pieces, piece_slice, row, sparse = refine_slices(
        model, points, off, [[v for _, v in kept] for kept in clipped], num_line_points,
        num_context_points, crop_radius, decay_scale, seed, precision, min_tube_points, batched)
    first = G.csr_offsets([len(kept) for kept in clipped])
    piece_line = np.array([l for kept in clipped for l, _ in kept], dtype=np.int64)[first[piece_slice] + row]
    fused, nodes = fuse_pieces(lines, pieces, piece_line, piece_slice, pq, step, min_count, max_gap, origin,
                               return_nodes=True)
    res = {"fused": fused, "pieces": pieces, "piece_line": piece_line, "piece_slice": piece_slice, "pose_index": chosen,
           "poses": pq, "nodes": nodes, "report": refine_report(len(chosen), pieces, sparse, nodes, fused, min_count)}
    if floor_report is not None:
        res["report"].update(PF.report_keys(floor_report))
    if support:
        res["support"] = cloud_support(cloud, fused, lines, step, crop_radius if support_radius is None else support_radius,
                                       intensity_floor, nodes["origin"])
    return res


def cloud_support(cloud, fused, lines, step, radius, intensity_floor, origin):
    """refine_drive's and link.refine_predictions' 'support' entry: the cloud goes to the device
    once and is read once per map.  lines None: no input map to score."""
    from . import support as S
    cloud_t = S._cloud(cloud, G.device("support"), "cloud_support")
    kw = dict(step=step, radius=radius, intensity_floor=intensity_floor, origin=origin, per_line=True)
    out = {} if lines is None else {"input": S.map_support(cloud_t, lines, **kw)}
    out["fused"] = S.map_support(cloud_t, fused, **kw)
    out["attributes"] = S.marking_attributes(out["fused"])
    return out
