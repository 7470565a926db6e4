"""Prediction scenes: the reference's tools/generate_inference_data_vma.py - the lane detector's
per-frame BEV-pixel polylines, the drive's poses, merged cloud and GT polylines in; one ego-frame
scene per camera frame out, each prediction paired with the GT line a global (Hungarian) assignment
gives it.  These are the files ``io.load_scene_items`` -> ``metrics.evaluate_scene`` read.  The
reference loops over frames in Python (a numpy pass over the cloud, one numpy call per
(prediction, GT) pair, scipy per frame); here every frame of a drive goes through one
``drive.slice_cloud``, one clip, one cost and one assignment launch (``csrc/prh_match.hpp``).

  pixel_to_ego / load_results / load_frame_poses / match_poses   host: the detector JSON, the poses
                                                  and the nearest-pose rule (:101-124,248-262,338-359)
  clip_lines_frames      HIP: GT polylines per frame, this tool's clip rule (:265-315,400-402),
                         through the driver drive.clip_lines uses (_gpu.clip_two_pass)
  line_costs             HIP: the (P_f, G_f) one-way xy Chamfer matrices of all frames (:434-448)
  assign                 HIP: minimum-cost assignment of every frame's matrix (:451-459)
  match_predictions      line_costs + assign
  write_prediction_scene / predictions_to_scenes   host: the tool's two files (:151-175) and main()

clip_lines_frames, line_costs, assign, match_predictions and predictions_to_scenes have no CPU
fallback: without a GPU they raise RuntimeError.
"""
import glob
import json
import os

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L
from . import drive as D
from .pcd import write_pcd_host, write_pcds

SEGMENT_LEN = 50.0               # generate_inference_data_vma.py:18
RADIUS = 60.0                    # :366
MAX_POSE_GAP_NS = 250_000_000    # :357
MATCH_THRESHOLD = 15.0           # :454
BEV_RES = 0.05                   # :177
BEV_HALF = 25.0                  # :248-255
MAX_LINES = 128                  # lines per side per frame assign() takes (MT_MAX_SIDE of csrc/prh_match.hpp)
STATUS_OK, STATUS_INVALID, STATUS_TOO_LARGE = 0, 1, 2


# ------------------------------------------------------------------ host side
def pixel_to_ego(pixels, res=BEV_RES, half=BEV_HALF):
    """(n,2) BEV pixels (u, v) -> (n,3) float64 ego x = half - v*res, y = half - u*res, z = 0 (:248-262)."""
    px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((len(px), 3), dtype=np.float64)
    out[:, 0] = half - px[:, 1] * res
    out[:, 1] = half - px[:, 0] * res
    return out


def load_results(json_path):
    """The detector's JSON (:330-346,412-422): list of {'ts' int, 'key', 'pixels' [(n,2) float64],
    'scores' [..]} sorted by timestamp.  A key whose basename up to '.jpg' is not an integer is
    ignored; an instance with fewer than two vertices is dropped; a missing score is 0.0."""
    with open(json_path, "r") as f:
        data = json.load(f)
    by_ts = {}
    for k in data.keys():
        try:
            by_ts[int(os.path.basename(k).split(".jpg")[0])] = k
        except Exception:
            pass
    frames = []
    for ts in sorted(by_ts):
        pixels, scores = [], []
        for inst in data[by_ts[ts]].get("pred_instances", []):
            if len(inst["data"]) > 1:
                pixels.append(np.asarray(inst["data"], dtype=np.float64).reshape(-1, 2))
                scores.append(inst.get("score", 0.0))
        frames.append({"ts": ts, "key": by_ts[ts], "pixels": pixels, "scores": scores})
    return frames


def load_frame_poses(pose_dir):
    """This tool's load_poses (:101-124): list of {'ts' int, 'x', 'y', 'z', 'q': [qx,qy,qz,qw]} sorted by
    the integer timestamp, which is the file name when that parses and the file's 'ts' otherwise."""
    poses = []
    for f in glob.glob(os.path.join(pose_dir, "*.json")):
        with open(f, "r") as fp:
            data = json.load(fp)
        try:
            ts = int(os.path.splitext(os.path.basename(f))[0])
        except (ValueError, TypeError):
            ts = int(data["ts"])
        poses.append({"ts": ts, "x": data["x"], "y": data["y"], "z": data["z"],
                      "q": [data["qx"], data["qy"], data["qz"], data["qw"]]})
    poses.sort(key=lambda p: p["ts"])
    return poses


def match_poses(result_ts, pose_ts, max_gap=MAX_POSE_GAP_NS):
    """Index of the pose nearest in time to every result timestamp (:353-359), the first one on a
    tie, -1 when the gap is > max_gap (or there is no pose).  Python integers throughout:
    nanosecond timestamps exceed 2^53."""
    pose_ts = [int(t) for t in pose_ts]
    out = np.full(len(result_ts), -1, dtype=np.int64)
    if not pose_ts:
        return out
    for n, ts in enumerate(result_ts):
        ts = int(ts)
        j = min(range(len(pose_ts)), key=lambda k: abs(pose_ts[k] - ts))
        if not abs(pose_ts[j] - ts) > max_gap:
            out[n] = j
    return out


def write_prediction_scene(pcd_path, json_path, points, items, pose_ts, result_ts):
    """The tool's scene files (save_pcd :151-166, save_json_vma_direct :168-175), byte for byte: the
    ASCII PCD drive.write_scene writes, and a JSON of timestamp (the pose's), result_timestamp and
    the items as given (dicts of 'category', 'attributes', 'position', 'noisy_candidates',
    'context_lines' with lists of {'x','y','z'}), indent 4."""
    write_pcd_host(pcd_path, points)
    _write_prediction_json(json_path, items, pose_ts, result_ts)


def _write_prediction_json(json_path, items, pose_ts, result_ts):
    """write_prediction_scene's JSON file (predictions_to_scenes writes the .pcd files through pcd.write_pcds)."""
    with open(json_path, "w") as f:
        json.dump({"timestamp": str(pose_ts), "result_timestamp": str(result_ts), "items": items}, f, indent=4)


# ------------------------------------------------------------------ GPU side
def _check_unit(poses, what):
    p = poses.detach().cpu().numpy() if torch.is_tensor(poses) else np.asarray(poses, dtype=np.float64)
    p = p.reshape(-1, 7)
    bad = np.flatnonzero(~(np.abs(np.sqrt((p[:, 3:] ** 2).sum(1)) - 1.0) <= 1e-6))
    if len(bad):
        raise ValueError(f"{what}: pose {int(bad[0])} has a quaternion of norm "
                         f"{float(np.sqrt((p[bad[0], 3:] ** 2).sum())):.9g}; this tool's frame is only a rotation "
                         "for unit quaternions")


def clip_lines_frames(lines, poses_xyzq, segment_len=SEGMENT_LEN, return_counts=False):
    """Every polyline of lines (list of (n,3)) in the ego frame of every pose, by this tool's rule
    (:400-402, 265-315), which is not drive.clip_lines' rule: a line counts only if some vertex has
    -segment_len/2 < x < segment_len/2 strictly; it is cut by the two half-plane passes of
    clip_polygon_against_plane (no de-duplication; an edge with |dx| < 1e-6 gives its first vertex
    as the intersection) and kept when more than one vertex remains.  Returns, per frame, the list
    of (line index, (k,3) float64) kept, in line order; return_counts=True also returns the (F,
    n_lines) int array of vertex counts before the keep rule (0 for a line the gate drops).
    Poses whose quaternion norm differs from 1 by more than 1e-6 raise ValueError."""
    dev = G.device("predictions")
    _check_unit(poses_xyzq, "clip_lines_frames")
    ps = G.poses(poses_xyzq, dev, "clip_lines_frames")
    return G.clip_two_pass(("prh_match_clip_workspace_bytes", "prh_match_clip_count", "prh_match_clip_write"), lines, ps,
                           segment_len, return_counts)


def _xy_csr(lines, dev):
    arrs = [np.asarray(l, dtype=np.float64) for l in lines]
    arrs = [a.reshape(-1, a.shape[-1] if a.ndim == 2 and a.shape[-1] in (2, 3) else 3)[:, :2] for a in arrs]
    off = G.csr_offsets([len(a) for a in arrs])
    xy = np.concatenate(arrs) if off[-1] > 0 else np.zeros((0, 2))
    return torch.from_numpy(np.ascontiguousarray(xy, dtype=np.float64)).to(dev), torch.from_numpy(off).to(dev)


def _frame_offsets(offsets, n_lines, what):
    off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    if len(off) < 1 or off[0] != 0 or off[-1] != n_lines or np.any(np.diff(off) < 0):
        raise ValueError(f"{what}: frame offsets must rise from 0 to the number of lines ({n_lines})")
    return off


def line_costs(pred_lines, pred_offsets, gt_lines, gt_offsets):
    """The cost matrices of every frame in one launch sequence (:434-448): frame f owns prediction
    lines pred_lines[pred_offsets[f]:pred_offsets[f+1]] and GT lines gt_lines[gt_offsets[f]:
    gt_offsets[f+1]] (lists of (n,3) or (n,2) arrays, only x and y are read), and
    cost[i,j] = mean_p min_g |pred_i[p].xy - gt_j[g].xy|.  Returns (costs flat float64 CUDA,
    cost_offsets (F+1,) int64 numpy, shapes (F,2) int numpy): frame f's matrix is
    costs[cost_offsets[f]:cost_offsets[f+1]].reshape(shapes[f]); a frame with P_f = 0 or G_f = 0 has
    an empty one.  Fixed reduction order, no atomics: bitwise reproducible."""
    return _costs_packed(_pack_lines(pred_lines, pred_offsets, gt_lines, gt_offsets))


def _pack_lines(pred_lines, pred_offsets, gt_lines, gt_offsets):
    """line_costs' arguments as device CSR arrays (the host half of the call)."""
    dev = G.device("predictions")
    p_off = _frame_offsets(pred_offsets, len(pred_lines), "line_costs")
    g_off = _frame_offsets(gt_offsets, len(gt_lines), "line_costs")
    if len(p_off) != len(g_off):
        raise ValueError("line_costs: prediction and GT offsets must describe the same frames")
    n_f = len(p_off) - 1
    shapes = np.stack([np.diff(p_off), np.diff(g_off)], 1).astype(np.int64).reshape(n_f, 2)
    c_off = G.csr_offsets(shapes[:, 0] * shapes[:, 1])
    pxy, pl_off = _xy_csr(pred_lines, dev)
    gxy, gl_off = _xy_csr(gt_lines, dev)
    pf, gf, cf = (torch.from_numpy(a).to(dev) for a in (p_off, g_off, c_off))
    return dev, len(pred_lines), n_f, (pxy, pl_off, pf), (gxy, gl_off, gf), cf, c_off, shapes.astype(np.int32)


def _costs_packed(packed):
    dev, n_pred, n_f, (pxy, pl_off, pf), (gxy, gl_off, gf), cf, c_off, shapes = packed
    costs = torch.empty((int(c_off[-1]),), dtype=torch.float64, device=dev)
    if c_off[-1] > 0:
        lib = L.lib()
        nb = lib.prh_match_costs_workspace_bytes(n_pred)
        ws = G.workspace(nb, dev)
        L.check(lib.prh_match_costs(G.ptr(pxy), G.ptr(pl_off), G.ptr(pf), n_pred, G.ptr(gxy), G.ptr(gl_off), G.ptr(gf), n_f,
                                    G.ptr(cf), G.ptr(costs), G.ptr(ws), nb, dev.index, G.stream(dev)), "prh_match_costs")
    return costs, c_off, shapes


def assign(costs, cost_offsets, shapes, threshold=None, return_duals=False):
    """Minimum-cost assignment of every frame's (P_f, G_f) matrix, min(P_f, G_f) pairs per frame, all
    frames in one launch (one wave per frame, shortest augmenting paths with potentials).  costs:
    flat float64 (CUDA tensor or numpy), frame f at cost_offsets[f], row major, shapes (F,2).
    Returns (match (sum P_f,) int32 numpy: the GT column of each prediction row or -1, total (F,)
    float64 numpy: the optimal sum).  With threshold, pairs whose cost is not < threshold become -1
    (:454-459); total is the sum before that.  return_duals=True adds (u (sum P_f,), v (sum G_f,)):
    the row / column potentials the solver ended with, cost[i,j] - u[i] - v[j] >= 0 up to rounding
    and = 0 on assigned pairs.  When several assignments are optimal any one of them may be
    returned; the same input gives the same bits every run.  At most MAX_LINES (128) lines per side
    per frame: more raise ValueError, and so does a frame with a NaN or infinite cost."""
    dev = G.device("predictions")
    shapes = np.ascontiguousarray(shapes, dtype=np.int32).reshape(-1, 2)
    n_f = len(shapes)
    c_off = np.ascontiguousarray(cost_offsets, dtype=np.int64).reshape(-1)
    cells = shapes[:, 0].astype(np.int64) * shapes[:, 1]
    if len(c_off) != n_f + 1 or np.any(shapes < 0) or np.any(np.diff(c_off) != cells):
        raise ValueError("assign: cost_offsets must have one entry per frame plus one and steps of P_f * G_f")
    if n_f and shapes.max() > MAX_LINES:
        f = int(np.argmax(shapes.max(1)))
        raise ValueError(f"assign: frame {f} is {shapes[f, 0]} x {shapes[f, 1]}; at most {MAX_LINES} lines per side")
    ct = G.as_cuda(costs, dev, "assign", torch.float64).reshape(-1)
    if ct.numel() != (int(c_off[-1]) if n_f else 0):
        raise ValueError(f"assign: {ct.numel()} costs for offsets that end at {int(c_off[-1]) if n_f else 0}")
    r_off = G.csr_offsets(shapes[:, 0])
    g_off = G.csr_offsets(shapes[:, 1])
    match = torch.full((int(r_off[-1]),), -1, dtype=torch.int32, device=dev)
    total = torch.zeros((n_f,), dtype=torch.float64, device=dev)
    status = torch.zeros((n_f,), dtype=torch.int32, device=dev)
    u = torch.zeros((int(r_off[-1]),), dtype=torch.float64, device=dev) if return_duals else None
    v = torch.zeros((int(g_off[-1]),), dtype=torch.float64, device=dev) if return_duals else None
    if n_f:
        cf, rf, gf = (torch.from_numpy(a).to(dev) for a in (c_off, r_off, g_off))
        sh = torch.from_numpy(shapes).to(dev)
        L.check(L.lib().prh_match_assign(G.ptr(ct), G.ptr(cf), G.ptr(sh), G.ptr(rf), G.ptr(gf), n_f, int(cells.max()),
                                         float(threshold) if threshold is not None else 0.0,
                                         1 if threshold is not None else 0, G.ptr(match), G.ptr(total), G.ptr(status),
                                         G.ptr(u), G.ptr(v), dev.index, G.stream(dev)), "prh_match_assign")
    st = status.cpu().numpy()
    if np.any(st != STATUS_OK):
        f = int(np.flatnonzero(st != STATUS_OK)[0])
        why = "a NaN or infinite cost" if st[f] == STATUS_INVALID else f"more than {MAX_LINES} lines per side"
        raise ValueError(f"assign: frame {f} ({shapes[f, 0]} x {shapes[f, 1]}) has {why}")
    res = (match.cpu().numpy(), total.cpu().numpy())
    return res + (u.cpu().numpy(), v.cpu().numpy()) if return_duals else res


def match_predictions(pred_lines_per_frame, gt_lines_per_frame, threshold=MATCH_THRESHOLD):
    """line_costs + assign for lists (per frame) of lists of polylines (:426-459).  Returns a list per
    frame of (match (P_f,) int32: GT index of each prediction or -1, cost (P_f, G_f) float64)."""
    if len(pred_lines_per_frame) != len(gt_lines_per_frame):
        raise ValueError("match_predictions: one list of predictions and one of GT lines per frame")
    G.device("predictions")
    p_off = G.csr_offsets([len(p) for p in pred_lines_per_frame])
    g_off = G.csr_offsets([len(g) for g in gt_lines_per_frame])
    costs, c_off, shapes = line_costs([l for p in pred_lines_per_frame for l in p], p_off,
                                      [l for g in gt_lines_per_frame for l in g], g_off)
    match, _ = assign(costs, c_off, shapes, threshold=threshold)
    costs = costs.cpu().numpy()
    return [(match[p_off[f]:p_off[f + 1]].copy(), costs[c_off[f]:c_off[f + 1]].reshape(shapes[f]).copy())
            for f in range(len(shapes))]


def predictions_to_scenes(drive_dir, gt_json, results_json, out_dir=None, segment_len=SEGMENT_LEN, radius=RADIUS,
                          max_pose_gap=MAX_POSE_GAP_NS, threshold=MATCH_THRESHOLD, verbose=True, lift=False,
                          align=False, align_max_yaw=0.0):
    """The tool's main() (:317-490) for one drive: drive_dir holds pose/*.json and merged.pcd, gt_json
    the GT polylines, results_json the detector's output.  One slice_cloud, one clip_lines_frames and
    one match_predictions call serve every frame that found a pose.  A frame is skipped when no pose
    lies within max_pose_gap, when its slice keeps no point or when it has no prediction.  Per
    prediction one item: category 'lane_line', attributes {'score'}, position = the matched clipped
    GT or [], noisy_candidates = [the prediction], context_lines = every clipped GT of the frame.
    With out_dir, TS.pcd / TS.json (TS = the result timestamp) are written for the frames kept.
    lift=True gives the noisy_candidates the z of the road under them (ground.lift_lines over the
    frames' slices, its defaults) instead of the detector's z = 0, and adds 'lift': lift_lines'
    report; matching stays on xy and is unchanged.
    align=True moves the x y of the noisy_candidates onto the paint (align.align_lines over the
    frames' slices, its defaults, after the lift) and adds 'align': align_lines' report; the matches,
    positions, context lines and PCD bytes are those of the detector's own lines.  align_max_yaw
    above 0 sweeps a yaw of up to that many radians about each frame's ego origin with the shift
    (align.align_lines_rigid, its other defaults): the report then has 'yaws' as well.
    Returns {'frames' [result ts], 'pose_index' (per frame, -1: none), 'pose_ts', 'points' (T,4) CUDA
    and 'offsets' over the frames with a pose (row 'slice' of each frame, -1: none), 'slice',
    'items' [per frame list of item dicts, [] for a skipped frame], 'matches', 'costs', 'gt_index'
    [per frame the GT item of each context line], 'written' [result ts]}."""
    G.device("predictions")
    poses = load_frame_poses(os.path.join(drive_dir, "pose"))
    res = {"frames": [], "pose_index": [], "pose_ts": [], "points": None, "offsets": None, "slice": [], "items": [],
           "matches": [], "costs": [], "gt_index": [], "written": []}
    if not poses:
        if verbose:
            print("No poses found.")
        return res
    cloud = D.load_merged_cloud(drive_dir)
    gt_items = D.load_gt_items(gt_json)
    frames = load_results(results_json)
    chosen = match_poses([fr["ts"] for fr in frames], [p["ts"] for p in poses], max_pose_gap)
    with_pose = np.flatnonzero(chosen >= 0)
    pq = D.poses_xyzq(poses, chosen[with_pose])
    points, offsets, _ = D.slice_cloud(np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4), pq, segment_len,
                                       radius)
    clipped = clip_lines_frames([it["points"] for it in gt_items], pq, segment_len)
    preds = [[pixel_to_ego(px) for px in frames[n]["pixels"]] for n in with_pose]
    matched = match_predictions(preds, [[v for _, v in c] for c in clipped], threshold)
    if lift:
        from .ground import lift_lines
        preds, res["lift"] = lift_lines(points, offsets, preds)
    if align:
        from .align import align as align_on_paint
        preds, res["align"] = align_on_paint(points, offsets, preds, align_max_yaw)
    off = offsets.cpu().numpy()
    pcd_paths = [None] * (len(off) - 1)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    slot = {int(n): s for s, n in enumerate(with_pose)}
    for n, fr in enumerate(frames):
        s = slot.get(n, -1)
        res["frames"].append(fr["ts"])
        res["pose_index"].append(int(chosen[n]))
        res["pose_ts"].append(poses[chosen[n]]["ts"] if s >= 0 else None)
        res["slice"].append(s)
        items = []
        if s >= 0 and off[s + 1] > off[s]:
            context = [D.xyz_dicts(v) for _, v in clipped[s]]
            for i, line in enumerate(preds[s]):
                g = int(matched[s][0][i])
                items.append({"category": "lane_line", "attributes": {"score": fr["scores"][i]},
                              "position": context[g] if g >= 0 else [], "noisy_candidates": [D.xyz_dicts(line)],
                              "context_lines": context})
        res["items"].append(items)
        res["matches"].append(matched[s][0] if s >= 0 else np.zeros(0, dtype=np.int32))
        res["costs"].append(matched[s][1] if s >= 0 else np.zeros((0, 0)))
        res["gt_index"].append([l for l, _ in clipped[s]] if s >= 0 else [])
        if s < 0:
            if verbose:
                print(f"  Skipping {fr['ts']}: no pose within {max_pose_gap / 1e6:.1f}ms")
        elif not items:
            if verbose:
                print(f"  Skipping {fr['ts']}: " + ("no point in the slice" if off[s + 1] == off[s] else
                                                    "No predictions found in JSON."))
        elif out_dir is not None:
            pcd_paths[s] = os.path.join(out_dir, f"{fr['ts']}.pcd")
            _write_prediction_json(os.path.join(out_dir, f"{fr['ts']}.json"), items, poses[chosen[n]]["ts"], fr["ts"])
            res["written"].append(fr["ts"])
    if out_dir is not None:
        write_pcds(pcd_paths, points, off)              # the text of every frame's slice from one device pass
    res.update(points=points, offsets=offsets)
    if verbose:
        kept = len(res["written"]) if out_dir is not None else sum(1 for it in res["items"] if it)
        print(f"Done. Generated {kept} samples" + (f" in {out_dir}" if out_dir is not None else ""))
    return res
