"""Scene evaluation on the GPU: the metric half of the reference's whole-scene script
(inference_whole_scene.py:26-92,170-193,299-387), whose scipy KDTree helpers run one line at a
time on the host.  fp64 HIP kernels (``csrc/prh_metrics.hpp``) compute, for every (item,
candidate) line of a scene at once:

  line_metrics         crop_gt_to_pred_range + resample_polyline + ADE + compute_chamfer_distance
                       for the noisy and the refined line (valid / bad_match as at :310,337-365)
  shift_sweep          mean_p min_g |pred_p + (dx,dy,0) - gt_g| for many shifts in one launch
  calibrate_alignment  the reference's coarse / fine (dx, dy) search on top of shift_sweep
  evaluate_scene       refine_scene's contexts and forward + the above, per scene

    items = io.load_scene_items(json_path)
    res = evaluate_scene(model, io.load_pcd_data(pcd_path), items)
    res["ade_noisy"], res["ade_refined"], res["calibration"]       # per-row arrays, ((dx,dy), dist)

There is no CPU fallback: without a GPU every function raises RuntimeError.
"""
import numpy as np
import torch

from . import _gpu as G
from . import _lib as L

BAD_MATCH_LAT = 1.0          # :341: a candidate whose initial Lat exceeds 1 m is matched to the wrong GT
_METRICS = ("ade_noisy", "ade_refined", "cd_noisy", "cd_refined", "lat_noisy", "lat_refined")


def line_metrics(noisy, refined, gt_lines, gt_index=None):
    """Per-line metrics of inference_whole_scene.py:337-365.

    noisy, refined: (L,M,3) float64 numpy arrays or CUDA tensors (M = 2..128), noisy being the
    resampled line the GT is cropped to.  gt_lines: list of (n,3) polylines (None or fewer than 2
    vertices = no usable GT).  gt_index: (L,) polyline of each line, -1 for none (default: line i
    uses gt_lines[i]).  Returns a dict of numpy arrays: crop_start, crop_end (inclusive indices
    into the GT polyline, -1 when not valid), reversed, valid, resampled_gt (L,M,3), ade_noisy,
    ade_refined, cd_noisy, cd_refined, lat_noisy, lat_refined (NaN when not valid) and
    bad_match = valid & (lat_noisy > 1.0)."""
    dev = G.device("metrics")
    nz = G.as_cuda(noisy, dev, "line_metrics", torch.float64)
    rf = G.as_cuda(refined, dev, "line_metrics", torch.float64)
    if nz.dim() != 3 or nz.shape[2] != 3 or rf.shape != nz.shape:
        raise ValueError(f"line_metrics: noisy and refined must both be (L,M,3), got {tuple(nz.shape)} and {tuple(rf.shape)}")
    n_lines, m = nz.shape[0], nz.shape[1]
    if not 2 <= m <= 128:
        raise ValueError(f"line_metrics: M must be 2..128, got {m}")
    gts = [np.zeros((0, 3)) if g is None else np.asarray(g, dtype=np.float64).reshape(-1, 3) for g in gt_lines]
    if gt_index is None:
        if len(gts) != n_lines:
            raise ValueError("line_metrics: without gt_index, gt_lines needs one polyline per line")
        gt_index = np.arange(n_lines)
    gt_index = np.asarray(gt_index, dtype=np.int64).reshape(-1)
    if len(gt_index) != n_lines or (n_lines and (gt_index.min() < -1 or gt_index.max() >= len(gts))):
        raise ValueError("line_metrics: gt_index must hold one index in [-1, len(gt_lines)) per line")
    offsets = np.zeros(len(gts) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(g) for g in gts])
    verts = np.concatenate(gts) if offsets[-1] > 0 else np.zeros((1, 3))      # never an empty buffer
    gt_t = torch.from_numpy(np.ascontiguousarray(verts)).to(dev)
    off_t = torch.from_numpy(offsets).to(dev)
    idx_t = torch.from_numpy(gt_index.astype(np.int32)).to(dev)
    info = torch.empty((n_lines, 4), dtype=torch.int32, device=dev)
    res = torch.empty((n_lines, m, 3), dtype=torch.float64, device=dev)
    met = torch.empty((n_lines, 6), dtype=torch.float64, device=dev)
    lib = L.lib()
    L.check(lib.prh_line_metrics(G.ptr(nz), G.ptr(rf), n_lines, m, G.ptr(gt_t), G.ptr(off_t), len(gts), G.ptr(idx_t),
                                 G.ptr(info), G.ptr(res), G.ptr(met), dev.index, G.stream(dev)), "prh_line_metrics")
    info, met = info.cpu().numpy(), met.cpu().numpy()
    out = {"crop_start": info[:, 0].astype(np.int64), "crop_end": info[:, 1].astype(np.int64),
           "reversed": info[:, 2].astype(bool), "valid": info[:, 3].astype(bool), "resampled_gt": res.cpu().numpy()}
    for k, name in enumerate(_METRICS):
        out[name] = met[:, k].copy()
    out["bad_match"] = out["valid"] & (np.nan_to_num(out["lat_noisy"], nan=0.0) > BAD_MATCH_LAT)
    return out


def _sweep(pred_t, gt_t, shifts, dev):
    sh = torch.from_numpy(np.ascontiguousarray(shifts, dtype=np.float64).reshape(-1, 2)).to(dev)
    n_s = sh.shape[0]
    out = torch.empty((n_s,), dtype=torch.float64, device=dev)
    lib = L.lib()
    nb = lib.prh_shift_sweep_workspace_bytes(pred_t.shape[0], gt_t.shape[0], n_s)
    ws = G.workspace(nb, dev)
    L.check(lib.prh_shift_sweep(G.ptr(pred_t), pred_t.shape[0], G.ptr(gt_t), gt_t.shape[0], G.ptr(sh), n_s, G.ptr(out),
                                G.ptr(ws), nb, dev.index, G.stream(dev)), "prh_shift_sweep")
    return out.cpu().numpy()


def shift_sweep(pred_points, gt_points, shifts):
    """(S,) float64: for every shift (dx, dy) of shifts (S,2), the mean over pred_points (P,3) of the
    distance from pred + (dx, dy, 0) to the nearest of gt_points (G,3) - calibrate_alignment's
    inner loop (:170-193) for all shifts in one launch.  Bitwise reproducible."""
    dev = G.device("metrics")
    pred_t = G.as_cuda(pred_points, dev, "shift_sweep", torch.float64).reshape(-1, 3)
    gt_t = G.as_cuda(gt_points, dev, "shift_sweep", torch.float64).reshape(-1, 3)
    if pred_t.shape[0] == 0 or gt_t.shape[0] == 0 or np.asarray(shifts).size == 0:
        raise ValueError("shift_sweep: needs at least one pred point, one GT point and one shift")
    return _sweep(pred_t, gt_t, shifts, dev)


def _grid(xs, ys):
    return np.array([(dx, dy) for dx in xs for dy in ys], dtype=np.float64).reshape(-1, 2)    # x outer, y inner


def calibrate_alignment(pred_lines, gt_lines, return_tables=False):
    """inference_whole_scene.py:148-193: brute-force (dx, dy) shift of the stacked pred_lines that
    minimises the mean distance to the nearest vertex of the stacked gt_lines.  Returns
    ((dx, dy), best_dist), ((0, 0), 999.0) when either list is empty.  The 400 coarse and the
    fine shifts (same np.arange grids, same strict-< choice in the same order) each run as one
    shift_sweep launch.  return_tables=True also returns {"coarse": (shifts, means), "fine": ...}."""
    if len(pred_lines) == 0 or len(gt_lines) == 0:
        return ((0, 0), 999.0, {}) if return_tables else ((0, 0), 999.0)
    dev = G.device("metrics")
    pred_t = G.as_cuda(np.vstack(pred_lines), dev, "calibrate_alignment", torch.float64)
    gt_t = G.as_cuda(np.vstack(gt_lines), dev, "calibrate_alignment", torch.float64)
    best_offset, best_dist = (0, 0), float("inf")
    tables = {}
    coarse = _grid(np.arange(-20, 20, 2.0), np.arange(-10, 10, 1.0))
    means = _sweep(pred_t, gt_t, coarse, dev)
    for (dx, dy), d in zip(coarse, means):
        if d < best_dist:
            best_dist, best_offset = d, (dx, dy)
    tables["coarse"] = (coarse, means)
    best_x, best_y = best_offset
    fine = _grid(np.arange(best_x - 2.0, best_x + 2.0, 0.2), np.arange(best_y - 1.0, best_y + 1.0, 0.2))
    means = _sweep(pred_t, gt_t, fine, dev)
    for (dx, dy), d in zip(fine, means):
        if d < best_dist:
            best_dist, best_offset = d, (dx, dy)
    tables["fine"] = (fine, means)
    best_offset = (np.float64(best_offset[0]), np.float64(best_offset[1]))
    return (best_offset, np.float64(best_dist), tables) if return_tables else (best_offset, np.float64(best_dist))


def scene_rows(items):
    """The (item, candidate) rows the reference's loop scores (:299-337): every candidate with at
    least 2 vertices, in item order.  Returns (rows [(item, candidate)], raw candidate lines,
    GT polyline per row or None, GT polylines for the calibration (every item GT with >= 2 vertices))."""
    rows, raw, gts, cal_gt = [], [], [], []
    for i, item in enumerate(items):
        gt = item.get("position")
        gt = None if gt is None else np.asarray(gt, dtype=np.float64).reshape(-1, 3)
        if gt is not None and len(gt) > 1:
            cal_gt.append(gt)
        for k, cand in enumerate(item.get("noisy_candidates", [])):
            cand = np.asarray(cand, dtype=np.float64).reshape(-1, 3)
            if len(cand) < 2:
                continue                                                     # :327
            rows.append((i, k))
            raw.append(cand)
            gts.append(gt if gt is not None and len(gt) > 1 else None)
    return rows, raw, gts, cal_gt


@torch.no_grad()
def evaluate_scene(model, pcd_points, items, num_line_points=32, num_context_points=1024, crop_radius=0.3,
                   decay_scale=2.0, batch_lines=2048, seed=0, precision=None):
    """Refine and score every (item, candidate) line of one scene (inference_whole_scene.py:299-365).

    items: io.load_scene_items output.  The refined lines come from refine_scene's path (same
    contexts, same forward); the metrics use the fp64 resample of each noisy line plus the model's
    offset, as the reference does.  Returns a dict of per-row numpy arrays - item_index,
    candidate_index, noisy (R,M,3), refined (R,M,3) and every field of line_metrics - plus
      calibration           calibrate_alignment(raw noisy candidates, item GTs) as the reference
                            computes it (:384-386), None when either list is empty
      calibration_refined   NOT in the reference: the same sweep on the refined lines (R x M points)
    """
    from .context import resample_polylines_device
    from .io import scene_offsets
    dev = G.device("metrics")
    rows, raw, gts, cal_gt = scene_rows(items)
    m = int(num_line_points)
    out = {"item_index": np.array([r[0] for r in rows], dtype=np.int64),
           "candidate_index": np.array([r[1] for r in rows], dtype=np.int64)}
    if rows:
        offset, _, _ = scene_offsets(model, pcd_points, raw, m, num_context_points, crop_radius, decay_scale,
                                     batch_lines, seed, precision)
        noisy = resample_polylines_device(raw, m, offset.device)
        refined = noisy + offset.double()
        gt_index = np.array([-1 if g is None else r for r, g in enumerate(gts)], dtype=np.int64)
        out.update(line_metrics(noisy, refined, gts, gt_index))
        out["noisy"], out["refined"] = noisy.cpu().numpy(), refined.cpu().numpy()
    else:
        empty = line_metrics(np.zeros((0, m, 3)), np.zeros((0, m, 3)), [], np.zeros(0, dtype=np.int64))
        out.update(empty)
        out["noisy"], out["refined"] = np.zeros((0, m, 3)), np.zeros((0, m, 3))
    out["calibration"] = calibrate_alignment(raw, cal_gt) if raw and cal_gt else None
    out["calibration_refined"] = calibrate_alignment(list(out["refined"]), cal_gt) if rows and cal_gt else None
    return out
