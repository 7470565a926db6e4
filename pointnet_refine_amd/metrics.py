"""Scene evaluation on the GPU: the metric half of the reference's whole-scene script
(inference_whole_scene.py:26-92,170-193,299-387), whose scipy KDTree helpers run one line at a
time on the host.  fp64 HIP kernels (``csrc/prh_metrics.hpp``) compute, for every (item,
candidate) line of a scene at once:

  line_metrics         crop_gt_to_pred_range + resample_polyline + ADE + compute_chamfer_distance
                       for the noisy and the refined line (valid / bad_match as at :310,337-365)
  shift_sweep          mean_p min_g |pred_p + (dx,dy,0) - gt_g| for many shifts in one launch
  calibrate_alignment  the reference's coarse / fine (dx, dy) search on top of shift_sweep
  evaluate_scene       refine_scene's contexts and forward + the above, per scene
  shift_sweep_ragged   many independent shift_sweep problems in one launch pair, bitwise what one
                       shift_sweep call per problem gives
  calibrate_alignments calibrate_alignment for many problems: two ragged launches in all
  evaluate_scenes      evaluate_scene for a list of scenes in one ragged pass (one context build
                       and forward per group of scenes, one line_metrics, one calibrate_alignments)

    items = io.load_scene_items(json_path)
    res = evaluate_scene(model, io.load_pcd_data(pcd_path), items)
    res["ade_noisy"], res["ade_refined"], res["calibration"]       # per-row arrays, ((dx,dy), dist)

There is no CPU fallback: without a GPU every function raises RuntimeError.
"""
import ctypes as C

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
    offsets = G.csr_offsets([len(g) for g in gts])
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
    return np.stack([np.repeat(xs, len(ys)), np.tile(ys, len(xs))], axis=1).astype(np.float64).reshape(-1, 2)   # x outer, y inner


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


# ------------------------------------------------------------------ ragged: many problems, one pass
SWEEP_QUERIES, SWEEP_SHIFTS = 256, 16          # csrc/prh_metrics.hpp: SW_THREADS, SW_SB
_MAX_ITEMS = 2 ** 31 - 1


def sweep_work_items(pred_counts, shift_counts):
    """Host plan of the ragged sweep: (item_offsets (n+1,) int64, n_qt (n,) int64).  Problem p has
    n_qt[p] = ceil(P_p / 256) query tiles and ceil(S_p / 16) shift tiles; item_offsets is the
    exclusive scan of their product, item_offsets[-1] the grid size (the library builds the same
    table from the offsets it is given)."""
    pc = np.asarray(pred_counts, dtype=np.int64).reshape(-1)
    sc = np.asarray(shift_counts, dtype=np.int64).reshape(-1)
    if len(pc) != len(sc) or (pc <= 0).any() or (sc <= 0).any():
        raise ValueError("sweep_work_items: one positive point count and one positive shift count per problem")
    n_qt = (pc + (SWEEP_QUERIES - 1)) // SWEEP_QUERIES
    out = G.csr_offsets(n_qt * ((sc + (SWEEP_SHIFTS - 1)) // SWEEP_SHIFTS))
    return out, n_qt


def sweep_item(item_offsets, n_qt, item):
    """(problem, query tile, shift tile) of a work item, as the kernel finds them: the last problem
    whose first item is <= item, then the tiles by division (the query tile runs fastest)."""
    p = int(np.searchsorted(item_offsets, item, side="right")) - 1
    r = int(item) - int(item_offsets[p])
    return p, r % int(n_qt[p]), r // int(n_qt[p])


def _points_csr(sets, width):
    """A list of (n,width) numpy arrays as one (N,width) float64 array and its (len+1,) int64 offsets."""
    arrs = [np.asarray(a, dtype=np.float64).reshape(-1, width) for a in sets]
    off = G.csr_offsets([len(a) for a in arrs])
    return (np.concatenate(arrs) if len(arrs) and off[-1] > 0 else np.zeros((0, width))), off


def _upload_packed(arrays, dev):
    """Several float64 host arrays in ONE upload: views of one device buffer, in the arrays' shapes."""
    sizes = [a.size for a in arrays]
    host = np.concatenate([np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in arrays]) if sum(sizes) else np.zeros(1)
    buf = torch.from_numpy(host).to(dev)
    out, at = [], 0
    for a, n in zip(arrays, sizes):
        out.append(buf[at:at + n].view(a.shape))
        at += n
    return out


def _sweep_ragged(pred_t, pred_off, gt_t, gt_off, gt_index, shifts_t, shift_off, dev):
    """One prh_shift_sweep_ragged call on device buffers and host CSR arrays; (total shifts,) numpy."""
    n = len(pred_off) - 1
    items, _ = sweep_work_items(np.diff(pred_off), np.diff(shift_off))
    if items[-1] > _MAX_ITEMS:
        raise ValueError(f"shift_sweep_ragged: {int(items[-1])} (problem, query tile, shift tile) work items do not fit one call")
    pred_off, gt_off, shift_off = (np.ascontiguousarray(o, dtype=np.int64) for o in (pred_off, gt_off, shift_off))
    gi = np.ascontiguousarray(gt_index, dtype=np.int32)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    out = torch.empty((int(shift_off[-1]),), dtype=torch.float64, device=dev)
    lib = L.lib()
    nb = lib.prh_shift_sweep_ragged_workspace_bytes(hp(pred_off), hp(shift_off), n)
    ws = G.workspace(nb, dev)
    L.check(lib.prh_shift_sweep_ragged(G.ptr(pred_t), hp(pred_off), G.ptr(gt_t), hp(gt_off), len(gt_off) - 1, hp(gi),
                                       G.ptr(shifts_t), hp(shift_off), n, G.ptr(out), G.ptr(ws), nb, dev.index,
                                       G.stream(dev)), "prh_shift_sweep_ragged")
    return out.cpu().numpy()


def _device_csr(sets, width, dev, what):
    """Sets given as CUDA tensors (numpy sets are uploaded one by one): (flat (N,width) CUDA float64, offsets)."""
    ts = [G.as_cuda(a, dev, what, torch.float64).reshape(-1, width) for a in sets]
    off = G.csr_offsets([t.shape[0] for t in ts])
    return (torch.cat(ts) if ts else torch.zeros((0, width), dtype=torch.float64, device=dev)), off


def shift_sweep_ragged(pred_sets, gt_sets, shifts, gt_index=None):
    """shift_sweep for many independent problems in one launch pair (prh_shift_sweep_ragged).

    pred_sets: one (P_p,3) point set per problem; gt_sets: (G,3) point sets; shifts: one (S_p,2)
    array per problem; gt_index (n,): the GT set of each problem, so that problems may share one
    (default: problem p uses gt_sets[p]).  Point sets are numpy arrays or CUDA tensors.  Returns a
    list of (S_p,) float64 arrays, entry p bitwise what shift_sweep(pred_sets[p],
    gt_sets[gt_index[p]], shifts[p]) returns.  With numpy inputs everything goes up in one upload;
    the means come back in one read-back.  A problem without a prediction point, a GT point or a
    shift is left out of the call (the mean over nothing: its entry is S_p NaNs)."""
    dev = G.device("metrics")
    n = len(pred_sets)
    if len(shifts) != n:
        raise ValueError("shift_sweep_ragged: one shift array per problem expected")
    if gt_index is None:
        if len(gt_sets) != n:
            raise ValueError("shift_sweep_ragged: without gt_index, gt_sets needs one set per problem")
        gt_index = np.arange(n)
    gt_index = np.asarray(gt_index, dtype=np.int64).reshape(-1)
    if len(gt_index) != n or (n and (gt_index.min() < 0 or gt_index.max() >= len(gt_sets))):
        raise ValueError("shift_sweep_ragged: gt_index must hold one index in [0, len(gt_sets)) per problem")
    sh = [np.asarray(s, dtype=np.float64).reshape(-1, 2) for s in shifts]
    rows = lambda a: int(a.numel() if torch.is_tensor(a) else np.asarray(a).size) // 3
    n_pred, n_gt = [rows(a) for a in pred_sets], [rows(a) for a in gt_sets]
    live = [p for p in range(n) if n_pred[p] > 0 and n_gt[gt_index[p]] > 0 and len(sh[p]) > 0]
    out = [np.full((len(s),), np.nan) for s in sh]
    if not live:
        return out
    used = sorted({int(gt_index[p]) for p in live})                       # GT sets that reach the device
    slot = {g: k for k, g in enumerate(used)}
    preds, gts = [pred_sets[p] for p in live], [gt_sets[g] for g in used]
    sh_flat, sh_off = _points_csr([sh[p] for p in live], 2)
    if any(torch.is_tensor(a) for a in preds + gts):
        pred_t, pred_off = _device_csr(preds, 3, dev, "shift_sweep_ragged")
        gt_t, gt_off = _device_csr(gts, 3, dev, "shift_sweep_ragged")
        sh_t = torch.from_numpy(sh_flat).to(dev)
    else:
        pred_flat, pred_off = _points_csr(preds, 3)
        gt_flat, gt_off = _points_csr(gts, 3)
        pred_t, gt_t, sh_t = _upload_packed([pred_flat, gt_flat, sh_flat], dev)
    means = _sweep_ragged(pred_t, pred_off, gt_t, gt_off, [slot[int(gt_index[p])] for p in live], sh_t, sh_off, dev)
    for k, p in enumerate(live):
        out[p] = means[sh_off[k]:sh_off[k + 1]].copy()
    return out


def fine_grids(best_offsets):
    """The fine grid of calibrate_alignment around each (dx, dy) of best_offsets (n,2): the same two
    np.arange calls per problem; their lengths go into the shift CSR as they come out."""
    return [_grid(np.arange(bx - 2.0, bx + 2.0, 0.2), np.arange(by - 1.0, by + 1.0, 0.2)) for bx, by in best_offsets]


def pick_shifts(shifts, means, offsets, best_dist, best_offset):
    """calibrate_alignment's choice, vectorised over problems.  shifts (T,2) and means (T,) are CSR
    rows cut by offsets (n+1,); best_dist (n,) and best_offset (n,2) carry the choice so far (inf and
    (0, 0) at the start).  Per problem: the first shift, in order, whose mean is the smallest one, if
    that mean is strictly below best_dist - what `if d < best_dist` gives in a loop.  A NaN mean is
    never chosen.  Returns the updated (best_dist, best_offset)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    best_dist, best_offset = np.array(best_dist, dtype=np.float64), np.array(best_offset, dtype=np.float64).reshape(-1, 2)
    n, lens = len(offsets) - 1, np.diff(offsets)
    if n == 0 or lens.max() == 0:
        return best_dist, best_offset
    table = np.full((n, int(lens.max())), np.inf)
    row = np.repeat(np.arange(n), lens)
    col = np.arange(int(offsets[-1])) - np.repeat(offsets[:-1], lens)
    means = np.asarray(means, dtype=np.float64)
    table[row, col] = np.where(np.isnan(means), np.inf, means)
    j = table.argmin(axis=1)                                        # the first index of the minimum
    v = table[np.arange(n), j]
    take = v < best_dist
    best_dist[take] = v[take]
    best_offset[take] = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)[offsets[:-1][take] + j[take]]
    return best_dist, best_offset


def calibrate_alignments(pred_lines_per_problem, gt_lines_per_problem, gt_index=None, return_tables=False):
    """calibrate_alignment for many problems at once: entry p of the returned list equals
    calibrate_alignment(pred_lines_per_problem[p], gt_lines_per_problem[gt_index[p]], return_tables).

    pred_lines_per_problem: one list of (n,3) polylines (or an (R,M,3) array) per problem;
    gt_lines_per_problem: lists of GT polylines; gt_index (n,): the GT list of each problem (default:
    its own), so that two problems - the raw and the refined lines of a scene - share one upload.
    One ragged launch runs the 400 coarse shifts of every problem, the choice runs on the host
    (pick_shifts), the fine grids are built per problem (fine_grids) and a second ragged launch runs
    them.  A problem with an empty list gives ((0, 0), 999.0) without reaching the device."""
    n = len(pred_lines_per_problem)
    if gt_index is None:
        if len(gt_lines_per_problem) != n:
            raise ValueError("calibrate_alignments: without gt_index, one GT list per problem expected")
        gt_index = np.arange(n)
    gt_index = np.asarray(gt_index, dtype=np.int64).reshape(-1)
    if len(gt_index) != n or (n and (gt_index.min() < 0 or gt_index.max() >= len(gt_lines_per_problem))):
        raise ValueError("calibrate_alignments: gt_index must hold one index in [0, len(gt_lines_per_problem)) per problem")
    out = [((0, 0), 999.0, {}) if return_tables else ((0, 0), 999.0)] * n
    live = [p for p in range(n) if len(pred_lines_per_problem[p]) > 0 and len(gt_lines_per_problem[gt_index[p]]) > 0]
    if not live:
        return out
    dev = G.device("metrics")
    used = sorted({int(gt_index[p]) for p in live})
    slot = {g: k for k, g in enumerate(used)}
    gi = [slot[int(gt_index[p])] for p in live]
    pred_flat, pred_off = _points_csr([np.vstack(pred_lines_per_problem[p]) for p in live], 3)
    gt_flat, gt_off = _points_csr([np.vstack(gt_lines_per_problem[g]) for g in used], 3)
    k = len(live)
    coarse = _grid(np.arange(-20, 20, 2.0), np.arange(-10, 10, 1.0))
    c_flat, c_off = np.tile(coarse, (k, 1)), np.arange(k + 1, dtype=np.int64) * len(coarse)
    pred_t, gt_t, c_t = _upload_packed([pred_flat, gt_flat, c_flat], dev)
    c_means = _sweep_ragged(pred_t, pred_off, gt_t, gt_off, gi, c_t, c_off, dev)
    best_dist, best_offset = pick_shifts(c_flat, c_means, c_off, np.full(k, np.inf), np.zeros((k, 2)))
    f_flat, f_off = _points_csr(fine_grids(best_offset), 2)
    f_means = _sweep_ragged(pred_t, pred_off, gt_t, gt_off, gi, torch.from_numpy(f_flat).to(dev), f_off, dev)
    best_dist, best_offset = pick_shifts(f_flat, f_means, f_off, best_dist, best_offset)
    for q, p in enumerate(live):
        res = ((np.float64(best_offset[q, 0]), np.float64(best_offset[q, 1])), np.float64(best_dist[q]))
        if return_tables:
            res += ({"coarse": (coarse, c_means[c_off[q]:c_off[q + 1]].copy()),
                     "fine": (f_flat[f_off[q]:f_off[q + 1]].copy(), f_means[f_off[q]:f_off[q + 1]].copy())},)
        out[p] = res
    return out


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


def scene_groups(n_points, max_points=None):
    """Consecutive groups [(s0, s1), ...] of scenes whose clouds (n_points per scene) together hold
    at most max_points points (None: one group).  Greedy from the left; a scene over the budget runs alone."""
    n = len(n_points)
    if max_points is None:
        return [(0, n)] if n else []
    groups, s0, held = [], 0, 0
    for s in range(n):
        if s > s0 and held + int(n_points[s]) > int(max_points):
            groups.append((s0, s))
            s0, held = s, 0
        held += int(n_points[s])
    if n > s0:
        groups.append((s0, n))
    return groups


def _cloud_rows(cloud):
    return int(cloud.shape[0]) if cloud.ndim == 2 else 0


@torch.no_grad()
def evaluate_scenes(model, scenes, num_line_points=32, num_context_points=1024, crop_radius=0.3, decay_scale=2.0,
                    batch_lines=2048, seed=0, precision=None, max_points=None, max_candidate_bytes=None):
    """evaluate_scene for a list of scenes in one ragged pass.

    scenes: list of (cloud, items) - cloud a numpy (n,>=4) array or a float32 CUDA tensor, items
    io.load_scene_items output.  Returns one dict per scene with the keys and dtypes of
    evaluate_scene.  The clouds are concatenated into one device buffer; one
    io.scene_offsets_ragged call builds every row's context from its own scene's cloud (byte for
    byte the per-scene contexts: every slice seed is `seed`) and runs the forward; then come one
    resample, one line_metrics call over all rows and one calibrate_alignments call with two
    problems per scene (raw candidates, refined lines) that share the scene's GT points.

    max_points cuts the scene list into consecutive groups whose clouds fit that many points, one
    buffer and one scene_offsets_ragged call per group (a scene over the budget runs alone);
    max_candidate_bytes is the ragged builder's candidate budget.  Only `refined` (and the metrics
    of the refined line) depend on the grouping, by which rows share a forward call - within fp32
    rounding of evaluate_scene; every other field is exactly evaluate_scene's."""
    from .context import resample_polylines_device
    from .io import scene_offsets_ragged
    dev = G.device("metrics")
    m = int(num_line_points)
    per_scene = [scene_rows(items) for _, items in scenes]                   # rows, raw, gts, cal_gt
    with_rows = [s for s, r in enumerate(per_scene) if r[0]]
    row_off = G.csr_offsets([len(r[0]) for r in per_scene])
    n_rows = int(row_off[-1])
    raw_all = [line for r in per_scene for line in r[1]]
    noisy = refined = None
    if n_rows:
        mdev = next(model.parameters()).device
        offsets = []
        for g0, g1 in scene_groups([_cloud_rows(scenes[s][0]) for s in with_rows], max_points):
            group = with_rows[g0:g1]
            so = G.csr_offsets([_cloud_rows(scenes[s][0]) for s in group])
            points = torch.empty((int(so[-1]), 4), dtype=torch.float32, device=mdev)
            for k, s in enumerate(group):                # one cloud at a time: never two copies of all of them
                cloud = scenes[s][0]
                if so[k + 1] == so[k]:
                    continue
                if not torch.is_tensor(cloud):
                    cloud = torch.from_numpy(np.ascontiguousarray(np.asarray(cloud)[:, :4], dtype=np.float32))
                points[so[k]:so[k + 1]].copy_(cloud[:, :4])
                del cloud
            raw = [line for s in group for line in per_scene[s][1]]
            line_slice = np.repeat(np.arange(len(group)), [len(per_scene[s][0]) for s in group])
            offset, _, _ = scene_offsets_ragged(model, points, so, raw, line_slice, [seed] * len(group), m,
                                                num_context_points, crop_radius, decay_scale, batch_lines, precision,
                                                max_candidate_bytes=max_candidate_bytes)
            offsets.append(offset)
            del points
        offset = offsets[0] if len(offsets) == 1 else torch.cat(offsets)
        noisy = resample_polylines_device(raw_all, m, offset.device)
        refined = noisy + offset.double()
        gts_all, gt_index = [], np.empty(n_rows, dtype=np.int64)
        for s, (rows, _, gts, _) in enumerate(per_scene):
            gt_index[row_off[s]:row_off[s + 1]] = [-1 if g is None else row_off[s] + r for r, g in enumerate(gts)]
            gts_all.extend(gts)
        lm = line_metrics(noisy, refined, gts_all, gt_index)
        noisy, refined = noisy.cpu().numpy(), refined.cpu().numpy()
    else:
        lm = line_metrics(np.zeros((0, m, 3)), np.zeros((0, m, 3)), [], np.zeros(0, dtype=np.int64))
        noisy = refined = np.zeros((0, m, 3))
    # two calibration problems per scene that has rows and GT, sharing the scene's GT set
    cal_scenes = [s for s in with_rows if per_scene[s][3]]
    preds = [x for s in cal_scenes for x in (per_scene[s][1], refined[row_off[s]:row_off[s + 1]])]
    cal = calibrate_alignments(preds, [per_scene[s][3] for s in cal_scenes], np.repeat(np.arange(len(cal_scenes)), 2)) \
        if cal_scenes else []
    cal_at = {s: k for k, s in enumerate(cal_scenes)}
    out = []
    for s, (rows, _, _, _) in enumerate(per_scene):
        r0, r1 = int(row_off[s]), int(row_off[s + 1])
        d = {"item_index": np.array([r[0] for r in rows], dtype=np.int64),
             "candidate_index": np.array([r[1] for r in rows], dtype=np.int64)}
        d.update({k: v[r0:r1].copy() for k, v in lm.items()})
        d["noisy"], d["refined"] = noisy[r0:r1].copy(), refined[r0:r1].copy()
        k = cal_at.get(s)
        d["calibration"] = None if k is None else cal[2 * k]
        d["calibration_refined"] = None if k is None else cal[2 * k + 1]
        out.append(d)
    return out
