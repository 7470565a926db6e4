"""GPU context builder: the per-line crop / weight / sample / centre step of
the reference's ``LaneRefineDataset.__getitem__`` (src/dataset.py:205-253) and
``process_single_line`` (inference_whole_scene.py:94-131), batched over all polylines of a scene
on the HIP path (``prh_context_build``).  Host side: polyline resampling (tiny, numpy).

    cloud = torch.from_numpy(pcd_points).float().cuda()            # (P,4) xyz + intensity
    ctx, noisy, centres, counts = build_contexts(cloud, raw_lines, num_context_points=1024,
                                                 crop_radius=0.3, seed=epoch)
    offsets = model(ctx, noisy)                                     # (6,L,32,3)
    refined = noisy + centres[:, None, :] + offsets[-1]             # original coordinates
"""
import ctypes as C

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L

DENSE_POINTS = 200          # src/dataset.py:214: tube continuity needs ~0.25 m spacing
CROP_BLOCK = 256            # points per work item of the crop passes (csrc/prh_context.hpp)
CANDIDATE_BYTES = 8         # per candidate of the ragged builder: int32 row + uint32 key


def resample_polyline(points, num_points=32):
    """Arc-length resampling by linear interpolation (reference: src/dataset.py:8-29)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if len(points) < 2:
        return np.zeros((num_points, 3))
    cum = np.concatenate(([0.0], np.cumsum(np.linalg.norm(np.diff(points, axis=0), axis=1))))
    t = np.linspace(0.0, cum[-1], num_points)
    return np.stack([np.interp(t, cum, points[:, k]) for k in range(3)], axis=1)


def resample_polylines_device(raw_lines, num_points, device):
    """resample_polyline for a list of polylines at once, on the device in float64 (padded
    cumulative arc lengths, searchsorted, linear interpolation = numpy.interp): (L,num_points,3)
    float64.  Lines with fewer than 2 points give zeros, as in the reference."""
    L = len(raw_lines)
    out = torch.zeros((L, num_points, 3), dtype=torch.float64, device=device)
    lens = [len(l) for l in raw_lines]
    keep = [i for i, n in enumerate(lens) if n >= 2]
    if not keep:
        return out
    nmax = max(lens[i] for i in keep)
    pad = np.zeros((len(keep), nmax, 3))
    cnt = np.zeros(len(keep), dtype=np.int64)
    for r, i in enumerate(keep):
        a = np.asarray(raw_lines[i], dtype=np.float64).reshape(-1, 3)
        pad[r, :len(a)] = a
        pad[r, len(a):] = a[-1]                 # repeat the end point: zero-length segments
        cnt[r] = len(a)
    pts = torch.from_numpy(pad).to(device)
    seg = (pts[:, 1:] - pts[:, :-1]).norm(dim=2)
    cum = torch.cat([torch.zeros((len(keep), 1), dtype=torch.float64, device=device), seg.cumsum(1)], 1)
    total = cum[:, -1:]
    t = total * torch.linspace(0.0, 1.0, num_points, dtype=torch.float64, device=device)[None, :]
    t[:, -1] = total[:, 0]
    # numpy.interp: index of the last knot <= t among the line's own knots
    n = torch.from_numpy(cnt).to(device)
    idx = torch.searchsorted(cum, t, right=True) - 1
    idx = torch.minimum(idx.clamp_(min=0), (n - 2)[:, None])
    x0, x1 = cum.gather(1, idx), cum.gather(1, idx + 1)
    w = ((t - x0) / (x1 - x0).clamp_min(1e-300)).clamp_(0.0, 1.0)
    w = torch.where(x1 > x0, w, torch.zeros_like(w))
    p0 = pts.gather(1, idx[:, :, None].expand(-1, -1, 3))
    p1 = pts.gather(1, (idx + 1)[:, :, None].expand(-1, -1, 3))
    out[torch.tensor(keep, device=device)] = p0 + (p1 - p0) * w[:, :, None]
    return out


def build_contexts_resampled(cloud, dense, line, num_context_points=1024, crop_radius=0.3,
                             decay_scale=2.0, seed=0, max_candidates=None, return_weights=False):
    """cloud (P,4), dense (L,D,3), line (L,M,3) float32 CUDA tensors ->
    context (L,N,4) centred on each line's mean, counts (L,) int32 [, weights (L,max_candidates)].

    The reference samples from EVERY point of a line's tube (src/dataset.py:86-130).  The kernels
    compact a tube's points into a candidate buffer of `max_candidates` slots per line; with
    max_candidates=None (default) the buffer starts at max(4*N, 8192) slots and, when the largest
    tube of the call turns out to hold more points than that (dense LiDAR at the training radius),
    the call is repeated with the buffer sized from the true counts - the draw is then identical
    to what a large enough buffer gives in the first place (same seed, same candidates in cloud
    order).  An explicit max_candidates is taken as is and a RuntimeWarning reports any tube it
    truncated."""
    for t, name in ((cloud, "cloud"), (dense, "dense"), (line, "line")):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(f"build_contexts: {name} must be a float32 CUDA tensor (there is no CPU fallback)")
    cloud, dense, line = cloud.contiguous(), dense.contiguous(), line.contiguous()
    if cloud.dim() != 2 or cloud.shape[1] != 4:
        raise RuntimeError(f"build_contexts: cloud must be (P,4), got {tuple(cloud.shape)}")
    if dense.dim() != 3 or line.dim() != 3 or dense.shape[0] != line.shape[0] or dense.shape[2] != 3 or line.shape[2] != 3:
        raise RuntimeError("build_contexts: dense (L,D,3) and line (L,M,3) expected")
    dev = cloud.device
    n_lines, n = dense.shape[0], int(num_context_points)
    npts = cloud.shape[0]
    auto = max_candidates is None
    if auto:
        max_candidates = max(4 * n, 8192)
    max_candidates = max(int(max_candidates), n + 1)
    out = torch.empty((n_lines, n, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((n_lines,), dtype=torch.int32, device=dev)
    if n_lines == 0:
        weights = torch.zeros((0, max_candidates), dtype=torch.float32, device=dev) if return_weights else None
        return (out, counts, weights) if return_weights else (out, counts)
    lib = L.lib()
    p = G.ptr
    while True:
        weights = torch.zeros((n_lines, max_candidates), dtype=torch.float32, device=dev) if return_weights else None
        nb = lib.prh_context_workspace_bytes(npts, n_lines, max_candidates)
        ws = G.workspace(nb, dev)
        L.check(lib.prh_context_build(p(cloud), npts, p(dense), dense.shape[1], p(line), line.shape[1], n_lines,
                                      float(crop_radius), float(decay_scale), n, max_candidates,
                                      C.c_ulonglong(int(seed) & 0xFFFFFFFFFFFFFFFF), p(out), p(counts), p(weights),
                                      p(ws), nb, dev.index, G.stream(dev)), "prh_context_build")
        largest = int(counts.max().item())           # one small read-back per scene
        if largest <= max_candidates:
            break
        if not auto:
            import warnings
            warnings.warn(f"build_contexts: a tube holds {largest} points but max_candidates={max_candidates}; "
                          f"its context was drawn from the first {max_candidates} points in cloud order only "
                          "(pass max_candidates=None to size the buffer from the counts)", RuntimeWarning)
            break
        max_candidates = largest                     # true counts are known now: one exact repeat
    return (out, counts, weights) if return_weights else (out, counts)


def build_contexts(cloud, raw_lines, num_line_points=32, num_context_points=1024, crop_radius=0.3,
                   decay_scale=2.0, seed=0, max_candidates=None):
    """raw_lines: sequence of (n_i,3) polylines in scene coordinates.  Returns
    context (L,N,4), noisy_line (L,M,3) centred, centres (L,3), counts (L,) - the model inputs of
    inference_whole_scene.py:98-126 for every line at once."""
    dev = cloud.device
    dense_t = resample_polylines_device(raw_lines, DENSE_POINTS, dev).float()
    line_t = resample_polylines_device(raw_lines, num_line_points, dev).float()
    ctx, counts = build_contexts_resampled(cloud, dense_t, line_t, num_context_points, crop_radius, decay_scale,
                                           seed, max_candidates)
    centres = line_t.mean(dim=1)
    return ctx, line_t - centres[:, None, :], centres, counts


# ------------------------------------------------------------------ ragged: many slices, one pass
def ragged_block_offsets(slice_offsets, line_slice):
    """Host plan of the ragged crop passes: (L+1,) int64, the exclusive scan over the lines of
    ceil(points of the line's slice / CROP_BLOCK).  Work item i belongs to the line l with
    out[l] <= i < out[l+1]; a line of an empty slice has none; out[-1] is the grid size.
    slice_offsets (S+1,) starts at 0 and never decreases; line_slice (L,) never decreases (lines are
    grouped by slice) and names slices 0..S-1 - RuntimeError otherwise, as the library says too."""
    so = np.asarray(slice_offsets, dtype=np.int64).reshape(-1)
    ls = np.asarray(line_slice, dtype=np.int64).reshape(-1)
    if len(so) < 2 or so[0] != 0 or (np.diff(so) < 0).any():
        raise RuntimeError("build_contexts_ragged: slice_offsets must start at 0 and never decrease")
    if len(ls) and (ls.min() < 0 or ls.max() >= len(so) - 1):
        raise RuntimeError(f"build_contexts_ragged: line_slice names a slice outside 0..{len(so) - 2}")
    if (np.diff(ls) < 0).any():
        raise RuntimeError("build_contexts_ragged: line_slice must never decrease (lines are grouped by slice)")
    blocks = (np.diff(so) + (CROP_BLOCK - 1)) // CROP_BLOCK
    out = G.csr_offsets(blocks[ls])
    return out


def ragged_runs(cand_offsets, max_candidate_bytes=None):
    """Runs of consecutive lines [(l0, l1), ...] covering 0..L whose candidates fit the byte budget
    (CANDIDATE_BYTES each; None: one run).  Greedy from the left; a line that alone exceeds the
    budget runs alone - the budget bounds the buffers of every other run."""
    co = np.asarray(cand_offsets, dtype=np.int64).reshape(-1)
    n = len(co) - 1
    if max_candidate_bytes is None:
        return [(0, n)] if n > 0 else []
    room = max(int(max_candidate_bytes), 0) // CANDIDATE_BYTES
    runs, l0 = [], 0
    while l0 < n:
        # the last l1 with co[l1] - co[l0] <= room, at least l0 + 1
        l1 = max(int(np.searchsorted(co, co[l0] + room, side="right")) - 1, l0 + 1)
        runs.append((l0, min(l1, n)))
        l0 = min(l1, n)
    return runs


def build_contexts_ragged_resampled(points, slice_offsets, dense, line, line_slice, slice_seeds,
                                    num_context_points=1024, crop_radius=0.3, decay_scale=2.0,
                                    max_candidate_bytes=None):
    """build_contexts_resampled for the lines of many slices at once (prh_context_ragged_count /
    _select): points (T,4) float32 CUDA holds the slices back to back, slice_offsets (S+1,) int64
    (host array, or a tensor that is read back) cuts it, line l of dense (L,D,3) / line (L,M,3) is
    cropped from slice line_slice[l] (never decreasing) and drawn with slice_seeds[line_slice[l]].
    Returns context (L,N,4), counts (L,) int32 - the bytes build_contexts_resampled gives per slice
    for that slice's points, lines and seed (a line's index in the hash is its position among its
    slice's lines, a point's its row within the slice).

    The candidates live in one CSR buffer sized from the true counts after one read-back: no
    max_candidates, no repeat.  max_candidate_bytes bounds that buffer (8 bytes per candidate): over
    it, the fill and draw pass runs over consecutive runs of lines (ragged_runs) that reuse the
    buffer; the result does not depend on the budget."""
    for t, name in ((points, "points"), (dense, "dense"), (line, "line")):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(f"build_contexts_ragged: {name} must be a float32 CUDA tensor (there is no CPU fallback)")
    points, dense, line = points.contiguous(), dense.contiguous(), line.contiguous()
    if points.dim() != 2 or points.shape[1] != 4:
        raise RuntimeError(f"build_contexts_ragged: points must be (T,4), got {tuple(points.shape)}")
    if dense.dim() != 3 or line.dim() != 3 or dense.shape[0] != line.shape[0] or dense.shape[2] != 3 or line.shape[2] != 3:
        raise RuntimeError("build_contexts_ragged: dense (L,D,3) and line (L,M,3) expected")
    if torch.is_tensor(slice_offsets):
        slice_offsets = slice_offsets.cpu().numpy()
    so = np.ascontiguousarray(slice_offsets, dtype=np.int64).reshape(-1)
    ls = np.ascontiguousarray(line_slice, dtype=np.int32).reshape(-1)
    seeds = np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in slice_seeds], dtype=np.uint64)
    n_lines, n, n_slices = dense.shape[0], int(num_context_points), len(so) - 1
    if len(ls) != n_lines or len(seeds) != n_slices:
        raise RuntimeError("build_contexts_ragged: one line_slice entry per line and one seed per slice expected")
    blk = ragged_block_offsets(so, ls)
    if so[-1] != points.shape[0]:
        raise RuntimeError(f"build_contexts_ragged: slice_offsets end at {so[-1]}, points has {points.shape[0]} rows")
    dev = points.device
    out = torch.empty((n_lines, n, 4), dtype=torch.float32, device=dev)
    counts = torch.empty((n_lines,), dtype=torch.int32, device=dev)
    if n_lines == 0:
        return out, counts
    lib = L.lib()
    p = G.ptr
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    cand_offsets = torch.empty((n_lines + 1,), dtype=torch.int64, device=dev)
    nb = lib.prh_context_ragged_workspace_bytes(n_lines, int(blk[-1]))
    if nb == 0:
        raise RuntimeError(f"build_contexts_ragged: {int(blk[-1])} (line, block) work items do not fit one call")
    ws = G.workspace(nb, dev)
    L.check(lib.prh_context_ragged_count(p(points), hp(so), n_slices, p(dense), dense.shape[1], hp(ls), hp(seeds),
                                         n_lines, float(crop_radius), p(counts), p(cand_offsets), p(ws), nb,
                                         dev.index, G.stream(dev)), "prh_context_ragged_count")
    total = int(cand_offsets[-1].item())                 # the one read-back of the call
    if max_candidate_bytes is None or total * CANDIDATE_BYTES <= int(max_candidate_bytes):
        runs, sizes = [(0, n_lines)], [total]
    else:
        co = cand_offsets.cpu().numpy()
        runs = ragged_runs(co, max_candidate_bytes)
        sizes = [int(co[l1] - co[l0]) for l0, l1 in runs]
    cap = max(sizes)
    cand = torch.empty((cap,), dtype=torch.int32, device=dev)
    keys = torch.empty((cap,), dtype=torch.int32, device=dev)          # uint32 keys, float weights before them
    for l0, l1 in runs:
        L.check(lib.prh_context_ragged_select(p(points), hp(so), n_slices, p(dense), dense.shape[1], p(line),
                                              line.shape[1], hp(ls), n_lines, float(crop_radius), float(decay_scale),
                                              n, p(counts), p(cand_offsets), l0, l1, p(cand), p(keys), cap, p(out),
                                              p(ws), nb, dev.index, G.stream(dev)), "prh_context_ragged_select")
    return out, counts


def build_contexts_ragged(points, slice_offsets, raw_lines, line_slice, slice_seeds, num_line_points=32,
                          num_context_points=1024, crop_radius=0.3, decay_scale=2.0, max_candidate_bytes=None):
    """build_contexts for the lines of many slices in one pass: raw_lines is the flat list of (n_i,3)
    polylines, each in the frame of its slice line_slice[i] (never decreasing).  Returns context
    (L,N,4), noisy_line (L,M,3) centred, centres (L,3), counts (L,); see
    build_contexts_ragged_resampled for points, slice_offsets, slice_seeds and the memory budget."""
    if not (torch.is_tensor(points) and points.is_cuda):
        raise RuntimeError("build_contexts_ragged: points must be a float32 CUDA tensor (there is no CPU fallback)")
    dev = points.device
    dense_t = resample_polylines_device(raw_lines, DENSE_POINTS, dev).float()
    line_t = resample_polylines_device(raw_lines, num_line_points, dev).float()
    ctx, counts = build_contexts_ragged_resampled(points, slice_offsets, dense_t, line_t, line_slice, slice_seeds,
                                                  num_context_points, crop_radius, decay_scale, max_candidate_bytes)
    centres = line_t.mean(dim=1)
    return ctx, line_t - centres[:, None, :], centres, counts
