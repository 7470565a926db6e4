"""Paint tracing: lane candidates read from the cloud itself, with no detector and no GT.

Every GT-free stage of the map tools starts from lines something else drew; a drive that has only
merged.pcd and pose/*.json has none.  The paint is in the cloud: per slice ``drive.slice_cloud``
returns, the bright points are summed into a grid of columns along ego x and narrow cells along y,
the cells that are ridges of a column are peaks, peaks of neighbouring columns are linked, and the
chains of links are polylines - 3-D and on the paint, so they go to ``fuse.refine_slices`` as they are
(``csrc/prh_trace.hpp``; the rule is in ``include/pointnet_refine_hip.h``, "Paint tracing - the
rule", and restated in ``tests/_trace_oracle.py``).

  paint_peaks    HIP: the tables, the peaks of every column and their mutual links, for all slices,
                 in chunks of slices whose tables fit table_bytes (the result does not see the chunks)
  chain_lines    host: list ranking over succ, the min_peaks / min_length filter, the polylines (numpy)
  trace_lines    paint_peaks + chain_lines
  refine_cloud   plan_slices, slice_cloud, trace_lines, fuse.refine_slices, link.fuse_unmatched and,
                 where asked, fuse.cloud_support: a lidar drive into a lane map

    lines_per_slice, report = trace_lines(points, offsets, intensity_floor=20.0)

The surface gate ("Paint tracing - the rule: surface gate"): a merged cloud holds bright things that
are not paint - the trail of a followed vehicle's plate half a metre up, guard-rail reflectors, signs -
and they outweigh the paint.  With a ground table (``paintfloor.surface_ground``; ``refine_cloud`` with
``surface=True`` builds it) a bright point counts only within ``band`` of the road height of its 1 m
cell; the others are counted in 'off_surface'.  Off by default, and then every bit is as before.

    table = paintfloor.surface_ground(points, offsets)
    lines_per_slice, report = trace_lines(points, offsets, intensity_floor=20.0, ground=table)

Scope: ridges within about atan(link_cells * cell / col) (17 degrees at the defaults) of the ego x
axis; cross-markings are not traced, and without an intensity_floor that separates paint from asphalt
the rule traces asphalt texture.  Without the surface gate a point counts whatever its height.  With it
the road is what "Ground lift - the rule" finds in constant 1 m cells: a point outside the ground
window is off the surface, and paint on a structure that rule does not call road - a bridge deck above
the lowest mode of its cell - is gated out with the structure.  paint_peaks, trace_lines and
refine_cloud have no CPU fallback: without a GPU they raise RuntimeError.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L
from . import drive as D
from . import fuse as F
from . import link as K
from . import paintfloor as PF

HALF_LENGTH, COL = 25.0, 0.5
HALF_WIDTH, CELL = 12.8, 0.05
MAX_HALF = 128.0             # half_length and half_width: the int64 sums are bounded for it
MAX_CELLS = 4096             # nx and ny
MAX_NMS = 31                 # prh_trace_max_nms()
MAX_SLICE_POINTS = 1 << 22
NMS, MIN_POINTS, MIN_WEIGHT = 4, 3, 1
LINK_CELLS, GAP_SLOPE, MAX_GAP_COLS = 3, 1, 24
MIN_PEAKS, MIN_LENGTH = 3, 5.0
TABLE_BYTES = 256 << 20
CELL_BYTES = 36
PEAK_KEYS = ("iy", "weight", "count", "xyz", "col")
BAND, GROUND_CELL = PF.BAND, PF.GROUND_CELL


def _int(v, lo, hi, name, what):
    if isinstance(v, (bool, np.bool_)) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: {name} must be an integer in {lo} .. {hi}")
    return int(v)


def _params(what, half_length=HALF_LENGTH, col=COL, half_width=HALF_WIDTH, cell=CELL, intensity_floor=0.0, nms=NMS,
            min_points=MIN_POINTS, min_weight=MIN_WEIGHT, link_cells=LINK_CELLS, gap_slope=GAP_SLOPE,
            max_gap_cols=MAX_GAP_COLS, table_bytes=TABLE_BYTES):
    """The checked parameters of paint_peaks, with nx and ny ("Paint tracing - the rule": Grid)."""
    half_length, col, half_width, cell, floor = (float(v) for v in (half_length, col, half_width, cell, intensity_floor))
    if not (0.0 < half_length <= MAX_HALF and 0.0 < half_width <= MAX_HALF):
        raise ValueError(f"{what}: 0 < half_length, half_width <= {MAX_HALF}")
    if not (np.isfinite(col) and col > 0.0 and np.isfinite(cell) and cell > 0.0):
        raise ValueError(f"{what}: col and cell must be positive and finite")
    if not np.isfinite(floor):
        raise ValueError(f"{what}: intensity_floor must be finite")
    fx, fy = np.rint(2.0 * half_length / col), np.rint(2.0 * half_width / cell)
    if not (1 <= fx <= MAX_CELLS and 1 <= fy <= MAX_CELLS):
        raise ValueError(f"{what}: 1 <= nx, ny <= {MAX_CELLS}, got {fx:g} x {fy:g}")
    return {"half_length": half_length, "col": col, "half_width": half_width, "cell": cell, "intensity_floor": floor,
            "nx": int(fx), "ny": int(fy), "nms": _int(nms, 0, MAX_NMS, "nms", what),
            "min_points": _int(min_points, 1, 2 ** 31 - 1, "min_points", what),
            "min_weight": _int(min_weight, 1, 2 ** 62, "min_weight", what),
            "link_cells": _int(link_cells, 0, MAX_CELLS, "link_cells", what),
            "gap_slope": _int(gap_slope, 0, MAX_CELLS, "gap_slope", what),
            "max_gap_cols": _int(max_gap_cols, 0, MAX_CELLS - 1, "max_gap_cols", what),
            "table_bytes": _int(table_bytes, 1, 2 ** 62, "table_bytes", what)}


def _surface_params(what, p, band=BAND, ground_cell=GROUND_CELL):
    """The checked parameters of the surface gate over the trace window of p = _params(...), with gx
    and gy ("Paint tracing - the rule: surface gate"): paintfloor's own check of its grid and band."""
    return PF._params(what, half_length=p["half_length"], half_width=p["half_width"], ground_cell=ground_cell, band=band)


def _chain_params(what, min_peaks, min_length):
    min_length = float(min_length)
    if not np.isfinite(min_length):
        raise ValueError(f"{what}: min_length must be finite")
    return _int(min_peaks, 1, 2 ** 31 - 1, "min_peaks", what), min_length


# ------------------------------------------------------------------ GPU side
def _row_ptr(off_t, s0):
    """The device address of off_t[s0] (int64): the offsets of a chunk's slices."""
    return C.c_void_p(off_t.data_ptr() + 8 * int(s0))


def _chunk_peaks(pts, off_t, off, s0, s1, p, dev, ground=None, sp=None):
    """The tables and the peaks of slices s0 .. s1: (col_counts (k*nx,) int32, the PEAK_KEYS tensors, kept points,
    with a ground table (S,gx,gy) and its parameters sp the (k,) int64 points off the surface, else None)."""
    lib = L.lib()
    k, nx, ny = s1 - s0, p["nx"], p["ny"]
    nb = lib.prh_trace_workspace_bytes(k, nx, ny)
    ws = G.workspace(nb, dev)
    hist = (G.ptr(pts), 1 if pts.dtype == torch.float64 else 0, _row_ptr(off_t, s0), k, int(off[s0]), int(off[s1] - off[s0]),
            p["half_length"], p["col"], nx, p["half_width"], p["cell"], ny, p["intensity_floor"], G.ptr(ws), nb)
    off_surface = None
    if ground is None:
        L.check(lib.prh_trace_hist(*hist, dev.index, G.stream(dev)), "prh_trace_hist")
    else:
        off_surface = torch.empty((k,), dtype=torch.int64, device=dev)
        # the rows of the chunk's own slices: the kernel counts slices from the chunk's first
        L.check(lib.prh_trace_hist_surface(*hist, sp["half_length"], sp["half_width"], sp["ground_cell"], sp["gx"], sp["gy"],
                                           G.ptr(ground[s0:s1]), sp["band"], G.ptr(off_surface), dev.index, G.stream(dev)),
                "prh_trace_hist_surface")
    counts = torch.empty((k * nx,), dtype=torch.int32, device=dev)
    peak = (p["nms"], p["min_points"], p["min_weight"])
    L.check(lib.prh_trace_peaks_count(G.ptr(ws), nb, k, nx, ny, *peak, G.ptr(counts), dev.index, G.stream(dev)),
            "prh_trace_peaks_count")
    col_off = G.exclusive_scan(counts)
    total = int(col_off[-1].item())
    out = {"iy": torch.empty((total,), dtype=torch.int32, device=dev),
           "weight": torch.empty((total,), dtype=torch.int64, device=dev),
           "count": torch.empty((total,), dtype=torch.int32, device=dev),
           "xyz": torch.empty((total, 3), dtype=torch.float64, device=dev),
           "col": torch.empty((total,), dtype=torch.int32, device=dev)}
    if total:
        L.check(lib.prh_trace_peaks_write(G.ptr(ws), nb, k, nx, ny, *peak, G.ptr(col_off), total, s0 * nx, G.ptr(out["iy"]),
                                          G.ptr(out["weight"]), G.ptr(out["count"]), G.ptr(out["xyz"]), G.ptr(out["col"]),
                                          dev.index, G.stream(dev)), "prh_trace_peaks_write")
    kept = ws[:4 * k * nx * ny].view(torch.int32).sum(dtype=torch.int64)      # the workspace begins with n
    return counts, out, kept, off_surface


def paint_peaks(points, slice_offsets, ground=None, band=BAND, ground_cell=GROUND_CELL, **params):
    """The peaks of every column of every slice and their mutual links ("Paint tracing - the rule").

    points (T,4) float64 or float32 x y z intensity, every slice in its own frame, with slice_offsets
    (S+1,) - what drive.slice_cloud returns (CUDA tensors are used where they are, numpy is
    uploaded).  params: half_length, col, half_width, cell, intensity_floor, nms, min_points,
    min_weight, link_cells, gap_slope, max_gap_cols (the rule's), table_bytes (the slices are
    processed in chunks whose tables fit it, at least one slice at a time: cost only).  ground:
    None, or the (S,gx,gy) float64 table of road heights over the trace window, NaN where there is
    none (numpy or CUDA; paintfloor.surface_ground(points, slice_offsets, half_length, half_width,
    ground_cell) makes it), which turns the surface gate on ("Paint tracing - the rule: surface
    gate"): a bright point counts only where fabs(z - ground) <= band in its ground_cell cell, and
    the result gains 'off_surface' (S,) int64, the bright points left out per slice.  Returns a
    dict of CUDA tensors: 'peak_offsets' (S*nx+1,) int64, the CSR of the peaks over (slice, column);
    per peak, in (slice, ix, iy) order, 'iy' int32, 'weight' int64 (b), 'count' int32 (n3), 'xyz'
    (P,3) float64, 'col' int32 (slice * nx + ix), 'succ' and 'pred' int32 (the linked peak, -1:
    none); 'bright_points' () int64, the points that entered the tables.  Bitwise reproducible,
    whatever the order of the points, their dtype or table_bytes."""
    what = "paint_peaks"
    p = _params(what, **params)
    sp = None
    if ground is not None:                                       # checked before the device is asked for
        sp = _surface_params(what, p, band, ground_cell)
        PF.ground_shape(ground, len(G.host(slice_offsets, np.int64).reshape(-1)) - 1, sp, what)
    dev = G.device("trace", points.device if torch.is_tensor(points) and points.is_cuda else None)
    pts = G.points4(points, dev, what)
    off = G.offsets(slice_offsets, pts.shape[0], what, "slice_offsets")
    if ground is not None:
        ground = G.as_cuda(ground, dev, what, torch.float64)
    n_s, nx, ny = len(off) - 1, p["nx"], p["ny"]
    if n_s and int(np.diff(off).max()) >= MAX_SLICE_POINTS:
        raise ValueError(f"{what}: fewer than 2^22 points per slice")
    if n_s * nx >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 columns in all")
    off_t = torch.from_numpy(off).to(dev)
    per_chunk = max(1, p["table_bytes"] // (nx * ny * CELL_BYTES))
    counts, parts, kept, gated = [], [], torch.zeros((), dtype=torch.int64, device=dev), []
    for s0 in range(0, n_s, per_chunk):
        c, part, k, o = _chunk_peaks(pts, off_t, off, s0, min(s0 + per_chunk, n_s), p, dev, ground, sp)
        counts.append(c)
        parts.append(part)
        kept = kept + k
        gated.append(o)
    out = {"peak_offsets": G.exclusive_scan(torch.cat(counts) if counts else torch.zeros((0,), dtype=torch.int32, device=dev))}
    for key, dtype in zip(PEAK_KEYS, (torch.int32, torch.int64, torch.int32, torch.float64, torch.int32)):
        shape = (0, 3) if key == "xyz" else (0,)
        out[key] = torch.cat([part[key] for part in parts]) if parts else torch.empty(shape, dtype=dtype, device=dev)
    n_p = out["iy"].shape[0]
    if n_p >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 peaks in all")
    out["succ"] = torch.empty((n_p,), dtype=torch.int32, device=dev)
    out["pred"] = torch.empty((n_p,), dtype=torch.int32, device=dev)
    L.check(L.lib().prh_trace_link(G.ptr(out["peak_offsets"]), n_s * nx, nx, G.ptr(out["iy"]), G.ptr(out["col"]), n_p,
                                   p["link_cells"], p["gap_slope"], p["max_gap_cols"], G.ptr(out["succ"]),
                                   G.ptr(out["pred"]), dev.index, G.stream(dev)), "prh_trace_link")
    out["bright_points"] = kept
    if ground is not None:
        out["off_surface"] = torch.cat(gated) if gated else torch.zeros((0,), dtype=torch.int64, device=dev)
    return out


# ------------------------------------------------------------------ host side
def chain_lines(xyz, col, succ, pred, n_slices, nx, min_peaks=MIN_PEAKS, min_length=MIN_LENGTH):
    """The host rule of trace_lines, vectorised.  xyz (P,3), col, succ, pred (P,) on the host, peaks in
    (slice, ix, iy) order.  A peak without pred is a head; pointer doubling gives every peak its head
    and its rank in the chain (a link goes to a higher column, so chains are simple and at most nx
    long); chains are ordered by head, which is the order of their heads' (slice, ix, iy); one is
    kept iff it has at least min_peaks peaks and x_last - x_first >= min_length.  Returns (per slice
    the list of (k,3) float64 polylines, the number of chains left out)."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    succ, pred, col = (np.asarray(a, dtype=np.int64) for a in (succ, pred, col))
    n_p = len(succ)
    lines = [[] for _ in range(n_slices)]
    if n_p == 0:
        return lines, 0
    me = np.arange(n_p)
    up = np.where(pred >= 0, pred, me)                           # towards the head
    rank = (pred >= 0).astype(np.int64)
    for _ in range(max(1, int(nx - 1).bit_length())):
        rank = rank + rank[up]
        up = up[up]
    order = np.lexsort((rank, up))                               # by head, then along the chain
    heads, first, length = np.unique(up[order], return_index=True, return_counts=True)
    last = first + length - 1
    x = xyz[order, 0]
    keep = (length >= int(min_peaks)) & (x[last] - x[first] >= float(min_length))
    ordered = xyz[order]
    for h, a, n in zip(heads[keep], first[keep], length[keep]):
        lines[int(col[h]) // nx].append(ordered[a:a + n].copy())
    return lines, int((~keep).sum())


def trace_lines(points, slice_offsets, min_peaks=MIN_PEAKS, min_length=MIN_LENGTH, ground=None, band=BAND,
                ground_cell=GROUND_CELL, **params):
    """Polylines along the paint of every slice ("Paint tracing - the rule").

    points, slice_offsets, ground, band, ground_cell and params: as paint_peaks takes them;
    min_peaks, min_length: the chain filter.  One paint_peaks call, then chain_lines on the host.
    Returns (lines_per_slice: per slice
    the list of (k,3) float64 polylines in that slice's ego frame, ordered by their heads' (ix, iy);
    report {'slices', 'bright_points', 'peaks', 'links', 'lines', 'lines_dropped_short'}: a chain that
    the filter leaves out, a single peak included, is counted in the last; with a ground table the
    report gains 'off_surface_points', the bright points the surface gate left out)."""
    what = "trace_lines"
    min_peaks, min_length = _chain_params(what, min_peaks, min_length)
    nx = _params(what, **params)["nx"]
    peaks = paint_peaks(points, slice_offsets, ground, band, ground_cell, **params)
    n_s = (peaks["peak_offsets"].shape[0] - 1) // nx
    succ = peaks["succ"].cpu().numpy()
    lines, dropped = chain_lines(peaks["xyz"].cpu().numpy(), peaks["col"].cpu().numpy(), succ, peaks["pred"].cpu().numpy(),
                                 n_s, nx, min_peaks, min_length)
    report = {"slices": n_s, "bright_points": int(peaks["bright_points"].item()), "peaks": int(len(succ)),
              "links": int((succ >= 0).sum()), "lines": int(sum(len(ls) for ls in lines)), "lines_dropped_short": dropped}
    if ground is not None:
        report["off_surface_points"] = int(peaks["off_surface"].sum().item())
    return lines, report


@torch.no_grad()
def refine_cloud(model, drive_dir_or_cloud, poses=None, num_line_points=32, num_context_points=1024, crop_radius=0.3,
                 decay_scale=2.0, seed=0, precision=None, segment_len=None, stride=None, radius=None, max_pose_gap=None,
                 min_tube_points=F.MIN_TUBE_POINTS, gate=K.GATE, min_in=K.MIN_IN, out_ratio=K.OUT_RATIO,
                 min_pieces=K.MIN_PIECES, step=F.STEP, min_count=F.MIN_COUNT, max_gap=F.MAX_GAP, origin=None, batched=False,
                 support=False, support_radius=None, device_sync=False, return_links=False, intensity_floor=0.0,
                 half_width=HALF_WIDTH, cell=CELL, col=COL, nms=NMS, link_cells=LINK_CELLS, gap_slope=GAP_SLOPE,
                 max_gap_cols=MAX_GAP_COLS, min_points=MIN_POINTS, min_weight=MIN_WEIGHT, min_peaks=MIN_PEAKS,
                 min_length=MIN_LENGTH, surface=False, surface_band=BAND):
    """A lidar drive refined into one drive-frame lane map, with no detector and no GT.

    drive_dir_or_cloud: a drive directory (merged.pcd and, when poses is None, pose/*.json) or the
    merged cloud itself, (P,4) float32 xyz + intensity (numpy or CUDA tensor); poses: load_poses'
    list, an (S,7) array of x y z qx qy qz qw in file-name order, or None - as fuse.refine_drive
    takes them, and so are segment_len, stride, radius and max_pose_gap.  A chain of the project's
    calls: drive.plan_slices picks the slice poses; drive.slice_cloud cuts every slice's points;
    trace_lines reads the paint of every slice (intensity_floor, half_width, cell, col, nms,
    link_cells, gap_slope, max_gap_cols, min_points, min_weight, min_peaks, min_length; the grid's
    half length is segment_len / 2); fuse.refine_slices runs the model with the traced lines as
    candidates; link.fuse_unmatched links and fuses the pieces (gate, min_in, out_ratio, min_pieces,
    step, min_count, max_gap, origin, device_sync, return_links: link.refine_predictions' arguments
    with its defaults); support=True scores the map against the cloud (fuse.cloud_support with
    support_radius, default crop_radius, and intensity_floor).  intensity_floor="auto" reads the floor
    from the slices themselves (paintfloor.paint_floor, once, before tracing; tracing and support use
    it alike) and the report gains 'floor', 'floor_surface_points', 'floor_paint_share' and
    'floor_contrast'.  surface=True traces the road surface only ("Paint tracing - the rule: surface
    gate"): paintfloor.surface_ground(points, offsets, half_length=segment_len / 2,
    half_width=half_width) is built once, trace_lines gets it with band = surface_band, and with
    intensity_floor="auto" the floor is read over the same window from the same table; the report
    gains 'trace_surface_band' and 'trace_off_surface_points'.  The model's contexts are cut from the
    whole slice either way, as the model was trained.

    Returns link.refine_predictions' dict - 'fused', 'pieces', 'piece_frame', 'piece_slice',
    'pose_index' (plan_slices' indices), 'poses', 'nodes', 'report', with support=True 'support' -
    and 'traced': the traced lines per slice; the report gains 'trace_slices',
    'trace_bright_points', 'trace_peaks', 'trace_links', 'trace_lines', 'trace_lines_dropped_short'
    (with surface=True also 'trace_surface_band', 'trace_off_surface_points')."""
    G.device("trace")
    m = int(num_line_points)
    if not 2 <= m <= F.MAX_POINTS:
        raise ValueError(f"refine_cloud: 2..{F.MAX_POINTS} points per line, got {num_line_points}")
    kw = {k: v for k, v in (("segment_len", segment_len), ("stride", stride), ("max_pose_gap", max_pose_gap)) if v is not None}
    segment_len = D.SEGMENT_LEN if segment_len is None else segment_len
    if isinstance(drive_dir_or_cloud, (str, os.PathLike)):
        if poses is None:
            poses = D.load_poses(os.path.join(drive_dir_or_cloud, "pose"))
        cloud = D.load_merged_cloud(drive_dir_or_cloud).astype(np.float32, copy=False)
    else:
        cloud = drive_dir_or_cloud
    if poses is None:
        raise ValueError("refine_cloud: poses are needed with a cloud")
    chosen = D.plan_slices(poses, **kw)
    if len(poses) and isinstance(poses[0], dict):
        pq = D.poses_xyzq(poses, chosen)
    else:
        pq = np.asarray(poses, dtype=np.float64).reshape(-1, 7)[chosen].reshape(-1, 7)
    trace_kw = dict(half_length=float(segment_len) / 2.0, col=col, half_width=half_width, cell=cell,
                    intensity_floor=intensity_floor, nms=nms, min_points=min_points, min_weight=min_weight,
                    link_cells=link_cells, gap_slope=gap_slope, max_gap_cols=max_gap_cols)
    # a bad parameter raises before the cloud is cut; "auto" is read from the slices below
    _params("refine_cloud", **dict(trace_kw, intensity_floor=0.0 if intensity_floor == "auto" else intensity_floor))
    _chain_params("refine_cloud", min_peaks, min_length)
    if surface:
        _surface_params("refine_cloud", {"half_length": float(segment_len) / 2.0, "half_width": float(half_width)}, surface_band)
    pieces, piece_slice, sparse = np.zeros((0, m, 3)), np.zeros(0, dtype=np.int64), 0
    traced = []
    trace_report = {"slices": 0, "bright_points": 0, "peaks": 0, "links": 0, "lines": 0, "lines_dropped_short": 0}
    if surface:
        trace_report["off_surface_points"] = 0
    if len(chosen):
        points, offsets, _ = D.slice_cloud(cloud, pq, segment_len, D.RADIUS if radius is None else radius)
        off = offsets.cpu().numpy()
        # "auto": read from the slices, once, for tracing and support alike
        if surface:
            # one table for the gate and, with "auto", for the floor: the same window, built once
            window = dict(half_length=float(segment_len) / 2.0, half_width=half_width)
            ground = PF.surface_ground(points, off, **window)
            intensity_floor, floor_report = PF.resolve(intensity_floor, points, off, "refine_cloud", ground, **window)
            trace_kw.update(ground=ground, band=surface_band)
        else:
            intensity_floor, floor_report = PF.resolve(intensity_floor, points, off, "refine_cloud")
        trace_kw["intensity_floor"] = intensity_floor
        traced, trace_report = trace_lines(points, off, min_peaks, min_length, **trace_kw)
        pieces, piece_slice, _, sparse = F.refine_slices(model, points, off, traced, m, num_context_points, crop_radius,
                                                         decay_scale, seed, precision, min_tube_points, batched)
    else:
        intensity_floor, floor_report = PF.resolve(intensity_floor, None, None, "refine_cloud")      # "auto" without a slice raises
    fused, nodes = K.fuse_unmatched(pieces, piece_slice, pq, gate, min_in, out_ratio, min_pieces, step, min_count, max_gap,
                                    origin, return_nodes=True, device_sync=device_sync, return_links=return_links)
    all_clusters = nodes["clusters_all"]
    report = F.refine_report(len(chosen), pieces, sparse, nodes, fused, min_count)
    report.update({"candidates": int(nodes["n_candidates"]), "edges": int(nodes["n_edges"]),
                   "clusters": int(all_clusters.max()) + 1 if len(all_clusters) else 0, "clusters_kept": len(fused),
                   "pieces_unlinked": int((nodes["cluster"] < 0).sum())})
    report.update({"trace_" + k: v for k, v in trace_report.items()})
    if surface:
        report["trace_surface_band"] = float(surface_band)
    if floor_report is not None:
        report.update(PF.report_keys(floor_report))
    res = {"fused": fused, "pieces": pieces, "piece_frame": piece_slice, "piece_slice": piece_slice.copy(),
           "pose_index": [int(c) for c in chosen], "poses": pq, "nodes": nodes, "report": report, "traced": traced}
    if support:
        res["support"] = F.cloud_support(cloud, fused, None, step, crop_radius if support_radius is None else support_radius,
                                         intensity_floor, nodes["origin"])
    return res
