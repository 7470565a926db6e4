"""Cloud support: what the merged cloud holds in the tube around every 0.5 m station of every map
polyline - how many points, how bright, on which side, how high - read in one pass over the cloud
(``csrc/prh_support.hpp``; the rule is in ``include/pointnet_refine_hip.h``, "Cloud support - the
rule", and restated in ``tests/_support_oracle.py``).  It scores a map against the lidar where no GT
file labels the drive.

  segment_grid        host: the uniform xy grid of (line, segment) lists the kernel walks (numpy)
  node_support        HIP: the int64 sums per node and the figures derived from them
  map_support         the GT-free counterpart of fuse.map_error: supported share, lateral offset
  marking_attributes  per line solid / dashed / none from the painted nodes

    res = refine_drive(model, drive_dir, None, lines, support=True, intensity_floor=20.0)
    res["support"]["input"]["offset_w_mean"], res["support"]["fused"]["offset_w_mean"]
    write_map_json("map.json", res["fused"], attributes=res["support"]["attributes"])

The GPU functions have no CPU fallback: without a GPU they raise RuntimeError.
"""
import numpy as np
import torch

from . import _gpu as G
from . import _lib as L
from . import fuse as F

STEP = F.STEP                # station spacing in metres
RADIUS = 0.3                 # tube radius in metres: the crop radius of the context builder
MAX_RADIUS = 8.0
CELL = 4.0                   # grid cell in metres: cost only, never the result
MAX_CELLS = 1 << 22          # prh_support_max_cells(): the cell is doubled until the grid fits
GUARD = 1e-6                 # metres added to the radius when boxes are expanded (rounding of the projection)
MAX_NODE_POINTS = 1 << 22    # points per node the int64 sums are bounded for
MIN_POINTS = 5
COLS = 8


# ------------------------------------------------------------------ host side
def segment_grid(lines_shifted, radius, cell=CELL):
    """The grid prh_support_accumulate walks.  lines_shifted: list of (n,3) polylines (origin already
    subtracted).  A uniform xy grid, cell metres wide, over the box of all segments expanded by
    radius (+ GUARD); cell index (floor((x - x0) / cell), floor((y - y0) / cell)) in fp64, the
    kernel's expression.  Per cell the (line, segment) pairs whose expanded box overlaps it, sorted
    by line, then segment; segments of zero length are left out (the rule cannot use them).  cell
    is doubled until the grid has at most MAX_CELLS cells.  Returns {'x0', 'y0', 'cell', 'nx', 'ny',
    'cell_offsets' (nx*ny+1,) int32, 'entries' (E,2) int32}; without a usable segment nx = ny = 0."""
    radius, cell = float(radius), float(cell)
    if not (radius > 0.0 and cell > 0.0 and np.isfinite(cell)):
        raise ValueError("segment_grid: radius and cell must be positive")
    a_all, b_all, sl, sk = [], [], [], []
    for l, v in enumerate(lines_shifted):
        v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
        if not np.isfinite(v).all():
            raise ValueError("segment_grid: line vertices must be finite")
        if len(v) < 2:
            continue
        e = v[1:] - v[:-1]
        k = np.flatnonzero((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] > 0.0)
        a_all.append(v[k])
        b_all.append(v[k + 1])
        sl.append(np.full(len(k), l, dtype=np.int64))
        sk.append(k.astype(np.int64))
    n_seg = sum(len(k) for k in sk)
    if n_seg == 0:
        return {"x0": 0.0, "y0": 0.0, "cell": cell, "nx": 0, "ny": 0, "cell_offsets": np.zeros(1, dtype=np.int32),
                "entries": np.zeros((0, 2), dtype=np.int32)}
    a, b, sl, sk = np.concatenate(a_all), np.concatenate(b_all), np.concatenate(sl), np.concatenate(sk)
    pad = radius + GUARD
    lo = np.minimum(a, b)[:, :2] - pad
    hi = np.maximum(a, b)[:, :2] + pad
    x0, y0 = float(lo[:, 0].min()), float(lo[:, 1].min())
    while True:
        nx = int(np.floor((hi[:, 0].max() - x0) / cell)) + 1
        ny = int(np.floor((hi[:, 1].max() - y0) / cell)) + 1
        if nx * ny <= MAX_CELLS:
            break
        cell *= 2.0
    ix0 = np.floor((lo[:, 0] - x0) / cell).astype(np.int64)
    ix1 = np.floor((hi[:, 0] - x0) / cell).astype(np.int64)
    iy0 = np.floor((lo[:, 1] - y0) / cell).astype(np.int64)
    iy1 = np.floor((hi[:, 1] - y0) / cell).astype(np.int64)
    w = ix1 - ix0 + 1
    count = w * (iy1 - iy0 + 1)
    total = int(count.sum())
    if total >= 2 ** 31:
        raise ValueError(f"segment_grid: {total} cell entries; use a larger cell")
    seg = np.repeat(np.arange(n_seg), count)
    local = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    cell_id = (iy0[seg] + local // w[seg]) * nx + ix0[seg] + local % w[seg]
    order = np.argsort(cell_id, kind="stable")           # segments come line by line, segment by segment
    offsets = G.csr_offsets(np.bincount(cell_id, minlength=nx * ny))
    entries = np.stack([sl[seg[order]], sk[seg[order]]], 1).astype(np.int32)
    return {"x0": x0, "y0": y0, "cell": cell, "nx": nx, "ny": ny, "cell_offsets": offsets.astype(np.int32),
            "entries": np.ascontiguousarray(entries)}


def derive(acc):
    """The per-node figures of an (N,8) int64 acc, fp64: {'n', 'n_paint' int64, 'weight' = [2] / (256
    n), 'offset_w' = [5] / (65536 [2]), 'offset' = [3] / (65536 n), 'spread' = sqrt(max([4] / n -
    ([3] / n)^2, 0)) / 65536, 'z' = [6] / (65536 n)}; NaN where the denominator is 0.  OverflowError
    when a node counts MAX_NODE_POINTS points or more (the bound the int64 sums are safe for)."""
    acc = np.asarray(acc, dtype=np.int64).reshape(-1, COLS)
    n = acc[:, 0]
    if len(n) and int(n.max()) >= MAX_NODE_POINTS:
        raise OverflowError(f"cloud support: a node counts {int(n.max())} points, the sums are bounded for fewer than "
                            f"{MAX_NODE_POINTS}")
    nf = n.astype(np.float64)
    col = acc.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m1 = col[:, 3] / nf
        out = {"n": n.copy(), "n_paint": acc[:, 1].copy(), "weight": col[:, 2] / (256.0 * nf),
               "offset_w": np.where(acc[:, 2] != 0, col[:, 5] / (65536.0 * col[:, 2]), np.nan),
               "offset": col[:, 3] / (65536.0 * nf),
               "spread": np.sqrt(np.maximum(col[:, 4] / nf - m1 * m1, 0.0)) / 65536.0,
               "z": col[:, 6] / (65536.0 * nf)}
    for k in ("weight", "offset", "spread", "z"):
        out[k] = np.where(n > 0, out[k], np.nan)
    return out


def _summary(acc, min_points):
    """map_support's figures over the rows of acc (the sums over nodes are taken in fp64: a column
    is bounded per node, not over a whole map)."""
    n = int(acc[:, 0].sum())
    c2, c3, c4, c5, c6 = (float(np.sum(acc[:, c], dtype=np.float64)) for c in (2, 3, 4, 5, 6))
    supported = int((acc[:, 0] >= int(min_points)).sum())
    nan = float("nan")
    return {"nodes": int(len(acc)), "supported": supported, "supported_share": supported / len(acc) if len(acc) else 0.0,
            "points": n, "offset_mean": c3 / (65536.0 * n) if n else nan,
            "offset_rms": float(np.sqrt(c4 / n)) / 65536.0 if n else nan,
            "offset_w_mean": c5 / (65536.0 * c2) if c2 else nan, "z_mean": c6 / (65536.0 * n) if n else nan}


def _polylines(fused_or_lines):
    """(flat list of polylines, owner line of each, number of lines): an entry is one (n,3) polyline
    or, as in fuse_pieces' fused, a list of them."""
    flat, owner = [], []
    for l, entry in enumerate(fused_or_lines):
        parts = list(entry) if isinstance(entry, (list, tuple)) and (len(entry) == 0 or np.ndim(entry[0]) == 2) else [entry]
        for p in parts:
            flat.append(np.asarray(p, dtype=np.float64).reshape(-1, 3))
            owner.append(l)
    return flat, np.asarray(owner, dtype=np.int64), len(fused_or_lines)


def _runs(mask):
    """Lengths of the runs of True in a boolean vector and of the False gaps between two runs."""
    m = np.concatenate(([False], np.asarray(mask, dtype=bool), [False]))
    edge = np.flatnonzero(m[1:] != m[:-1])
    start, end = edge[0::2], edge[1::2]
    return end - start, start[1:] - end[:-1]


def marking_attributes(support, min_points=MIN_POINTS, min_paint_points=3, solid_share=0.8, dashed_share=0.15):
    """The marking type of every line from its painted nodes.  support: map_support's result (its
    polylines grouped by line) or node_support's (every polyline a line).  A node is supported if n
    >= min_points and painted if also n_paint >= min_paint_points.  Per line {'supported_share'
    (supported nodes over nodes), 'painted_share' (painted over supported nodes, nan without one),
    'runs' (runs of consecutive painted nodes; a run ends with its polyline), 'mean_run_m',
    'mean_gap_m' (unpainted stretches between two runs of one polyline; nan without one), 'marking':
    'solid' at painted_share >= solid_share, 'dashed' at dashed_share <= painted_share < solid_share
    with at least 2 runs, 'none' below dashed_share, else 'unknown'}."""
    if "acc" in support:
        node, owner = support, np.arange(len(support["offsets"]) - 1)
        n_lines = len(owner)
    else:
        node, owner, n_lines = support["support"], support["polyline_line"], support["lines"]
    step, off = float(node["step"]), node["offsets"]
    n, n_paint = node["acc"][:, 0], node["acc"][:, 1]
    out = []
    for l in range(n_lines):
        nodes = sup = painted = 0
        runs, gaps = [], []
        for p in np.flatnonzero(owner == l):
            ok = n[off[p]:off[p + 1]] >= int(min_points)
            paint = ok & (n_paint[off[p]:off[p + 1]] >= int(min_paint_points))
            r, g = _runs(paint)
            runs += list(r)
            gaps += list(g)
            nodes += len(ok)
            sup += int(ok.sum())
            painted += int(paint.sum())
        share = painted / sup if sup else float("nan")
        if share >= solid_share:
            marking = "solid"
        elif share >= dashed_share:
            marking = "dashed" if len(runs) >= 2 else "unknown"
        elif share < dashed_share:
            marking = "none"
        else:
            marking = "unknown"
        out.append({"supported_share": sup / nodes if nodes else 0.0, "painted_share": share, "runs": len(runs),
                    "mean_run_m": float(np.mean(runs)) * step if runs else float("nan"),
                    "mean_gap_m": float(np.mean(gaps)) * step if gaps else float("nan"), "marking": marking})
    return out


# ------------------------------------------------------------------ GPU side
def _cloud(cloud, dev, what):
    """(T,4) float32 CUDA, 16-byte aligned: numpy is uploaded once, a CUDA tensor stays where it is."""
    if not torch.is_tensor(cloud):
        cloud = np.asarray(cloud)
        if cloud.ndim != 2 or cloud.shape[1] != 4:
            raise ValueError(f"{what}: cloud must be (T,4) x y z intensity, got {cloud.shape}")
    elif cloud.dim() != 2 or cloud.shape[1] != 4:
        raise ValueError(f"{what}: cloud must be (T,4) x y z intensity, got {tuple(cloud.shape)}")
    t = G.as_cuda(cloud, dev, what, torch.float32)
    if t.shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 points")
    return t.clone() if t.numel() and t.data_ptr() % 16 else t


def node_support(cloud, lines, step=STEP, radius=RADIUS, intensity_floor=0.0, origin=None, cell=CELL):
    """What the cloud holds around every station of every line ("Cloud support - the rule").

    cloud (T,4) float32 x y z intensity in the drive frame, numpy (uploaded once) or a CUDA tensor
    (used where it is); lines: list of (n,3) polylines.  Line l has the nodes 0 .. floor(length /
    step); a point within radius of a line counts for the node nearest to its projection, for every
    line it is near.  origin (default: the first vertex of the first line with one, rounded down to
    1000 m) is subtracted from lines and points.  cell is the grid's cell in metres: cost only.
    Returns {'acc' (N,8) int64: count, painted count (weight > 0), sum of weights * 256, of lateral
    offsets * 65536, of their squares, of weight * offset, of heights * 65536, 0; 'offsets'
    (n_lines+1,), 'origin', 'step', 'radius', 'intensity_floor'} and derive()'s per-node arrays 'n',
    'n_paint', 'weight', 'offset_w', 'offset', 'spread', 'z'.  Bitwise reproducible, whatever the
    order of the points."""
    step, radius, intensity_floor = float(step), float(radius), float(intensity_floor)
    if not step > 0.0:
        raise ValueError("node_support: step must be positive")
    if not 0.0 < radius <= MAX_RADIUS:
        raise ValueError(f"node_support: 0 < radius <= {MAX_RADIUS}")
    if not np.isfinite(intensity_floor):
        raise ValueError("node_support: intensity_floor must be finite")
    dev = G.device("support", cloud.device if torch.is_tensor(cloud) and cloud.is_cuda else None)
    arrs = [np.asarray(l, dtype=np.float64).reshape(-1, 3) for l in lines]
    first = next((a[0] for a in arrs if len(a)), np.zeros(3))
    org = F.floor_km(first) if origin is None else np.asarray(origin, dtype=np.float64).reshape(3)
    shifted, cums = F._lines(arrs, org)
    node_off = F.node_offsets(cums, step)
    n_nodes = int(node_off[-1])
    pts = _cloud(cloud, dev, "node_support")
    acc = torch.zeros((n_nodes, COLS), dtype=torch.int64, device=dev)
    if pts.shape[0] and n_nodes:
        grid = segment_grid(shifted, radius, cell)
        if len(grid["entries"]):
            lib = L.lib()
            verts, off_t, _ = G.lines_csr(shifted, dev)
            cum_t = torch.from_numpy(np.concatenate(cums)).to(dev)
            no_t = torch.from_numpy(node_off).to(dev)
            co_t = torch.from_numpy(grid["cell_offsets"]).to(dev)
            en_t = torch.from_numpy(grid["entries"]).to(dev)
            L.check(lib.prh_support_accumulate(
                G.ptr(pts), pts.shape[0], float(org[0]), float(org[1]), float(org[2]), grid["x0"], grid["y0"],
                grid["cell"], grid["nx"], grid["ny"], G.ptr(co_t), G.ptr(en_t), len(grid["entries"]), G.ptr(verts),
                G.ptr(off_t), G.ptr(cum_t), len(arrs), G.ptr(no_t), n_nodes, step, radius * radius, intensity_floor,
                G.ptr(acc), dev.index, G.stream(dev)), "prh_support_accumulate")
    acc_h = acc.cpu().numpy()
    out = {"acc": acc_h, "offsets": node_off, "origin": org, "step": step, "radius": radius,
           "intensity_floor": intensity_floor}
    out.update(derive(acc_h))
    return out


def map_support(cloud, fused_or_lines, min_points=MIN_POINTS, step=STEP, radius=RADIUS, intensity_floor=0.0,
                origin=None, cell=CELL, per_line=False):
    """How much lidar evidence a map has under it: the GT-free counterpart of fuse.map_error.

    fused_or_lines: per line one (n,3) polyline or, as fuse_pieces returns, a list of polylines;
    every polyline is scored as its own polyline (node_support) and the sums are added per line.
    Returns {'nodes', 'supported' (nodes with n >= min_points), 'supported_share', 'points' (hits),
    'offset_mean', 'offset_rms' (lateral offset of the hits, metres, left positive), 'offset_w_mean'
    (the same weighted by intensity above the floor: where the paint lies), 'z_mean'; nan without a
    hit}, with per_line=True also 'per_line': the same per line; and what marking_attributes needs:
    'support' (node_support's dict over the polylines), 'polyline_line', 'lines'."""
    flat, owner, n_lines = _polylines(fused_or_lines)
    node = node_support(cloud, flat, step, radius, intensity_floor, origin, cell)
    acc, off = node["acc"], node["offsets"]
    out = _summary(acc, min_points)
    out.update(support=node, polyline_line=owner, lines=n_lines)
    if per_line:
        rows = [np.concatenate([acc[off[p]:off[p + 1]] for p in np.flatnonzero(owner == l)] + [acc[:0]])
                for l in range(n_lines)]
        out["per_line"] = [_summary(r, min_points) for r in rows]
    return out
