"""Paint alignment: the xy shift that puts the detector's lines on the paint, read from the cloud.

The detector's lines reach the ego frame through a camera-lidar extrinsic and a nearest-pose match
(``predictions.match_poses``), so a few tenths of a metre of systematic offset are normal; the
context builder's tube is 0.3 m wide, and beyond it the model refines against bare asphalt.
``metrics.calibrate_alignment`` finds such a shift only against GT.  This module finds it from the
frame's own slice of the cloud: for every (slice, shift) of a brute-force grid the sum, over (bright
point, line) pairs, of the point's intensity weight times a taper of its distance to the shifted
line, in integers (``csrc/prh_align.hpp``; the rule is in ``include/pointnet_refine_hip.h``, "Paint
alignment - the rule", and restated in ``tests/_align_oracle.py``).  It is the xy twin of
``ground.lift_lines`` and plugs into the same places.

  shift_grid       host: one grid of shifts around a centre, x outer, y inner (numpy)
  segment_bitmaps  host: per slice the cells a reach-expanded segment box touches (numpy)
  paint_scores     HIP: candidate filter (count, scan, write), then the score sweep: per (slice,
                   shift) the int64 score and hit count
  pick_shift       host: the shortest shift among the near-best rows, the min_points and gain tests
  align_lines      a coarse and a fine paint_scores call with their picks: x y of every vertex moved
                   by its slice's (or the drive's) shift

    shifted, report = align_lines(points, offsets, [[pixel_to_ego(px) for px in frame] for frame in frames])

The rigid twin ("Rigid paint alignment - the rule") sweeps poses (dx, dy, theta): a yaw about a
per-slice pivot - the sensor - plus the shift, for the heading error a shift cannot take out.

  pose_grid        host: shift_grid crossed with a grid of yaws, the yaw index outer (numpy)
  pose_table       host: (K,3) dx dy theta -> (K,4) dx dy cos sin, the bits the device and the oracle get
  rigid_reach      host: per slice the reach of a pose table (conservative; cost only)
  rigid_scores     HIP: the candidate filter in cell or arrival order, then prh_align_score_rigid
  pick_pose        host: pick_shift with the norm dx^2 + dy^2 + (lever theta)^2
  apply_pose       host: a pose applied to (n,3) vertices
  align_lines_rigid  the coarse and the fine rigid_scores call with their picks
  align            align_lines at max_yaw = 0, align_lines_rigid above it

Both kinds of table go down one path (prepare, select_candidates, score_candidates, _scores, _stage,
_two_stage, _pick): a shift table is (K,2) and takes prh_align_score after the arrival-order filter,
a pose table is (K,3) and takes prh_align_score_rigid after the filter in ORDER.

paint_scores, rigid_scores, align_lines and align_lines_rigid have no CPU fallback: without a GPU
they raise RuntimeError.
"""
import math

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L

RADIUS = 0.15                # metres: the tube around a shifted line
MAX_RADIUS = 1.0
GUARD = 1e-6                 # metres added to the reach (rounding of d2)
MAX_COORD = 1e6              # |vertex coordinate| the guard is sized for
MAX_SHIFT = 4.0              # |shift component|
MAX_SHIFTS = 4096            # prh_align_max_shifts(): rows of one slice's table
CELL = 1.0                   # metres: the bitmap's cell
MAX_CELLS = 1 << 26          # the cell is doubled until all bitmaps together fit: cost only, never the result
MIN_POINTS = 32
KEEP = (63, 64)
GAIN = (5, 4)
COARSE_HALF, COARSE_STEP = 1.0, 0.1
FINE_HALF, FINE_STEP = 0.1, 0.02
CANDIDATES, SHIFTS = 256, 16     # a work item of prh_align_score
MAX_YAW = 0.1                # |theta| of a pose row, radians
MAX_POSES = 32768            # prh_align_max_poses(): rows of one slice's pose table
LEVER = 25.0                 # metres: the half length of a slice; what a radian of yaw moves a line end by
COARSE_YAW, COARSE_YAW_STEP = 0.02, 0.004
FINE_YAW_HALF, FINE_YAW_STEP = 0.004, 0.001
ORDER = "cell"               # rigid_scores' default candidate order (DESIGN.md 4u has the measurement)


# ------------------------------------------------------------------ host side
def shift_grid(centre=(0.0, 0.0), half=COARSE_HALF, step=COARSE_STEP):
    """((2n+1)^2, 2) float64: centre + j * step for j = -n .. n with n = round(half / step), x outer
    and y inner (metrics._grid's order)."""
    half, step = float(half), float(step)
    if not (step > 0.0 and np.isfinite(step) and half >= 0.0 and np.isfinite(half)):
        raise ValueError("shift_grid: step > 0 and half >= 0")
    n = int(round(half / step))
    j = np.arange(-n, n + 1, dtype=np.float64) * step
    xs, ys = float(centre[0]) + j, float(centre[1]) + j
    return np.stack([np.repeat(xs, len(ys)), np.tile(ys, len(xs))], axis=1).astype(np.float64).reshape(-1, 2)


def lines_csr(lines_per_slice, what="paint_scores"):
    """The lines of every slice as CSR: (vertices (V,3) float64, line_offsets (L+1,) int64,
    slice_line_offsets (S+1,) int64).  A vertex must be finite and within MAX_COORD of the origin."""
    flat = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for ls in lines_per_slice for v in ls]
    per_slice = np.array([len(ls) for ls in lines_per_slice], dtype=np.int64)
    sl_off = G.csr_offsets(per_slice)
    l_off = G.csr_offsets([len(v) for v in flat])
    verts = np.ascontiguousarray(np.concatenate(flat)) if l_off[-1] > 0 else np.zeros((0, 3))
    if not (np.isfinite(verts).all() and (len(verts) == 0 or np.abs(verts).max() <= MAX_COORD)):
        raise ValueError(f"{what}: line vertices must be finite and within {MAX_COORD:g} m of the slice's origin")
    return verts, l_off, sl_off


def slice_reach(shifts, shift_offsets, radius):
    """(S,) float64: radius + max_k max(|dx|, |dy|) + GUARD over every slice's own table (a slice
    without a shift: radius + GUARD)."""
    sh = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    off = np.asarray(shift_offsets, dtype=np.int64).reshape(-1)
    big = np.zeros(len(off) - 1)
    used = np.flatnonzero(np.diff(off) > 0)
    if len(used):
        big[used] = np.maximum.reduceat(np.abs(sh).max(axis=1), off[:-1][used])
    return float(radius) + big + GUARD


def segment_bitmaps(vertices, line_offsets, slice_line_offsets, reach, cell=CELL):
    """The bitmaps prh_align_select_* look a point up in ("Paint alignment - the rule").  Per slice
    a uniform xy grid, cell metres wide, over the box of its vertices expanded by reach[s]; cell
    index floor((x - x0) / cell) in fp64, the kernels' expression.  A cell is set when the xy box of
    a segment (two consecutive vertices of one line), expanded by reach[s], touches it.  cell is
    doubled until all grids together have at most MAX_CELLS cells.  Returns {'origin' (S,2)
    float64, 'shape' (S,2) int32 = nx ny (0 0 for a slice without a vertex), 'cell_base' (S,)
    int64, 'n_cells', 'cell', 'bitmap' (ceil(n_cells / 32),) uint32: cell c is bit c & 31 of word
    c >> 5}."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    l_off = np.asarray(line_offsets, dtype=np.int64).reshape(-1)
    sl_off = np.asarray(slice_line_offsets, dtype=np.int64).reshape(-1)
    reach = np.asarray(reach, dtype=np.float64).reshape(-1)
    v_off = l_off[sl_off]                                   # the vertices of every slice
    maps = G.box_grids(v[:, :2], v_off, reach, cell, MAX_CELLS)
    origin, shape, base, n_cells, cell = (maps[k] for k in ("origin", "shape", "cell_base", "n_cells", "cell"))
    shape = shape.astype(np.int64)
    bits = np.zeros(n_cells, dtype=bool)
    # segments: vertex k and k + 1 of one line
    is_a = np.ones(len(v), dtype=bool)
    is_a[l_off[1:][l_off[1:] > 0] - 1] = False               # a line's last vertex starts no segment
    a = np.flatnonzero(is_a)
    if len(a):
        s_of = np.searchsorted(v_off, a, side="right") - 1
        r = reach[s_of]
        lo = np.minimum(v[a, :2], v[a + 1, :2]) - r[:, None]
        hi = np.maximum(v[a, :2], v[a + 1, :2]) + r[:, None]
        i0 = np.floor((lo - origin[s_of]) / cell).astype(np.int64)
        i1 = np.floor((hi - origin[s_of]) / cell).astype(np.int64)
        i0 = np.maximum(i0, 0)
        i1 = np.minimum(i1, shape[s_of] - 1)
        nxy = np.maximum(i1 - i0 + 1, 0)
        cnt = nxy[:, 0] * nxy[:, 1]
        seg = np.repeat(np.arange(len(a)), cnt)
        k = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        ix = i0[seg, 0] + k % np.maximum(nxy[seg, 0], 1)
        iy = i0[seg, 1] + k // np.maximum(nxy[seg, 0], 1)
        bits[base[s_of[seg]] + iy * shape[s_of[seg], 0] + ix] = True
    packed = np.packbits(bits, bitorder="little")
    words = np.zeros(((n_cells + 31) // 32) * 4, dtype=np.uint8)
    words[:len(packed)] = packed
    return dict(maps, bitmap=words.view("<u4").astype(np.uint32))


def _ratio(pair, what, name, allow_above_one):
    try:
        num, den = pair
        ok = int(num) == num and int(den) == den and int(num) >= 1 and int(den) >= 1
        ok = ok and (allow_above_one or int(num) <= int(den)) and max(int(num), int(den)) <= 65536
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: {name} = (num, den), positive integers up to 65536")
    return int(num), int(den)


def _pick(what, rows, score, hits, norm2, key, zero, min_points, keep, gain, check=None):
    """Steps 6-10 of either rule over one table: pick_shift and pick_pose.  rows (K,cols) float64; norm2: the
    squared length of rows[near], by which the near-best rows are ranked; key: 'shift' or 'pose', the result's key
    and the word of the error texts; zero: how those name the all-zero row; check: the caller's own validation, in
    its place after the shared ones."""
    sc = [int(x) for x in np.asarray(score).reshape(-1)]
    ht = [int(x) for x in np.asarray(hits).reshape(-1)]
    if not (len(rows) == len(sc) == len(ht)):
        raise ValueError(f"{what}: one score and one hit count per {key}")
    keep_num, keep_den = _ratio(keep, what, "keep", False)
    gain_num, gain_den = _ratio(gain, what, "gain", True)
    if int(min_points) != min_points or int(min_points) < 1:
        raise ValueError(f"{what}: min_points must be an integer >= 1")
    if check is not None:
        check()
    zeros = np.flatnonzero((rows == 0.0).all(axis=1))
    if len(zeros) == 0:
        raise ValueError(f"{what}: the table must contain the {key} {zero}")
    k0 = int(zeros[0])
    none = {key: np.zeros(rows.shape[1]), "row": k0, "aligned": False, "score_zero": sc[k0], "score_best": sc[k0]}
    best = max(sc)
    if best == 0 or ht[sc.index(best)] < int(min_points):
        return none
    near = [k for k in range(len(sc)) if sc[k] * keep_den >= best * keep_num]
    row = near[int(np.argmin(norm2(rows[near])))]            # argmin: the first of equal values, the lowest row
    none["score_best"] = sc[row]
    if not sc[row] * gain_den > sc[k0] * gain_num:
        return none
    return {key: rows[row].copy(), "row": row, "aligned": True, "score_zero": sc[k0], "score_best": sc[row]}


def pick_shift(shifts, score, hits, min_points=MIN_POINTS, keep=KEEP, gain=GAIN):
    """Steps 6-10 of the rule over one table.  shifts (K,2) float64, score and hits (K,) integers.
    Returns {'shift' (2,) float64, 'row' (the accepted row, or k0), 'aligned' bool, 'score_zero',
    'score_best' (Python ints: the score at (0, 0) and at the near-best row)}."""
    sh = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    return _pick("pick_shift", sh, score, hits, lambda r: r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1], "shift", "(0, 0)",
                 min_points, keep, gain)


def work_items(cand_offsets, shift_offsets, slice_vertices):
    """The plan of prh_align_score: (W,3) int64 = (slice, first candidate row, first shift row), one
    item per (slice, tile of CANDIDATES candidates, tile of SHIFTS shifts), the candidate tile
    running fastest; slices without a candidate, a shift or a vertex have none."""
    c_off = np.asarray(cand_offsets, dtype=np.int64)
    k_off = np.asarray(shift_offsets, dtype=np.int64)
    nc, nk = np.diff(c_off), np.diff(k_off)
    nct, nkt = (nc + CANDIDATES - 1) // CANDIDATES, (nk + SHIFTS - 1) // SHIFTS
    per = np.where(np.asarray(slice_vertices) > 0, nct * nkt, 0)
    s = np.repeat(np.arange(len(nc), dtype=np.int64), per)
    r = np.arange(int(per.sum()), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)
    div = np.maximum(nct[s], 1)
    return np.ascontiguousarray(np.stack([s, c_off[s] + (r % div) * CANDIDATES, k_off[s] + (r // div) * SHIFTS], 1))


# ------------------------------------------------------------------ GPU side
def _params(radius, intensity_floor, cell, what):
    radius, intensity_floor, cell = float(radius), float(intensity_floor), float(cell)
    if not 0.0 < radius <= MAX_RADIUS:
        raise ValueError(f"{what}: 0 < radius <= {MAX_RADIUS}")
    if not np.isfinite(intensity_floor):
        raise ValueError(f"{what}: intensity_floor must be finite")
    if not (np.isfinite(cell) and cell > 0.0):
        raise ValueError(f"{what}: cell must be positive and finite")
    return radius, intensity_floor, cell


def prepare(points, slice_offsets, lines_per_slice, table, table_offsets, radius, intensity_floor, cell, what, pivots=None,
            rigid=False):
    """Validation and the host side of one paint_scores or (rigid) rigid_scores call: the points on the device, the
    lines as CSR, every slice's reach and bitmap.  table: (K,2) shifts dx dy, or with rigid (K,3) poses dx dy theta
    and pivots (S,2) or None.  Returns the dict select_candidates and score_candidates take; 'sh' is the table the
    device gets, for poses pose_table's (K,4)."""
    name, cols, names, max_rows = ("poses", 3, "dx dy theta", MAX_POSES) if rigid else ("shifts", 2, "dx dy", MAX_SHIFTS)
    radius, intensity_floor, cell = _params(radius, intensity_floor, cell, what)
    dev = G.device("align", points.device if torch.is_tensor(points) and points.is_cuda else None)
    pts = G.points4(points, dev, what)
    off = G.offsets(slice_offsets, pts.shape[0], what, "slice_offsets")
    n_s = len(off) - 1
    if len(lines_per_slice) != n_s:
        raise ValueError(f"{what}: one list of lines per slice ({n_s}), got {len(lines_per_slice)}")
    verts, l_off, sl_off = lines_csr(lines_per_slice, what)
    shape = tuple(table.shape) if torch.is_tensor(table) else np.shape(table)
    if len(shape) != 2 or shape[1] != cols:
        raise ValueError(f"{what}: {name} must be (K,{cols}) {names}, got {shape}")
    tb = np.ascontiguousarray(G.host(table, np.float64).reshape(-1, cols))
    if not (np.isfinite(tb).all() and (len(tb) == 0 or (np.abs(tb[:, :2]).max() <= MAX_SHIFT
                                                        and (not rigid or np.abs(tb[:, 2]).max() <= MAX_YAW)))):
        limits = f"|dx|, |dy| <= {MAX_SHIFT:g} and |theta| <= {MAX_YAW:g}" if rigid else f"|component| <= {MAX_SHIFT:g}"
        raise ValueError(f"{what}: {name} must be finite with {limits}")
    k_off = G.offsets(table_offsets, len(tb), what, name[:-1] + "_offsets")
    if len(k_off) != len(off):
        raise ValueError(f"{what}: slice_offsets and {name[:-1]}_offsets must describe the same slices")
    if n_s and int(np.diff(k_off).max()) > max_rows:
        raise ValueError(f"{what}: at most {max_rows} {name} per slice")
    pv = _pivots(pivots, n_s, what) if rigid else None
    reach = rigid_reach(tb, k_off, radius, verts, l_off, sl_off, pv) if rigid else slice_reach(tb, k_off, radius)
    maps = segment_bitmaps(verts, l_off, sl_off, reach, cell)
    return {"dev": dev, "pts": pts, "off": off, "n_s": n_s, "verts": verts, "l_off": l_off, "sl_off": sl_off,
            "sh": pose_table(tb) if rigid else tb, "k_off": k_off, "reach": reach, "maps": maps, "radius": radius,
            "pivots": pv, "rigid": rigid, "intensity_floor": intensity_floor, "what": what}


def select_candidates(p, order="arrival"):
    """The candidate filter - count, the scan, write: (records (C,4) float64 CUDA - x y z and the bits of qi -,
    cand_offsets (S+1,) int64 CUDA, the same offsets as numpy).  order 'arrival': prh_align_select_*, one counter per
    slice, a slice's records as they arrive; 'cell': prh_align_select_cells_*, one counter per bitmap cell, a slice's
    records in ascending cell order (arrival order inside a cell)."""
    lib, dev, pts, maps, n_s = L.lib(), p["dev"], p["pts"], p["maps"], p["n_s"]
    n_cells = maps["n_cells"]
    if n_s == 0 or pts.shape[0] == 0 or n_cells == 0:
        return torch.empty((0, 4), dtype=torch.float64, device=dev), None, np.zeros(n_s + 1, dtype=np.int64)
    entry, n = ("prh_align_select_cells", n_cells) if order == "cell" else ("prh_align_select", n_s)
    counts = torch.zeros((n,), dtype=torch.int32, device=dev)
    off_t = torch.from_numpy(p["off"]).to(dev)
    g_t = tuple(torch.from_numpy(np.ascontiguousarray(maps[k])).to(dev) for k in ("origin", "shape", "cell_base"))
    bitmap = torch.from_numpy(maps["bitmap"].view(np.int32)).to(dev)
    args = (G.ptr(pts), 1 if pts.dtype == torch.float64 else 0, G.ptr(off_t), n_s, pts.shape[0], G.ptr(g_t[0]), G.ptr(g_t[1]),
            G.ptr(g_t[2]), G.ptr(bitmap), n_cells, maps["cell"], p["intensity_floor"])
    L.check(getattr(lib, entry + "_count")(*args, G.ptr(counts), dev.index, G.stream(dev)), entry + "_count")
    scan = G.exclusive_scan(counts)
    # cells of a slice are contiguous from cell_base[s]: the slice's rows start at the scan there
    cand_off = torch.cat([scan[g_t[2]], scan[-1:]]).contiguous() if order == "cell" else scan
    c_off = cand_off.cpu().numpy()
    total = int(c_off[-1])
    rec = torch.empty((total, 4), dtype=torch.float64, device=dev)
    if total:
        nb = getattr(lib, entry + "_workspace_bytes")(n)
        ws = G.workspace(nb, dev)
        L.check(getattr(lib, entry + "_write")(*args, G.ptr(scan), G.ptr(rec), total, G.ptr(ws), nb, dev.index, G.stream(dev)),
                entry + "_write")
    return rec, cand_off, c_off


def score_candidates(p, rec, cand_off, c_off):
    """The plan and the score sweep over the selected candidates - prh_align_score for a shift p,
    prh_align_score_rigid for a rigid one: acc (K,2) int64 CUDA = score, hits."""
    dev, table, rigid = p["dev"], p["sh"], p["rigid"]
    acc = torch.zeros((len(table), 2), dtype=torch.int64, device=dev)
    if p["n_s"] and int((np.diff(c_off) * np.diff(p["sl_off"])).max()) >= 2 ** 31:
        raise OverflowError(f"{p['what']}: a slice has 2^31 or more (candidate, line) pairs")
    items = work_items(c_off, p["k_off"], np.diff(p["l_off"][p["sl_off"]]))
    if rec.shape[0] == 0 or len(items) == 0:
        return acc
    up = [torch.from_numpy(np.ascontiguousarray(x)).to(dev)
          for x in (p["verts"], p["l_off"], p["sl_off"], table, p["k_off"], p["reach"], items) + ((p["pivots"],) if rigid else ())]
    verts, l_off, sl_off, tb, k_off, reach, plan, *pv = (G.ptr(t) for t in up)
    entry = "prh_align_score_rigid" if rigid else "prh_align_score"
    L.check(getattr(L.lib(), entry)(G.ptr(rec), G.ptr(cand_off), rec.shape[0], verts, len(p["verts"]), l_off, len(p["l_off"]) - 1,
                                    sl_off, tb, k_off, len(table), *pv, reach, p["n_s"], plan, len(items),
                                    p["radius"] * p["radius"], G.ptr(acc), dev.index, G.stream(dev)), entry)
    return acc


def _scores(points, slice_offsets, lines_per_slice, table, table_offsets, radius, intensity_floor, cell, what, pivots=None,
            rigid=False, order="arrival"):
    if order not in ("cell", "arrival"):
        raise ValueError(f"{what}: order must be 'cell' or 'arrival'")
    p = prepare(points, slice_offsets, lines_per_slice, table, table_offsets, radius, intensity_floor, cell, what, pivots, rigid)
    rec, cand_off, c_off = select_candidates(p, order)
    acc = score_candidates(p, rec, cand_off, c_off)
    return {"score": acc[:, 0], "hits": acc[:, 1], "candidates": np.diff(c_off)}


def paint_scores(points, slice_offsets, lines_per_slice, shifts, shift_offsets, radius=RADIUS, intensity_floor=0.0,
                 cell=CELL):
    """The paint score of every (slice, shift) ("Paint alignment - the rule", steps 1-5).

    points (T,4) float64 or float32 x y z intensity, every slice in its own frame, with slice_offsets
    (S+1,) - what drive.slice_cloud returns (CUDA tensors are used where they are, numpy is
    uploaded); lines_per_slice: per slice the list of (n,3) polylines in that slice's frame; shifts
    (K,2) float64 dx dy grouped by slice with shift_offsets (S+1,).  A point weighs rint(256 *
    clamp(I - intensity_floor, 0, 4096)); a (point, line) pair within radius of each other once the
    line is moved by the shift adds weight * rint(1024 * (1 - d2 / radius^2)) to the shift's score
    and 1 to its hits.  cell is the width of the filter's bitmap cells: cost only.  Returns a dict of
    CUDA tensors 'score' (K,) int64 and 'hits' (K,) int64.  Bitwise reproducible, whatever the order
    of the points."""
    res = _scores(points, slice_offsets, lines_per_slice, shifts, shift_offsets, radius, intensity_floor, cell,
                  "paint_scores")
    return {"score": res["score"], "hits": res["hits"]}


def _stage(points, off, lines, tables, scope, radius, intensity_floor, pick, what, **scores_kw):
    """One _scores call over per-slice tables and the picks - pick(table, score, hits): per slice under scope
    'frame', once on the summed tables under scope 'drive' (every slice's table is then the same)."""
    n_s = len(lines)
    if n_s == 0:
        return [], np.zeros(0, dtype=np.int64)
    k_off = G.csr_offsets([len(t) for t in tables])
    res = _scores(points, off, lines, np.concatenate(tables), k_off, radius, intensity_floor, CELL, what, **scores_kw)
    score, hits = res["score"].cpu().numpy(), res["hits"].cpu().numpy()
    if scope == "drive":
        k = len(tables[0])
        one = pick(tables[0], [int(x) for x in score.reshape(n_s, k).astype(object).sum(axis=0)],
                   [int(x) for x in hits.reshape(n_s, k).astype(object).sum(axis=0)])
        picks = [one] * n_s
    else:
        picks = [pick(tables[s], score[k_off[s]:k_off[s + 1]], hits[k_off[s]:k_off[s + 1]]) for s in range(n_s)]
    return picks, res["candidates"]


def _two_stage(what, points, off, lines, scope, radius, intensity_floor, coarse, fine, pick, key, columns, **scores_kw):
    """What align_lines and align_lines_rigid share: the coarse table for every slice and its picks, the table
    fine(coarse pick) per slice and the final picks.  key: 'shift' or 'pose'; columns(rows): the report's entries
    for the picked rows (S,cols).  Returns (the picked rows, the report)."""
    n_s = len(lines)
    first, _ = _stage(points, off, lines, [coarse] * n_s, scope, radius, intensity_floor, pick, what, **scores_kw)
    picks, cands = _stage(points, off, lines, [fine(p[key]) for p in first], scope, radius, intensity_floor, pick, what,
                          **scores_kw)
    rows = np.array([p[key] for p in picks], dtype=np.float64).reshape(n_s, coarse.shape[1])
    aligned = int(sum(1 for p in picks if p["aligned"]))
    report = {"frames": n_s, "frames_aligned": aligned, "frames_unaligned": n_s - aligned, **columns(rows),
              "score_zero": np.array([p["score_zero"] for p in picks], dtype=np.int64),
              "score_best": np.array([p["score_best"] for p in picks], dtype=np.int64),
              "candidates": int(np.sum(cands))}
    return rows, report


def _own_lines(lines_per_slice):
    return [[np.array(v, dtype=np.float64).reshape(-1, 3) for v in ls] for ls in lines_per_slice]


def align_lines(points, slice_offsets, lines_per_slice, max_shift=COARSE_HALF, radius=RADIUS, intensity_floor=0.0,
                scope="frame", min_points=MIN_POINTS, keep=KEEP, gain=GAIN):
    """Put every line on the paint of its own slice.

    points, slice_offsets: as paint_scores takes them; lines_per_slice: per slice the list of (n,3)
    polylines in that slice's frame.  A coarse paint_scores call over shift_grid((0, 0), max_shift,
    0.1) and its picks, a fine one over shift_grid(coarse pick, 0.1, 0.02) with the row (0, 0)
    appended, and the final picks over the fine tables (pick_shift: min_points, keep, gain).
    scope='frame' picks per slice; scope='drive' adds the slices' tables up and picks once, in both
    stages, so every slice gets the same shift.  x and y of every vertex move by the slice's shift;
    z never changes.  Returns (the shifted (n,3) float64 lines in the same nesting, report
    {'frames', 'frames_aligned', 'frames_unaligned', 'shifts' (S,2) float64, 'score_zero' and
    'score_best' (S,) int64: the final table's score at (0, 0) and at the near-best row (the summed
    table's under scope='drive'), 'candidates': the points the final sweep kept})."""
    what = "align_lines"
    G.device("align")
    if scope not in ("frame", "drive"):
        raise ValueError(f"{what}: scope must be 'frame' or 'drive'")
    max_shift = float(max_shift)
    if not (np.isfinite(max_shift) and 0.0 < max_shift <= MAX_SHIFT - FINE_HALF):
        raise ValueError(f"{what}: 0 < max_shift <= {MAX_SHIFT - FINE_HALF}")
    coarse = shift_grid((0.0, 0.0), max_shift, COARSE_STEP)
    if len(coarse) > MAX_SHIFTS:
        raise ValueError(f"{what}: max_shift gives {len(coarse)} coarse shifts, at most {MAX_SHIFTS}")
    pick_kw = {"min_points": min_points, "keep": keep, "gain": gain}
    pick_shift(np.zeros((1, 2)), [0], [0], **pick_kw)         # validates min_points, keep and gain
    lines = _own_lines(lines_per_slice)
    off = G.host(slice_offsets, np.int64).reshape(-1)
    shifts, report = _two_stage(
        what, points, off, lines, scope, radius, intensity_floor, coarse,
        lambda c: np.concatenate([shift_grid(c, FINE_HALF, FINE_STEP), np.zeros((1, 2))]),
        lambda t, sc, ht: pick_shift(t, sc, ht, **pick_kw), "shift", lambda rows: {"shifts": rows})
    for s, ls in enumerate(lines):
        for v in ls:
            v[:, 0] = v[:, 0] + shifts[s, 0]
            v[:, 1] = v[:, 1] + shifts[s, 1]
    return lines, report


# ------------------------------------------------------------------ rigid: host side
def pose_grid(centre=(0.0, 0.0), half=COARSE_HALF, step=COARSE_STEP, yaw_centre=0.0, yaw_half=COARSE_YAW,
              yaw_step=COARSE_YAW_STEP):
    """((2m+1) (2n+1)^2, 3) float64 dx dy theta: shift_grid(centre, half, step) under every yaw
    yaw_centre + j * yaw_step, j = -m .. m with m = round(yaw_half / yaw_step); the yaw index runs
    outer.  yaw_half = 0 gives the one yaw yaw_centre."""
    yaw_centre, yaw_half, yaw_step = float(yaw_centre), float(yaw_half), float(yaw_step)
    if not (yaw_step > 0.0 and np.isfinite(yaw_step) and yaw_half >= 0.0 and np.isfinite(yaw_half)
            and np.isfinite(yaw_centre)):
        raise ValueError("pose_grid: yaw_step > 0 and yaw_half >= 0")
    sh = shift_grid(centre, half, step)
    m = int(round(yaw_half / yaw_step))
    th = yaw_centre + np.arange(-m, m + 1, dtype=np.float64) * yaw_step
    return np.concatenate([np.tile(sh, (len(th), 1)), np.repeat(th, len(sh))[:, None]], axis=1)


def pose_table(poses):
    """(K,3) dx dy theta -> (K,4) float64 dx dy cos(theta) sin(theta): the table the device and the
    oracle take.  math.cos and math.sin, once per distinct theta."""
    ps = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    uniq, inv = np.unique(np.ascontiguousarray(ps[:, 2]).view(np.int64), return_inverse=True)   # as bits: -0.0 is not 0.0
    cs = np.array([[math.cos(float(v)), math.sin(float(v))] for v in uniq.view(np.float64)], dtype=np.float64).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([ps[:, :2], cs[inv.reshape(-1)]], axis=1))


def _pivots(pivots, n_s, what):
    if pivots is None:
        return np.zeros((n_s, 2))
    shape = tuple(pivots.shape) if torch.is_tensor(pivots) else np.shape(pivots)
    if shape != (n_s, 2):
        raise ValueError(f"{what}: pivots must be ({n_s},2) x y, one per slice, got {shape}")
    pv = np.ascontiguousarray(G.host(pivots, np.float64).reshape(n_s, 2))
    if not (np.isfinite(pv).all() and (n_s == 0 or np.abs(pv).max() <= MAX_COORD)):
        raise ValueError(f"{what}: pivots must be finite and within {MAX_COORD:g} m of the slice's origin")
    return pv


def rigid_reach(poses, pose_offsets, radius, vertices, line_offsets, slice_line_offsets, pivots):
    """(S,) float64: ((radius + m) + a * (rho + radius)) + GUARD per slice, m = max_k max(|dx|, |dy|)
    and a = max_k |theta| over the slice's own rows of poses (K,3), rho the largest xy distance of a
    vertex of the slice from its pivot ("Rigid paint alignment - the rule", Reach).  With a = 0 these
    are slice_reach's bits."""
    ps = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    off = np.asarray(pose_offsets, dtype=np.int64).reshape(-1)
    n_s = len(off) - 1
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    pv = np.asarray(pivots, dtype=np.float64).reshape(n_s, 2)
    v_off = np.asarray(line_offsets, dtype=np.int64)[np.asarray(slice_line_offsets, dtype=np.int64)]
    big, yaw, rho = np.zeros(n_s), np.zeros(n_s), np.zeros(n_s)
    used = np.flatnonzero(np.diff(off) > 0)
    if len(used):
        big[used] = np.maximum.reduceat(np.abs(ps[:, :2]).max(axis=1), off[:-1][used])
        yaw[used] = np.maximum.reduceat(np.abs(ps[:, 2]), off[:-1][used])
    used = np.flatnonzero(np.diff(v_off) > 0)
    if len(used):
        g = v[:, :2] - np.repeat(pv, np.diff(v_off), axis=0)
        rho[used] = np.maximum.reduceat(np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]), v_off[:-1][used])
    return ((float(radius) + big) + yaw * (rho + float(radius))) + GUARD


def pick_pose(poses, score, hits, lever=LEVER, min_points=MIN_POINTS, keep=KEEP, gain=GAIN):
    """Steps 6'-10 of the rigid rule over one table.  poses (K,3) float64 dx dy theta, score and hits
    (K,) integers.  Returns {'pose' (3,) float64, 'row' (the accepted row, or k0), 'aligned' bool,
    'score_zero', 'score_best' (Python ints: the score at (0, 0, 0) and at the near-best row)}."""
    ps = np.asarray(poses, dtype=np.float64).reshape(-1, 3)

    def check():
        if not (np.isfinite(float(lever)) and float(lever) > 0.0):
            raise ValueError("pick_pose: lever must be positive and finite")

    def norm2(r):
        lt = float(lever) * r[:, 2]
        return r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + lt * lt
    return _pick("pick_pose", ps, score, hits, norm2, "pose", "(0, 0, 0)", min_points, keep, gain, check)


def apply_pose(vertices, pose, pivot=(0.0, 0.0)):
    """(n,3) float64: the vertices under the pose (dx, dy, theta) about pivot - x' = ((c gx - s gy) +
    px) + dx, y' = ((s gx + c gy) + py) + dy with g = vertex - pivot, z untouched.  A new array."""
    v = np.array(vertices, dtype=np.float64).reshape(-1, 3)
    dx, dy, th = (float(x) for x in pose)
    c, s = math.cos(th), math.sin(th)
    px, py = float(pivot[0]), float(pivot[1])
    gx, gy = v[:, 0] - px, v[:, 1] - py
    x = ((c * gx - s * gy) + px) + dx
    y = ((s * gx + c * gy) + py) + dy
    v[:, 0], v[:, 1] = x, y
    return v


# ------------------------------------------------------------------ rigid: GPU side
def rigid_scores(points, slice_offsets, lines_per_slice, poses, pose_offsets, pivots=None, radius=RADIUS,
                 intensity_floor=0.0, cell=CELL, order=ORDER):
    """The paint score of every (slice, pose) ("Rigid paint alignment - the rule", steps 1-5).

    points, slice_offsets, lines_per_slice, radius, intensity_floor, cell: as paint_scores takes
    them.  poses (K,3) float64 dx dy theta grouped by slice with pose_offsets (S+1,): |dx|, |dy| <= 4,
    |theta| <= 0.1 rad, at most MAX_POSES rows per slice.  A pose moves a line vertex p to R(theta)(p
    - pivot) + pivot + (dx, dy); pivots (S,2), one per slice, default (0, 0).  The cosine and sine go
    to the device as pose_table computes them.  order: 'cell' hands the score kernel each slice's
    candidates sorted by bitmap cell, 'arrival' in the order of the per-slice filter - cost
    only, the tables are bitwise equal.  Returns a dict of CUDA tensors 'score' (K,) int64 and 'hits'
    (K,) int64.  A table whose thetas are all 0, with the default pivots, gives paint_scores'
    integers."""
    res = _scores(points, slice_offsets, lines_per_slice, poses, pose_offsets, radius, intensity_floor, cell, "rigid_scores",
                  pivots, True, order)
    return {"score": res["score"], "hits": res["hits"]}


def align_lines_rigid(points, slice_offsets, lines_per_slice, max_shift=COARSE_HALF, max_yaw=COARSE_YAW, lever=LEVER,
                      radius=RADIUS, intensity_floor=0.0, scope="frame", min_points=MIN_POINTS, keep=KEEP, gain=GAIN,
                      pivots=None):
    """Put every line on the paint of its own slice by a yaw about the slice's pivot and a shift.

    align_lines with pose tables.  Coarse: pose_grid((0, 0), max_shift, 0.1, 0, max_yaw, 0.004) (441 x
    11 rows at the defaults); fine: pose_grid(coarse shift, 0.1, 0.02, coarse theta, 0.004, 0.001)
    with the row (0, 0, 0) appended; the picks are pick_pose's (lever, min_points, keep, gain).
    max_yaw = 0 leaves the one yaw 0 in both stages: the result is then align_lines', bit for bit.
    pivots (S,2): the point of every slice's frame the yaw turns about, default (0, 0), the sensor.
    x and y of every vertex move by apply_pose; z never changes.  Returns (the moved (n,3) float64
    lines in the same nesting, report: align_lines' keys plus 'yaws' (S,) float64)."""
    what = "align_lines_rigid"
    G.device("align")
    if scope not in ("frame", "drive"):
        raise ValueError(f"{what}: scope must be 'frame' or 'drive'")
    max_shift, max_yaw = float(max_shift), float(max_yaw)
    if not (np.isfinite(max_shift) and 0.0 < max_shift <= MAX_SHIFT - FINE_HALF):
        raise ValueError(f"{what}: 0 < max_shift <= {MAX_SHIFT - FINE_HALF}")
    if not (np.isfinite(max_yaw) and 0.0 <= max_yaw <= MAX_YAW - FINE_YAW_HALF):
        raise ValueError(f"{what}: 0 <= max_yaw <= {MAX_YAW - FINE_YAW_HALF}")
    coarse = pose_grid((0.0, 0.0), max_shift, COARSE_STEP, 0.0, max_yaw, COARSE_YAW_STEP)
    if len(coarse) > MAX_POSES:
        raise ValueError(f"{what}: max_shift and max_yaw give {len(coarse)} coarse poses, at most {MAX_POSES}")
    pick_kw = {"min_points": min_points, "keep": keep, "gain": gain}
    pick_pose(np.zeros((1, 3)), [0], [0], lever, **pick_kw)   # validates lever, min_points, keep and gain
    lines = _own_lines(lines_per_slice)
    off = G.host(slice_offsets, np.int64).reshape(-1)
    pv = _pivots(pivots, len(lines), what)
    fine_yaw = FINE_YAW_HALF if max_yaw > 0.0 else 0.0
    poses, report = _two_stage(
        what, points, off, lines, scope, radius, intensity_floor, coarse,
        lambda c: np.concatenate([pose_grid(c[:2], FINE_HALF, FINE_STEP, c[2], fine_yaw, FINE_YAW_STEP), np.zeros((1, 3))]),
        lambda t, sc, ht: pick_pose(t, sc, ht, lever, **pick_kw), "pose",
        lambda rows: {"shifts": np.ascontiguousarray(rows[:, :2]), "yaws": np.ascontiguousarray(rows[:, 2])},
        pivots=pv, rigid=True, order=ORDER)
    return [[apply_pose(v, poses[s], pv[s]) for v in ls] for s, ls in enumerate(lines)], report


def align(points, slice_offsets, lines_per_slice, max_yaw=0.0, **kw):
    """align_lines(points, slice_offsets, lines_per_slice, **kw) at max_yaw = 0, align_lines_rigid(..., max_yaw=max_yaw,
    **kw) above it: the shift path and its kernels run untouched unless a yaw is asked for."""
    if float(max_yaw) > 0.0:
        return align_lines_rigid(points, slice_offsets, lines_per_slice, max_yaw=max_yaw, **kw)
    return align_lines(points, slice_offsets, lines_per_slice, **kw)
