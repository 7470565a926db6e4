"""Ground lift: the height of the road surface under the detector's lines, read from the cloud.

``predictions.pixel_to_ego`` gives the detector's BEV pixels z = 0, as the reference does; the
context builder's tube is 3-D and 0.3 m wide, so wherever the road is not within 0.3 m of z = 0 in
the ego frame (a pose origin at sensor height, a degree of pitch, a slope) the tube is empty and the
line is dropped.  The slices ``drive.slice_cloud`` returns already hold the answer: a robust "height
of the road under this xy" for every station of every line of every frame, found in one ragged pass
(``csrc/prh_ground.hpp``; the rule is in ``include/pointnet_refine_hip.h``, "Ground lift - the rule",
and restated in ``tests/_ground_oracle.py``).

  line_stations    host: stations every `step` metres of xy arc length along every line (numpy)
  slice_grids      host: the uniform xy cell grid of every slice, laid over its queries (numpy)
  ground_heights   HIP: per query the road height, the points it rests on, all hits, the mode's bin
  lift_lines       line_stations + one ground_heights call + the host rule: z of every vertex
                   interpolated between the stations that found ground

    lifted, report = lift_lines(points, offsets, [[pixel_to_ego(px) for px in frame] for frame in frames])

ground_heights and lift_lines have no CPU fallback: without a GPU they raise RuntimeError.
"""
import numpy as np
import torch

from . import _gpu as G
from . import _lib as L

RADIUS = 0.5                 # metres around a station, in xy
MAX_RADIUS = 4.0
GUARD = 1e-6                 # metres added to the radius where cells are chosen (rounding of d2)
MAX_COORD = 1e6              # |query coordinate| the guard is sized for
Z_LO, BIN, N_BINS = -8.0, 0.0625, 256
MAX_BINS = 256               # prh_ground_max_bins()
Z_LIMIT = 256.0              # the histogram lies inside [-Z_LIMIT, Z_LIMIT]: the int64 sums are bounded for it
MIN_POINTS = 5
PEAK_SHARE = (1, 2)
MAX_PEAK_DEN = 65536
MAX_CELLS = 1 << 26          # the cell is doubled until all grids together fit: cost only, never the result
STEP = 1.0                   # station spacing in metres


# ------------------------------------------------------------------ host side
def line_stations(lines, step=STEP):
    """Stations along every line.  lines: list of (n,3) or (n,2) polylines.  Per line, cum is the xy
    arc length over its vertices; the stations lie at s_j = j * step for j = 0 .. floor(total /
    step), plus total itself if it is not already the last; a line of one vertex or of zero xy length
    has the single station at its first vertex, a line without a vertex has none.  Returns (xy (N,2)
    float64: np.interp over cum per coordinate, arc (N,) float64, offsets (L+1,) int64: line l owns
    stations offsets[l] .. offsets[l+1])."""
    step = float(step)
    if not (step > 0.0 and np.isfinite(step)):
        raise ValueError("line_stations: step must be positive")
    xy, arc, counts = [], [], []
    for l, v in enumerate(lines):
        v = np.asarray(v, dtype=np.float64)
        v = v.reshape(-1, v.shape[-1] if v.ndim == 2 and v.shape[-1] in (2, 3) else 3)
        if not np.isfinite(v[:, :2]).all():
            raise ValueError(f"line_stations: line {l} has a non-finite x or y")
        if len(v) == 0:
            counts.append(0)
            continue
        cum = vertex_arcs(v)
        total = float(cum[-1])
        if not total > 0.0:
            s = np.zeros(1)
            pxy = v[:1, :2].copy()
        else:
            s = np.arange(int(np.floor(total / step)) + 1, dtype=np.float64) * step
            if s[-1] != total:
                s = np.append(s, total)
            pxy = np.stack([np.interp(s, cum, v[:, 0]), np.interp(s, cum, v[:, 1])], 1)
        xy.append(pxy)
        arc.append(s)
        counts.append(len(s))
    off = G.csr_offsets(counts)
    if off[-1] == 0:
        return np.zeros((0, 2)), np.zeros(0), off
    return np.concatenate(xy), np.concatenate(arc), off


def vertex_arcs(v):
    """(n,) float64: the xy arc length from the first vertex to every vertex of one polyline."""
    v = np.asarray(v, dtype=np.float64)
    cum = np.zeros(len(v))
    if len(v) > 1:
        d = v[1:, :2] - v[:-1, :2]
        cum[1:] = np.cumsum(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
    return cum


def slice_grids(queries, query_offsets, radius, cell):
    """The grids prh_ground_bin_* and prh_ground_query walk ("Ground lift - the rule").  queries (Q,2)
    float64 and query_offsets (S+1,) on the host.  Per slice a uniform xy grid, cell metres wide,
    over the box of its queries expanded by reach = radius + GUARD; cell index floor((x - x0) /
    cell) in fp64, the kernels' expression.  cell is doubled until all grids together have at most
    MAX_CELLS cells.  Returns {'origin' (S,2) float64, 'shape' (S,2) int32 = nx ny (0 0 for a slice
    without a query), 'cell_base' (S,) int64, 'n_cells', 'cell', 'reach'}."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 2)
    qoff = np.asarray(query_offsets, dtype=np.int64).reshape(-1)
    reach = float(radius) + GUARD
    return dict(G.box_grids(q, qoff, reach, cell, MAX_CELLS), reach=reach)


def _params(radius, min_points, peak_share, z_lo, bin, n_bins, what):
    radius, z_lo, bin = float(radius), float(z_lo), float(bin)
    if not 0.0 < radius <= MAX_RADIUS:
        raise ValueError(f"{what}: 0 < radius <= {MAX_RADIUS}")
    if int(n_bins) != n_bins or not 1 <= int(n_bins) <= MAX_BINS:
        raise ValueError(f"{what}: 1 <= n_bins <= {MAX_BINS}")
    if not (bin > 0.0 and np.isfinite(bin) and z_lo >= -Z_LIMIT and z_lo + int(n_bins) * bin <= Z_LIMIT):
        raise ValueError(f"{what}: bin > 0 and the histogram [z_lo, z_lo + n_bins * bin) inside [-{Z_LIMIT}, {Z_LIMIT}]")
    if int(min_points) != min_points or int(min_points) < 1:
        raise ValueError(f"{what}: min_points must be an integer >= 1")
    try:
        num, den = peak_share
        ok = int(num) == num and int(den) == den and 1 <= int(num) <= int(den) <= MAX_PEAK_DEN
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: peak_share = (num, den), integers with 1 <= num <= den <= {MAX_PEAK_DEN}")
    return radius, int(min_points), int(num), int(den), z_lo, bin, int(n_bins)


# ------------------------------------------------------------------ GPU side
def bin_points(pts, off_t, grids, dev):
    """prh_ground_bin_count, the scan, prh_ground_bin_write: (cell_offsets (n_cells+1,) int64 CUDA,
    rows (R,) int32 CUDA, the device copies of the grid arrays)."""
    lib = L.lib()
    n_s, n_cells = len(grids["cell_base"]), grids["n_cells"]
    is_double = 1 if pts.dtype == torch.float64 else 0
    g_t = tuple(torch.from_numpy(np.ascontiguousarray(grids[k])).to(dev) for k in ("origin", "shape", "cell_base"))
    counts = torch.zeros((n_cells,), dtype=torch.int32, device=dev)
    args = (G.ptr(pts), is_double, G.ptr(off_t), n_s, pts.shape[0], G.ptr(g_t[0]), G.ptr(g_t[1]), G.ptr(g_t[2]), n_cells,
            grids["cell"])
    L.check(lib.prh_ground_bin_count(*args, G.ptr(counts), dev.index, G.stream(dev)), "prh_ground_bin_count")
    cell_off = G.exclusive_scan(counts)
    total = int(cell_off[-1].item())
    rows = torch.empty((total,), dtype=torch.int32, device=dev)
    if total:
        nb = lib.prh_ground_bin_workspace_bytes(n_cells)
        ws = G.workspace(nb, dev)
        L.check(lib.prh_ground_bin_write(*args, G.ptr(cell_off), G.ptr(rows), total, G.ptr(ws), nb, dev.index, G.stream(dev)),
                "prh_ground_bin_write")
    return cell_off, rows, g_t


def query_heights(pts, off_t, q_t, qoff_t, grids, g_t, cell_off, rows, params, dev):
    """prh_ground_query over binned points: the dict ground_heights returns."""
    radius, min_points, num, den, z_lo, bin, n_bins = params
    n_q = q_t.shape[0]
    out = {"height": torch.empty((n_q,), dtype=torch.float64, device=dev),
           "count": torch.empty((n_q,), dtype=torch.int32, device=dev),
           "hits": torch.empty((n_q,), dtype=torch.int32, device=dev),
           "bin": torch.empty((n_q,), dtype=torch.int32, device=dev)}
    if n_q:
        L.check(L.lib().prh_ground_query(
            G.ptr(pts), 1 if pts.dtype == torch.float64 else 0, G.ptr(off_t), len(grids["cell_base"]), pts.shape[0],
            G.ptr(q_t), G.ptr(qoff_t), n_q, G.ptr(g_t[0]), G.ptr(g_t[1]), G.ptr(g_t[2]), grids["n_cells"], grids["cell"],
            G.ptr(cell_off), G.ptr(rows), rows.shape[0], radius * radius, grids["reach"], z_lo, bin, n_bins, min_points,
            num, den, G.ptr(out["height"]), G.ptr(out["count"]), G.ptr(out["hits"]), G.ptr(out["bin"]), dev.index,
            G.stream(dev)), "prh_ground_query")
    return out


def ground_heights(points, slice_offsets, queries, query_offsets, radius=RADIUS, min_points=MIN_POINTS,
                   peak_share=PEAK_SHARE, z_lo=Z_LO, bin=BIN, n_bins=N_BINS, cell=None):
    """The road height under every query ("Ground lift - the rule").

    points (T,4) float64 or float32 x y z intensity, every slice in its own frame, with slice_offsets
    (S+1,) - what drive.slice_cloud returns (CUDA tensors are used where they are, numpy is
    uploaded); queries (Q,2) float64 xy grouped by slice with query_offsets (S+1,).  A query sees the
    points of its slice within radius in xy; their heights are binned (n_bins bins of `bin` metres
    from z_lo), and the lowest mode that holds at least peak_share = (num, den) of the strongest
    three-bin window - and min_points points - is the ground.  cell (default: radius) is the width
    of the grid the points are sorted into, >= radius: cost only.  Returns a dict of CUDA tensors
    'height' (Q,) float64 (NaN: no ground), 'count' (Q,) int32 the points the height is the mean
    of, 'hits' (Q,) int32 all points within radius, 'bin' (Q,) int32 the mode's bin (-1: none).
    Bitwise reproducible, whatever the order of the points."""
    what = "ground_heights"
    params = _params(radius, min_points, peak_share, z_lo, bin, n_bins, what)
    radius = params[0]
    cell = radius if cell is None else float(cell)
    if not (np.isfinite(cell) and cell >= radius):
        raise ValueError(f"{what}: cell must be finite and >= radius")
    dev = G.device("ground", points.device if torch.is_tensor(points) and points.is_cuda else None)
    pts = G.points4(points, dev, what)
    off = G.offsets(slice_offsets, pts.shape[0], what, "slice_offsets")
    if len(off) > 1 and int(np.diff(off).max()) >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 points per slice")
    shape = tuple(queries.shape) if torch.is_tensor(queries) else np.shape(queries)
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"{what}: queries must be (Q,2) x y, got {shape}")
    q = np.ascontiguousarray(G.host(queries, np.float64).reshape(-1, 2))
    if not (np.isfinite(q).all() and (len(q) == 0 or np.abs(q).max() <= MAX_COORD)):
        raise ValueError(f"{what}: queries must be finite and within {MAX_COORD:g} m of the slice's origin")
    qoff = G.offsets(query_offsets, len(q), what, "query_offsets")
    if len(qoff) != len(off):
        raise ValueError(f"{what}: slice_offsets and query_offsets must describe the same slices")
    grids = slice_grids(q, qoff, radius, cell)
    off_t = torch.from_numpy(off).to(dev)
    cell_off, rows, g_t = bin_points(pts, off_t, grids, dev)
    return query_heights(pts, off_t, torch.from_numpy(q).to(dev), torch.from_numpy(qoff).to(dev), grids, g_t, cell_off,
                         rows, params, dev)


def lift_vertices(lines, station_arc, station_offsets, height):
    """The host rule of lift_lines.  Per line, over its stations with a finite height, z(vertex) =
    np.interp(vertex arc, s[valid], h[valid]) - np.interp holds the end values outside the range; a
    line with no valid station is returned unchanged.  x and y are never changed.  Returns (list of
    (n,3) float64, lifted (L,) bool)."""
    out, lifted = [], np.zeros(len(lines), dtype=bool)
    for l, v in enumerate(lines):
        v = np.array(v, dtype=np.float64).reshape(-1, 3)
        s = station_arc[station_offsets[l]:station_offsets[l + 1]]
        h = height[station_offsets[l]:station_offsets[l + 1]]
        ok = np.isfinite(h)
        if len(v) and ok.any():
            v[:, 2] = np.interp(vertex_arcs(v), s[ok], h[ok])
            lifted[l] = True
        out.append(v)
    return out, lifted


def lift_lines(points, slice_offsets, lines_per_slice, step=STEP, **ground_kw):
    """Put every line on the road of its own slice.

    points, slice_offsets: as ground_heights takes them; lines_per_slice: per slice the list of (n,3)
    polylines in that slice's frame (the detector's lines have z = 0; whatever z they carry is
    replaced).  One line_stations call, one ground_heights call for all slices (ground_kw: its
    radius, min_points, peak_share, z_lo, bin, n_bins, cell), then lift_vertices.  Returns (the
    lifted (n,3) float64 lines in the same nesting, report {'lines', 'lines_lifted',
    'lines_unlifted', 'stations', 'stations_without_ground'}); a line with no station that found
    ground is returned unchanged and counted in 'lines_unlifted'."""
    G.device("ground")
    flat = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for ls in lines_per_slice for v in ls]
    xy, arc, s_off = line_stations(flat, step)
    per_slice = np.array([len(ls) for ls in lines_per_slice], dtype=np.int64)
    l_off = G.csr_offsets(per_slice)
    res = ground_heights(points, slice_offsets, xy, s_off[l_off], **ground_kw)
    height = res["height"].cpu().numpy()
    out, lifted = lift_vertices(flat, arc, s_off, height)
    report = {"lines": len(flat), "lines_lifted": int(lifted.sum()), "lines_unlifted": int((~lifted).sum()),
              "stations": int(len(arc)), "stations_without_ground": int((~np.isfinite(height)).sum())}
    return [out[l_off[s]:l_off[s + 1]] for s in range(len(per_slice))], report
