"""Inputs the paint-tracing tests share (test_trace_cpu.py, test_trace_gpu.py and the maker of g21).
A case is {'points' (T,4) float64, 'slice_offsets', 'kw'}: the arguments of paint_peaks / trace_lines.
The designed cases (cells, peaks, nms0, links) are written point by point and go into the fixture; the
seeded ones (compaction, ragged) are generated here and the oracle's result is computed once per
process and never written to.

paint_peaks_np is the second, independent restatement of the rule: dense numpy tables, shifted
comparisons for the peaks and a dense peak-id map for the links, where the oracle walks dicts and
lists.  The analytic frame and the drive are _align_cases' (paint_cloud, paint_frame, paint_drive)."""
import functools

import numpy as np

import _align_cases as AC
import _trace_oracle as O

NAN, INF = float("nan"), float("inf")
FIXTURE_CASES = ("cells", "peaks", "nms0", "links")
KEYS = O.PEAK_KEYS
# exact-binary grids: cell borders are exact in fp64
SMALL = dict(half_length=2.0, col=0.5, half_width=0.5, cell=0.0625)        # nx 8, ny 16
WIDE = dict(half_length=25.0, col=0.5, half_width=2.0, cell=0.0625)       # nx 100, ny 64


def _case(slices, kw):
    slices = [np.asarray(s, dtype=np.float64).reshape(-1, 4) for s in slices]
    pts = np.concatenate(slices) if slices else np.zeros((0, 4))
    return {"points": np.ascontiguousarray(pts), "kw": dict(kw),
            "slice_offsets": np.cumsum([0] + [len(s) for s in slices]).astype(np.int64)}


def at(grid, ix, iy, intensity=50.0, fx=0.5, fy=0.5, z=0.0):
    """A point inside cell (ix, iy) of grid, at the fraction (fx, fy) of the cell."""
    return [-grid["half_length"] + (ix + fx) * grid["col"], -grid["half_width"] + (iy + fy) * grid["cell"], z, intensity]


def cells_case():
    """min_points 1, nms 1 on the 8 x 16 grid: every kept point shows as a peak of its own column.
    Column 0: y exactly at -half_width (cell 0).  1: one ulp below -half_width (dropped); one ulp
    below +half_width, where y + half_width rounds onto the border (dropped: the rule decides on the
    rounded sum), and two ulps below, where the sum is exact (cell 15).  2: y exactly at +half_width
    (dropped) and on the border of cells 6 and 7 (cell 7).  3: x exactly on the border of columns 2
    and 3 (column 3), and x exactly at +half_length (dropped).  4: non-finite x, y, z and I, |z| = 512
    (kept) and one ulp above.  5: qi == 0 (I at the floor, below it, 0.5 / 256 above: rint to even 0)
    and 1.5 / 256 above (qi 2).  6: the weight clamp.  7: x one ulp below +half_length (the sum rounds
    to the border: dropped) and two ulps below (column 7)."""
    g = SMALL
    floor = 8.0
    pts = [[-1.75, -0.5, 0.0, 20.0],
           [-1.25, np.nextafter(-0.5, -INF), 0.0, 20.0], [-1.25, np.nextafter(0.5, -INF), 0.0, 21.0],
           [-1.25, 0.5 - 2.0 ** -53, 0.0, 26.0],
           [-0.75, 0.5, 0.0, 22.0], [-0.75, -0.0625, 0.0, 23.0],
           [-0.5, 0.03125, 0.125, 24.0], [2.0, 0.03125, 0.0, 24.0],
           [NAN, 0.0, 0.0, 30.0], [0.25, INF, 0.0, 30.0], [0.25, 0.0, NAN, 30.0], [0.25, 0.0, -INF, 30.0],
           [0.25, 0.0, 0.0, NAN], [0.25, 0.0, 0.0, INF], [0.25, -0.25, 512.0, 31.0],
           [0.25, 0.25, np.nextafter(512.0, INF), 31.0], [0.25, 0.3125, -512.0, 32.0],
           [0.75, -0.25, 0.0, floor], [0.75, -0.25, 0.0, 3.0], [0.75, -0.25, 0.0, floor + 0.5 / 256.0],
           [0.75, 0.25, 0.0, floor + 1.5 / 256.0],
           [1.25, 0.0, 0.03125, 5000.0], [1.25, 0.0, 0.0625, 9000.0],
           [np.nextafter(2.0, -INF), 0.0, 0.0, 40.0], [2.0 - 2.0 ** -51, 0.25, 0.0, 41.0]]
    return _case([pts], dict(g, intensity_floor=floor, min_points=1, nms=1, min_length=0.5))


def peaks_case():
    """The default nms 4 and min_points 3 on the 8 x 16 grid, one scenario per slice.
    0: two points in one box (min_points - 1): no peak.  1: three points: a peak.  2: a two-cell
    plateau (bright points in cells 7 and 8 only, so b[7] == b[8]; a point with qi == 0 among them is
    not counted): the lower cell wins.  3: points in cell 0 and in cell ny - 1, where nms reaches
    outside the grid (the peaks are cells 0 and ny - 2: with nms >= 1 the strict lower side keeps cell
    ny - 1 from ever being one).  4: two ridges 3 cells apart: nms leaves the stronger; 7 cells apart:
    both.  5: three points spread over cells 5, 6, 7: n3 of cell 6 is 3."""
    g = SMALL
    s0 = [at(g, 1, 6), at(g, 1, 7)]
    s1 = [at(g, 1, 6), at(g, 1, 7), at(g, 1, 7, 30.0)]
    s2 = [at(g, 2, 7, 40.0), at(g, 2, 7, 20.0), at(g, 2, 8, 60.0), at(g, 2, 8, 0.0)]
    s3 = [at(g, 3, 0, 30.0 + k) for k in range(3)] + [at(g, 3, 15, 40.0 + k) for k in range(3)]
    s4 = ([at(g, 4, 4, 30.0)] * 3 + [at(g, 4, 7, 31.0)] * 3 + [at(g, 5, 2, 30.0)] * 3 + [at(g, 5, 9, 29.0)] * 3)
    s5 = [at(g, 6, 5, 10.0), at(g, 6, 6, 10.0), at(g, 6, 7, 10.0)]
    return _case([s0, s1, s2, s3, s4, s5], dict(g, intensity_floor=0.0))


def nms0_case():
    """nms 0 on the 8 x 16 grid: every cell whose box holds min_points points is a peak, cell ny - 1
    included; a single point gives peaks in three cells, at the border in two."""
    g = SMALL
    return _case([[at(g, 1, 15, 30.0), at(g, 1, 15, 31.0), at(g, 2, 0, 32.0), at(g, 2, 0, 33.0), at(g, 3, 8, 34.0),
                   at(g, 3, 8, 35.0), at(g, 4, 5, 36.0)]], dict(g, nms=0, min_points=2))


def links_case():
    """min_points 1, nms 1 on the 100 x 64 grid: single bright points are peaks; one scenario per slice.
    0: a link tie (column 11 holds iy 18 and 22, both 2 from iy 20 in column 10): the smaller iy wins,
    and 22 -> 20 is the non-mutual pair.  1: |diy| == tol (3).  2: |diy| == tol + 1: no link.  3: a gap
    of exactly max_gap_cols + 1 columns: linked.  4: one more: not.  5: a chain of exactly min_length
    (x every 2.5 m, 3 peaks): kept.  6: the last peak 1 / 1024 m nearer: dropped.  7: two peaks only
    (min_peaks - 1).  8: tol grows with the gap: dc 3 allows |diy| 5."""
    g = WIDE
    s0 = [at(g, 10, 20), at(g, 11, 18), at(g, 11, 22), at(g, 12, 18), at(g, 30, 18)]
    s1 = [at(g, 10, 20), at(g, 11, 23), at(g, 22, 23)]
    s2 = [at(g, 10, 20), at(g, 11, 24)]
    s3 = [at(g, 10, 20), at(g, 35, 20), at(g, 36, 21)]
    s4 = [at(g, 10, 20), at(g, 36, 20), at(g, 37, 21)]
    s5 = [at(g, 29, 30), at(g, 34, 31), at(g, 39, 30)]
    s6 = [at(g, 29, 30), at(g, 34, 31), at(g, 39, 30)]
    s6[2][0] -= 1.0 / 1024.0
    s7 = [at(g, 10, 20), at(g, 30, 20)]
    s8 = [at(g, 50, 20), at(g, 53, 25), at(g, 56, 31), at(g, 70, 31)]
    return _case([s0, s1, s2, s3, s4, s5, s6, s7, s8], dict(g, min_points=1, nms=1))


def compaction_case():
    """Columns holding 0, 1, 63, 64, 65 and 257 peaks: ny 2048, nms 1, min_points 1, one bright point
    in every fourth cell (the box spreads it over three cells, the lowest of which is the peak)."""
    rng = np.random.default_rng(210)
    g = dict(half_length=1.5, col=0.5, half_width=12.8, cell=0.0125)
    pts = []
    for ix, n in enumerate((0, 1, 63, 64, 65, 257)):
        first = int(rng.integers(0, 2048 // 4 - n + 1))
        for k in range(n):
            pts.append(at(g, ix, 4 * (first + k) + 1, float(rng.integers(20, 60)), float(rng.uniform(0.1, 0.9)),
                          float(rng.uniform(0.1, 0.9)), float(rng.normal(0.0, 0.02))))
    return _case([pts], dict(g, min_points=1, nms=1))


def ragged_case():
    """Seven slices at the default parameters and floor 20: paint over |x| <= 6; no row at all;
    asphalt only (no bright point); one bright point; paint again; one dim point; paint."""
    rng = np.random.default_rng(211)

    def paint():
        return AC.paint_cloud(rng, -6.0, 6.0, paint_per_m=40.0)

    dim = AC.paint_cloud(rng, -6.0, 6.0, paint_per_m=0.0)
    return _case([paint(), np.zeros((0, 4)), dim, [[1.0, 0.3, 0.0, 55.0]], paint(), [[1.0, 0.3, 0.0, 5.0]], paint()],
                 dict(intensity_floor=20.0))


DESIGNED = {"cells": cells_case, "peaks": peaks_case, "nms0": nms0_case, "links": links_case}
SEEDED = {"compaction": compaction_case, "ragged": ragged_case}


@functools.lru_cache(maxsize=None)
def case(name):
    return dict(DESIGNED, **SEEDED)[name]()


def as_arrays(peaks):
    """The oracle's lists as the arrays paint_peaks returns."""
    return {"peak_offsets": np.array(peaks["peak_offsets"], dtype=np.int64), "iy": np.array(peaks["iy"], dtype=np.int32),
            "weight": np.array(peaks["weight"], dtype=np.int64), "count": np.array(peaks["count"], dtype=np.int32),
            "xyz": np.array(peaks["xyz"], dtype=np.float64).reshape(-1, 3), "col": np.array(peaks["col"], dtype=np.int32),
            "succ": np.array(peaks["succ"], dtype=np.int32), "pred": np.array(peaks["pred"], dtype=np.int32),
            "bright_points": np.int64(peaks["bright_points"])}


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's (peaks as arrays, lines per slice, report) for case(name): computed once per process."""
    c = case(name)
    p = O.params(c["kw"])
    peaks = O.paint_peaks(c["points"], c["slice_offsets"], **c["kw"])
    n_s = len(c["slice_offsets"]) - 1
    lines, dropped = O.chain_lines(peaks, n_s, O.grid_shape(p)[0], p["min_peaks"], p["min_length"])
    lines = [[np.array(l, dtype=np.float64).reshape(-1, 3) for l in ls] for ls in lines]
    return as_arrays(peaks), lines, dropped


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, want, what=""):
    for k in KEYS + ("bright_points",):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g.reshape(-1)), bits(w.reshape(-1))), (what, k)


def same_lines(got, want, what=""):
    assert len(got) == len(want), what
    for s, (gs, ws) in enumerate(zip(got, want)):
        assert len(gs) == len(ws), (what, s, len(gs), len(ws))
        for g, w in zip(gs, ws):
            g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
            assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (what, s)


# ------------------------------------------------------------------ the numpy restatement
def _shift(a, k):
    """a[..., iy + k] with 0 outside the grid."""
    out = np.zeros_like(a)
    if k == 0:
        out[...] = a
    elif 0 < k < a.shape[-1]:
        out[..., :-k] = a[..., k:]
    elif 0 < -k < a.shape[-1]:
        out[..., -k:] = a[..., :k]
    return out


def paint_peaks_np(points, slice_offsets, **kw):
    p = O.params(kw)
    nx, ny = int(np.rint(2.0 * p["half_length"] / p["col"])), int(np.rint(2.0 * p["half_width"] / p["cell"]))
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    off = np.asarray(slice_offsets, dtype=np.int64)
    n_s = len(off) - 1
    sl = np.repeat(np.arange(n_s), np.diff(off))
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((pts[:, 0] + p["half_length"]) / p["col"])
        fy = np.floor((pts[:, 1] + p["half_width"]) / p["cell"])
        wi = np.minimum(np.maximum(pts[:, 3] - float(p["intensity_floor"]), 0.0), 4096.0)
        qi = np.where(np.isfinite(pts[:, 3]), np.rint(np.nan_to_num(wi) * 256.0), 0.0).astype(np.int64)
        keep = (np.isfinite(pts[:, :3]).all(axis=1) & (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny) & (qi > 0)
                & (np.abs(pts[:, 2]) <= 512.0))
    sl, qi, xyz = sl[keep], qi[keep], pts[keep, :3]
    ix, iy = fx[keep].astype(np.int64), fy[keep].astype(np.int64)
    q = np.rint(xyz * 1024.0).astype(np.int64)
    tabs = np.zeros((5, n_s, nx, ny), dtype=np.int64)
    for k, v in enumerate((np.ones_like(qi), qi, qi * q[:, 0], qi * q[:, 1], qi * q[:, 2])):
        np.add.at(tabs[k], (sl, ix, iy), v)
    box = _shift(tabs, -1) + tabs + _shift(tabs, 1)
    n3, b = box[0], box[1]
    peak = (n3 >= int(p["min_points"])) & (b >= int(p["min_weight"]))
    for k in range(1, int(p["nms"]) + 1):
        peak &= (b > _shift(b, -k)) & (b >= _shift(b, k))
    ps, pix, piy = np.nonzero(peak)                              # C order: slice, ix, iy
    n_p = len(ps)
    fb = b[ps, pix, piy].astype(np.float64)
    out = {"peak_offsets": np.concatenate([[0], np.cumsum(peak.sum(axis=2).reshape(-1))]).astype(np.int64),
           "iy": piy.astype(np.int32), "weight": b[ps, pix, piy], "count": n3[ps, pix, piy].astype(np.int32),
           "xyz": np.stack([(box[k][ps, pix, piy].astype(np.float64) / fb) / 1024.0 for k in (2, 3, 4)], 1).reshape(-1, 3),
           "col": (ps * nx + pix).astype(np.int32), "bright_points": np.int64(keep.sum())}
    ident = np.full((n_s, nx, ny), -1, dtype=np.int64)
    ident[ps, pix, piy] = np.arange(n_p)

    def raw(direction):
        res = np.full(n_p, -1, dtype=np.int64)
        open_ = np.ones(n_p, dtype=bool)
        for dc in range(1, int(p["max_gap_cols"]) + 2):
            c = pix + direction * dc
            tol = int(p["link_cells"]) + int(p["gap_slope"]) * (dc - 1)
            for d in [0] + [v for k in range(1, min(tol, ny) + 1) for v in (-k, k)]:     # |d| rising, the smaller iy first
                j = piy + d
                ok = open_ & (c >= 0) & (c < nx) & (j >= 0) & (j < ny)
                hit = np.zeros(n_p, dtype=bool)
                hit[ok] = ident[ps[ok], c[ok], j[ok]] >= 0
                res[hit] = ident[ps[hit], c[hit], j[hit]]
                open_ &= ~hit
        return res

    fwd, back = raw(1), raw(-1)
    me = np.arange(n_p)
    out["succ"] = np.where((fwd >= 0) & (back[np.maximum(fwd, 0)] == me), fwd, -1).astype(np.int32)
    out["pred"] = np.where((back >= 0) & (fwd[np.maximum(back, 0)] == me), back, -1).astype(np.int32)
    return out


# ------------------------------------------------------------------ analytic inputs
def dashed(points, lane=0, period=12.0, on=3.0):
    """points without the bright points of lane `lane` (|y - lane| <= PAINT_HALF in the straight frame)
    outside the dashes (x + 25) mod period < on."""
    y = AC.LANE_Y[lane]
    paint = (np.abs(points[:, 1] - y) <= AC.PAINT_HALF) & (points[:, 3] >= 40.0)
    return points[~paint | (np.mod(points[:, 0] + 25.0, period) < on)]


def turned(points, angle):
    c, s = np.cos(angle), np.sin(angle)
    out = points.copy()
    out[:, 0] = c * points[:, 0] - s * points[:, 1]
    out[:, 1] = s * points[:, 0] + c * points[:, 1]
    return out


def bent(points, curvature):
    out = points.copy()
    out[:, 1] = points[:, 1] + 0.5 * curvature * points[:, 0] * points[:, 0]
    return out


def drive_slices(segment_len=50.0):
    """paint_drive()'s cloud cut per pose on the host: (points (T,4) float64, slice_offsets, poses)."""
    import _fuse_oracle as FO
    cloud, poses, _ = AC.paint_drive()
    slices = []
    for pose in poses:
        ego = FO.to_ego(cloud[:, :3], pose)
        sel = np.abs(ego[:, 0]) <= segment_len / 2.0
        slices.append(np.column_stack([ego[sel], cloud[sel, 3]]))
    return np.concatenate(slices), np.cumsum([0] + [len(s) for s in slices]).astype(np.int64), poses
