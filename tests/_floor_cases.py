"""The designed cases of the paint floor tests (test_floor_cpu.py, test_floor_gpu.py): points with a
ground table given, so the histogram kernel is reached without the ground stage, and hand-made
histogram rows for the threshold kernel.  Expected values come from tests/_floor_oracle.py alone."""
import functools
import math

import numpy as np

import _floor_oracle as O

RUN = 2048                    # the rows one block of prh_floor_hist walks
# an exact-binary grid: cell borders are exact in fp64.  gx 8, gy 4
SMALL = dict(half_length=2.0, half_width=1.0, ground_cell=0.5, band=0.125)
GATE_BINS = (2, 64, 65, 256, 1024)
NAN, INF = float("nan"), float("inf")


def up(v):
    return math.nextafter(v, INF)


def down(v):
    return math.nextafter(v, -INF)


def small_ground():
    """(1,8,4): cell (ix, iy) at 0.25 * ix - 0.5, cell (5, 2) without ground."""
    g = np.repeat((0.25 * np.arange(8.0) - 0.5)[:, None], 4, 1)
    g[5, 2] = NAN
    return g[None]


def at(ix, iy, intensity, dz=0.0, fx=0.5, fy=0.5):
    """A point inside cell (ix, iy) of SMALL at the fraction (fx, fy), dz above that cell's ground."""
    return [-2.0 + (ix + fx) * 0.5, -1.0 + (iy + fy) * 0.5, 0.25 * ix - 0.5 + dz, intensity]


def gates_case(n_bins=64, bin_width=0.5):
    """One slice on the 8 x 4 grid, band 0.125 (exact).  Cells: x exactly on the border of cells 2 and 3
    (cell 3), y exactly at -half_width (cell 0), one ulp below -half_width (dropped), x exactly at
    +half_length (dropped) and one ulp below it, where x + half_length rounds onto the border (dropped: the
    rule decides on the rounded sum) and two ulps below (cell 7), non-finite x and y.  Ground: a point in
    the NaN cell.  Band: |z - g| exactly band on both sides (kept), just beyond on both (dropped; on the
    lower side that takes two ulps of z, because the difference rounds one away), z NaN, +inf and -inf.  Intensity: -0.0 (bin 0), the smallest negative (dropped), NaN, +inf and -inf
    (dropped), n_bins * bin_width exactly, one ulp below it, 1e30 and 1e300 (the last bin), a bin
    border and one ulp below it, and a ladder over every fourth of a bin up to past the last."""
    top = n_bins * bin_width
    g3 = 0.25 * 3 - 0.5
    pts = [at(3, 1, 1.0, fx=0.0), at(2, 0, 1.5, fy=0.0), [0.25, down(-1.0), -0.5 + 0.25 * 4, 2.0],
           [2.0, 0.25, 1.25, 2.5], [down(2.0), 0.25, 1.25, 2.5], [down(down(2.0)), 0.25, 1.25, 3.0],
           [NAN, 0.0, 0.0, 3.0], [0.0, INF, 0.0, 3.0], [-INF, 0.0, 0.0, 3.0],
           at(5, 2, 3.5), at(5, 1, 3.5),
           at(3, 2, 4.0, dz=0.125), at(3, 2, 4.5, dz=-0.125), [-0.25, 0.25, up(g3 + 0.125), 5.0],
           [-0.25, 0.25, down(down(g3 - 0.125)), 5.0], at(3, 2, 5.5, dz=NAN), at(3, 2, 5.5, dz=INF), at(3, 2, 5.5, dz=-INF),
           at(1, 1, -0.0), at(1, 1, -5e-324), at(1, 1, NAN), at(1, 1, INF), at(1, 1, -INF), at(1, 1, top),
           at(1, 1, down(top)), at(1, 1, 1e30), at(1, 1, 1e300), at(1, 1, 3 * bin_width), at(1, 1, down(3 * bin_width))]
    pts += [at(k % 8, (k // 8) % 2, 0.25 * bin_width * k, dz=0.01 * (k % 7 - 3)) for k in range(4 * min(n_bins, 80) + 9)]
    return {"points": np.array(pts, dtype=np.float64), "slice_offsets": np.array([0, len(pts)], dtype=np.int64),
            "ground": small_ground(), "kw": dict(SMALL, n_bins=n_bins, bin_width=bin_width)}


BLOCK_SIZES = (RUN - 8, 1, 0, 7, RUN - 1, RUN, RUN + 1, 3 * RUN + 5)


def blocks_case():
    """Default parameters (gx 50, gy 26: the ceil of 25.6).  Slices of RUN - 8, 1, 0, 7, RUN - 1, RUN, RUN
    + 1 and 3 * RUN + 5 points: the first block holds three slices and the empty one, later blocks
    straddle two, the last slice fills whole blocks; the slice of 7 points lies 1 m above its ground (no
    surface point).  Asphalt at 0-10 and paint at 40-60, a few points outside the window, a tenth of
    the points outside the band, a tenth of the ground cells NaN.  Every value is a float32 value."""
    rng = np.random.default_rng(220)
    gx, gy = O.grid_shape(O.params({}))
    n_s = len(BLOCK_SIZES)
    ground = rng.uniform(-0.5, 0.5, (n_s, gx, gy))
    ground[rng.random((n_s, gx, gy)) < 0.1] = NAN
    slices = []
    for s, n in enumerate(BLOCK_SIZES):
        x, y = rng.uniform(-25.5, 25.5, n), rng.uniform(-13.0, 13.0, n)
        ix = np.clip(np.floor(x + 25.0), 0, gx - 1).astype(int)
        iy = np.clip(np.floor(y + 12.8), 0, gy - 1).astype(int)
        z = np.nan_to_num(ground[s, ix, iy]) + rng.uniform(-0.165, 0.165, n) + (1.0 if n == 7 else 0.0)
        paint = rng.random(n) < 0.3
        slices.append(np.column_stack([x, y, z, np.where(paint, rng.uniform(40.0, 60.0, n), rng.uniform(0.0, 10.0, n))]))
    pts = np.concatenate(slices).astype(np.float32).astype(np.float64)
    return {"points": np.ascontiguousarray(pts), "slice_offsets": np.cumsum((0,) + BLOCK_SIZES).astype(np.int64),
            "ground": ground, "kw": {}}


def contention_case():
    """20,000 points of one intensity on the flat ground of one slice."""
    rng = np.random.default_rng(221)
    n = 20000
    pts = np.column_stack([rng.uniform(-24.0, 24.0, n), rng.uniform(-12.0, 12.0, n), rng.uniform(-0.1, 0.1, n), np.full(n, 7.5)])
    return {"points": pts, "slice_offsets": np.array([0, n], dtype=np.int64), "ground": np.zeros((1, 50, 26)), "kw": {}}


@functools.lru_cache(maxsize=None)
def case(name, *args):
    return {"gates": gates_case, "blocks": blocks_case, "contention": contention_case}[name](*args)


@functools.lru_cache(maxsize=None)
def expected(name, *args):
    """The oracle's histograms of case(name) as (S,n_bins) int64: computed once per process."""
    c = case(name, *args)
    return np.array(O.surface_histograms(c["points"], c["slice_offsets"], c["ground"], **c["kw"]), dtype=np.int64)


# ------------------------------------------------------------------ histogram rows
def row(n, counts):
    h = [0] * n
    for b, c in counts.items():
        h[b] = c
    return h


def uniform_row():
    """U(0,10) / U(40,60): 56 asphalt points per bin 0 .. 9 and 6 paint points per bin 40 .. 59."""
    return row(256, {b: 56 if b < 10 else 6 for b in list(range(10)) + list(range(40, 60))})


# (row, min_points, (t_lo, t_hi, t*)): the rows the issue pins
PINNED = {
    "uniform": (uniform_row(), 16, (10, 40, 25)),
    "three": (row(256, {0: 100, 10: 100, 20: 100}), 16, (1, 20, 10)),
    "mirror": (row(256, {0: 100, 9: 150, 11: 150, 20: 100}), 1, (1, 9, 5)),
}
# rows without a floor: all zero, one bin, min_points one short below and above
NO_FLOOR = {
    "zero": (row(64, {}), 1),
    "one_bin": (row(64, {5: 1000}), 1),
    "short_below": (row(64, {3: 15, 30: 400}), 16),
    "short_above": (row(64, {3: 400, 30: 15}), 16),
}


def random_rows(rng, n_rows, n_bins, top=50):
    """Small two-population rows with gaps, ties and empty stretches."""
    rows = []
    for _ in range(n_rows):
        h = rng.integers(0, top, n_bins)
        h[rng.random(n_bins) < rng.uniform(0.0, 0.9)] = 0
        rows.append([int(c) for c in h])
    return rows


def otsu_arrays(rows, min_points):
    """The oracle's outputs of rows as the arrays otsu_floors returns."""
    res = [O.otsu(h, min_points) for h in rows]
    dtypes = (np.int32,) * 3 + (np.int64,) * 6 + (np.float64,)
    return {k: np.array([r[k] for r in res], dtype=d) for k, d in zip(O.OTSU_KEYS, dtypes)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_otsu(got, want, what=""):
    for k in O.OTSU_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(bits(g), bits(w)), (what, k, g[:8], w[:8])
