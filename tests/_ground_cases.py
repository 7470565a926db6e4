"""Inputs the ground-lift tests share (test_ground_cpu.py, test_ground_gpu.py and the maker of g18).
A case is {'points' (T,4) float64, 'slice_offsets', 'queries' (Q,2), 'query_offsets', 'kw'}: the
arguments of ground_heights.  The designed cases (hits, bins, params, cells) are written point by
point and go into the fixture; the seeded ones (queries, ragged, road, slabs) are generated here and
the oracle's result is computed once per process and never written to.

In the designed cases every cluster sits around its own query, and the queries are far enough apart
that a cluster is seen by its query alone."""
import functools

import numpy as np

import _ground_oracle as O

RADIUS, Z_LO, BIN, N_BINS, MIN_POINTS = 0.5, -8.0, 0.0625, 256, 5
GUARD = 1e-6
FIXTURE_CASES = ("hits", "bins", "params", "cells")
KEYS = ("height", "count", "hits", "bin")


def _ring(q, n, z, r=0.25):
    """n points on a circle of radius r around q (exact sixteenths where n allows), heights z (scalar or list)."""
    a = 2.0 * np.pi * (np.arange(n) + 0.25) / n
    x = q[0] + np.round(r * np.cos(a) * 64.0) / 64.0
    y = q[1] + np.round(r * np.sin(a) * 64.0) / 64.0
    return np.column_stack([x, y, np.broadcast_to(np.asarray(z, dtype=np.float64), (n,)), np.zeros(n)])


def _case(points, queries, kw=None, slice_offsets=None, query_offsets=None):
    points = np.ascontiguousarray(np.concatenate(points) if isinstance(points, list) else points, dtype=np.float64)
    queries = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 2)
    return {"points": points.reshape(-1, 4), "queries": queries, "kw": dict(kw or {}),
            "slice_offsets": np.array([0, len(points)] if slice_offsets is None else slice_offsets, dtype=np.int64),
            "query_offsets": np.array([0, len(queries)] if query_offsets is None else query_offsets, dtype=np.int64)}


def bin_centre(b, z_lo=Z_LO, bin=BIN):
    return z_lo + (b + 0.5) * bin


def hits_case():
    """No hit; min_points - 1 and exactly min_points hits; points at d2 == r2 exactly and one ulp
    outside; non-finite points among finite ones."""
    q = np.array([[0.0, 0.0], [4.0, 0.0], [8.0, 0.0], [12.0, 0.0], [16.0, 0.0], [20.0, 0.0]])
    z = bin_centre(100)
    nan, inf = float("nan"), float("inf")
    on = [[12.5, 0.0, z, 0.0], [11.5, 0.0, z, 0.0], [12.0, 0.5, z, 0.0], [12.0, -0.5, z, 0.0],         # d2 == r2
          [np.nextafter(12.5, inf), 0.0, z, 0.0], [12.0, np.nextafter(-0.5, -inf), z, 0.0]]            # one ulp outside
    bad = [[nan, 0.0, z, 0.0], [16.0, inf, z, 0.0], [16.1, 0.1, nan, 0.0], [16.1, -0.1, -inf, 0.0], [-inf, nan, inf, 0.0],
           [15.9, 0.1, inf, 0.0]]
    pts = [_ring(q[1], MIN_POINTS - 1, z), _ring(q[2], MIN_POINTS, z), np.array(on), _ring(q[3], 1, z, 0.125),
           np.array(bad), _ring(q[4], MIN_POINTS, z),
           _ring(q[5], 2 * MIN_POINTS, [bin_centre(60)] * (MIN_POINTS - 1) + [bin_centre(64)] * (MIN_POINTS + 1))]
    return _case(pts, q)


def bins_case():
    """z exactly on bin edges; z just outside the histogram on both sides; all hits in bin 0 and all
    in bin n_bins - 1; two equal modes; a climb of two bins; negative z whose qz is a half-way case."""
    q = np.array([[4.0 * k, 10.0] for k in range(8)])
    inf = float("inf")
    edge = [Z_LO + b * BIN for b in (96, 96, 97, 97, 97, 98, 99)]                       # on the edges: bin b itself
    top = Z_LO + N_BINS * BIN
    outside = [np.nextafter(Z_LO, -inf)] * 3 + [top] * 3 + [top + 1.0] + [Z_LO] * 3 + [np.nextafter(top, -inf)] * 4
    low = [Z_LO, Z_LO + 0.01, Z_LO + 0.03, np.nextafter(Z_LO + BIN, -inf), Z_LO + 0.05, Z_LO + 0.06]
    high = [np.nextafter(top, -inf), top - 0.01, top - 0.03, top - BIN, top - 0.05, top - 0.06]
    equal = [bin_centre(100)] * 6 + [bin_centre(140)] * 6
    climb = [bin_centre(50)] * 6 + [bin_centre(51)] * 2 + [bin_centre(52)] * 3 + [bin_centre(53)] * 4
    half = [-(2 * k + 1) / 131072.0 - 1.5 for k in (0, 1, 2, 3, 4, 5, 6)]               # z * 65536 = -(98304 + k) - 0.5
    strong_above = [bin_centre(80)] * 7 + [bin_centre(120)] * 13                        # 7 >= ceil(13 / 2): the lower wins
    zs = (edge, outside, low, high, equal, climb, half, strong_above)
    return _case([_ring(q[k], len(z), z) for k, z in enumerate(zs)], q)


def params_case():
    """Other parameters than the defaults: 40 bins of 1/8 m from -2, min_points 3, peak share 2/3, radius 1."""
    q = np.array([[0.0, 0.0], [6.0, 0.0], [12.0, 0.0]])
    kw = {"radius": 1.0, "z_lo": -2.0, "bin": 0.125, "n_bins": 40, "min_points": 3, "peak_share": (2, 3)}
    c = lambda b: bin_centre(b, -2.0, 0.125)
    zs = ([c(5)] * 7 + [c(20)] * 12,            # 7 < ceil(12 * 2 / 3) = 8: the upper mode
          [c(5)] * 8 + [c(20)] * 12,            # 8 >= 8: the lower mode
          [c(39)] * 2 + [3.0] * 5)              # 2 < min_points in the histogram, 5 above it: no ground, 7 hits
    return _case([_ring(q[k], len(z), z, 0.75) for k, z in enumerate(zs)], q, kw)


def cells_case():
    """Points exactly on cell borders (and one ulp to either side) of the grid the host lays for cell
    = radius and cell = 4 radius; 1, 63, 64, 65 and 257 points in one cell."""
    sizes = (1, 63, 64, 65, 257)
    q = np.array([[3.0 * k, 30.0] for k in range(len(sizes))] + [[15.25, 30.25], [17.25, 31.25]])
    rng = np.random.default_rng(18)
    pts = []
    for k, n in enumerate(sizes):               # a patch 1/8 m wide right of and above the query: one cell
        xy = q[k] + (1 + rng.integers(0, 8, (n, 2))) / 64.0
        z = bin_centre(90) + rng.integers(-6, 7, n) / 256.0
        pts.append(np.column_stack([xy, z, np.zeros(n)]))
    x0 = q[:, 0].min() - (RADIUS + GUARD)       # the grid's origin, as the rule lays it
    y0 = q[:, 1].min() - (RADIUS + GUARD)
    inf = float("inf")
    for k, cell in ((len(sizes), RADIUS), (len(sizes) + 1, 4.0 * RADIUS)):
        bx = [x0 + j * cell for j in range(int((q[k, 0] - 0.5 - x0) / cell), int((q[k, 0] + 0.5 - x0) / cell) + 2)]
        by = [y0 + j * cell for j in range(int((q[k, 1] - 0.5 - y0) / cell), int((q[k, 1] + 0.5 - y0) / cell) + 2)]
        edge = [[x, y] for x in bx for y in by] + [[np.nextafter(x, s), np.nextafter(y, s)] for x in bx for y in by
                                                   for s in (-inf, inf)]
        edge = np.array(edge)
        z = bin_centre(90) + (np.arange(len(edge)) % 5 - 2) / 256.0
        pts.append(np.column_stack([edge, z, np.zeros(len(edge))]))
    return _case(pts, q)


def _road(rng, n, x_lo, x_hi, y_lo, y_hi, z, sigma=0.02):
    """n points of a flat road: xy in sixty-fourths, z = z + N(0, sigma) in 1/4096."""
    x = np.round(rng.uniform(x_lo, x_hi, n) * 64.0) / 64.0
    y = np.round(rng.uniform(y_lo, y_hi, n) * 64.0) / 64.0
    h = np.round((z + rng.normal(0.0, sigma, n)) * 4096.0) / 4096.0
    return np.column_stack([x, y, h, rng.uniform(0.0, 60.0, n).round()])


def queries_case(n_q):
    """Q queries along a road of 1,500 points 30 m long; the last one outside the points' extent."""
    rng = np.random.default_rng(180)
    pts = _road(rng, 1500, 0.0, 30.0, -0.75, 0.75, -1.7)
    q = np.column_stack([np.linspace(0.3, 29.7, n_q), rng.uniform(-0.3, 0.3, n_q)])
    q[-1] = [45.0, 9.0] if n_q > 1 else q[-1]
    return _case(pts, q)


def ragged_case():
    """Six slices: three roads of 700, 1,300 and 401 points over the same xy at -1.7, -0.4 and +2.0 m
    (each the decoy of its neighbours), an empty slice, a slice with queries and no points, a slice
    with points and no queries."""
    rng = np.random.default_rng(181)
    roads = [_road(rng, n, -0.6, 16.6, -0.6, 0.6, z) for n, z in ((700, -1.7), (1300, -0.4), (401, 2.0))]
    lonely = _road(rng, 90, 0.0, 5.0, -1.0, 1.0, 0.5)
    qs = [np.column_stack([np.linspace(0.0, 16.0, n), np.full(n, y)]) for n, y in ((17, 0.25), (9, -0.25), (33, 0.0))]
    qs.append(np.array([[1.0, 0.0], [2.0, 0.5]]))
    soff = np.cumsum([0, 700, 1300, 401, 0, 0, 90])
    qoff = np.cumsum([0, 17, 9, 33, 0, 2, 0])
    return _case(roads + [lonely], np.concatenate(qs), None, soff, qoff)


def analytic_road():
    """The plane z = -1.7 + 0.02 x + 0.01 y with N(0, 0.02) noise at 100 points / m^2 over x in
    [-0.5, 20.5], y in [-2.3, 2.3]; stations every metre on y = +-1.75.  Returns (case, plane heights)."""
    rng = np.random.default_rng(182)
    n = int(round(100 * 21.0 * 4.6))
    x, y = rng.uniform(-0.5, 20.5, n), rng.uniform(-2.3, 2.3, n)
    z = -1.7 + 0.02 * x + 0.01 * y + rng.normal(0.0, 0.02, n)
    q = np.array([[float(i), s] for s in (-1.75, 1.75) for i in range(21)])
    return _case(np.column_stack([x, y, z, np.zeros(n)]), q), -1.7 + 0.02 * q[:, 0] + 0.01 * q[:, 1]


def slab_case(density_ratio):
    """A road at -1.7 m at 100 points / m^2 and a slab 1.2 m above it at density_ratio times that, 4 m x 4 m."""
    rng = np.random.default_rng(183)
    road = _road(rng, 1600, 0.0, 4.0, 0.0, 4.0, -1.7)
    slab = _road(rng, int(1600 * density_ratio), 0.0, 4.0, 0.0, 4.0, -0.5)
    return _case([road, slab], np.array([[1.0, 1.0], [2.0, 2.0], [3.0, 3.0], [1.0, 3.0]]))


DESIGNED = {"hits": hits_case, "bins": bins_case, "params": params_case, "cells": cells_case}


@functools.lru_cache(maxsize=None)
def case(name):
    """A case by name: a designed one, 'queries<Q>', 'ragged'."""
    if name in DESIGNED:
        return DESIGNED[name]()
    if name.startswith("queries"):
        return queries_case(int(name[len("queries"):]))
    return {"ragged": ragged_case}[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's outputs for case(name): computed once per process."""
    c = case(name)
    return O.ground_heights(c["points"], c["slice_offsets"], c["queries"], c["query_offsets"], **c["kw"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
