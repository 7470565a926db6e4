"""Inputs the surface-gate tests share (test_trace_surface_cpu.py, test_trace_surface_gpu.py).  A case is
{'points' (T,4) float64, 'slice_offsets', 'ground' (S,gx,gy) float64, 'kw'}: the arguments of
_trace_surface_oracle.paint_peaks and, without the g_* window, of trace.paint_peaks.  Every coordinate
but the two marked ones is a float32 value, and the grids are exact in binary."""
import functools

import numpy as np

import _trace_surface_oracle as SO

NAN, INF = float("nan"), float("inf")
# trace grid: x in [-4, 4) in 16 columns, y in [-2, 2) in 64 cells; ground grid: 8 x 4 cells of 1 m
GRID = dict(half_length=4.0, col=0.5, half_width=2.0, cell=0.0625)
BAND = 0.125                 # exact in binary, so z - g == band can be met exactly
FLOOR = 8.0
KW = dict(GRID, intensity_floor=FLOOR, min_points=1, nms=1, band=BAND)


def designed_case():
    """Two slices.  Slice 0's road is at 0 but for cell (2, 1) at 1.5 and cell (3, 2), which has none;
    slice 1's road is at 2 everywhere, so a point of slice 1 tested against slice 0's rows is misjudged.
    Returns (case, the expected off_surface, the rows of slice 0 in the order of 'what')."""
    ground = np.zeros((2, 8, 4))
    ground[0, 2, 1], ground[0, 3, 2], ground[1] = 1.5, NAN, 2.0
    s0 = [
        ("z - g == band: kept", [-1.5, -0.5, 1.625, 50.0], False),
        ("one ulp beyond band (float64 only)", [-1.5, -0.25, np.nextafter(1.625, INF), 50.0], True),
        ("g - z == band: kept", [-1.25, -0.75, 1.375, 50.0], False),
        ("one ulp beyond, below (float64 only)", [-1.25, -0.875, np.nextafter(1.375, -INF), 50.0], True),
        ("a NaN ground cell", [-0.5, 0.5, 0.0, 50.0], True),
        ("x on a ground-cell edge belongs to the upper cell, whose road is at 0", [-1.0, -0.5, 0.0, 50.0], False),
        ("the same edge at the lower cell's height", [-1.0, -0.375, 1.5, 50.0], True),
        ("-0.0 in x, y and z", [-0.0, -0.0, -0.0, 50.0], False),
        ("z = inf over the NaN cell: the tracing rule drops it first", [-0.5, 0.75, INF, 50.0], None),
        ("|z| > 512 over the NaN cell: likewise", [-0.75, 0.75, 600.0, 50.0], None),
        ("a dim point off the surface: qi == 0 drops it first", [1.5, 0.5, 5.0, FLOOR], None),
        ("outside the trace grid and off the surface", [4.0, 0.5, 5.0, 50.0], None),
        ("inside the trace grid, outside a ground window of half length 3: x high", [3.5, 1.5, 0.0, 50.0], False),
        ("the same: x low", [-3.5, 1.5, 0.0, 50.0], False),
        ("a bright thing 0.625 m up", [2.5, -1.5, 0.625, 200.0], True),
    ]
    s1 = [("on slice 1's road", [0.5, 0.5, 2.0, 50.0], False), ("on slice 0's road, in slice 1", [0.5, -0.5, 0.0, 50.0], True)]
    pts = np.array([r[1] for r in s0 + s1], dtype=np.float64)
    case = {"points": pts, "slice_offsets": np.array([0, len(s0), len(s0) + len(s1)], dtype=np.int64), "ground": ground,
            "kw": dict(KW)}
    return case, [sum(r[2] is True for r in s0), sum(r[2] is True for r in s1)], s0 + s1


def as_float32_values(case):
    """The case with every coordinate rounded to float32 (held as float64): what both dtypes can be given."""
    return dict(case, points=case["points"].astype(np.float32).astype(np.float64))


RAGGED_GRID = dict(half_length=8.0, col=0.5, half_width=4.0, cell=0.0625)      # 32 x 128 cells; ground 16 x 8
RAGGED_SIZES = (0, 1, 257, 5000)


@functools.lru_cache(maxsize=None)
def ragged_case():
    """Slices of 0, 1, 257 and 5,000 points, shuffled; slice s's road is a plane at 1 + s / 4 with a step
    per ground cell and a few cells without ground; 30 % of the points are paint on two lanes at
    intensity 40-60, the rest asphalt at 0-10, and about a third of the paint is lifted 0.6 m off the
    road.  Every value is a float32 value.  Returns (case, the oracle's result: computed once)."""
    rng = np.random.default_rng(230)
    ground = np.stack([1.0 + 0.25 * s + 0.015625 * rng.integers(-2, 3, (16, 8)) for s in range(len(RAGGED_SIZES))])
    ground[rng.random(ground.shape) < 0.05] = NAN
    slices = []
    for s, n in enumerate(RAGGED_SIZES):
        x, y = rng.uniform(-8.5, 8.5, n), rng.uniform(-4.25, 4.25, n)
        paint = rng.random(n) < 0.3
        y[paint] = rng.choice([-1.7, 1.9], int(paint.sum())) + rng.uniform(-0.075, 0.075, int(paint.sum()))
        gix, giy = np.clip(np.floor(x + 8.0), 0, 15).astype(int), np.clip(np.floor(y + 4.0), 0, 7).astype(int)
        z = np.nan_to_num(ground[s][gix, giy], nan=1.0) + rng.normal(0.0, 0.02, n) + 0.6 * (paint & (rng.random(n) < 0.33))
        slices.append(np.column_stack([x, y, z, np.where(paint, rng.uniform(40.0, 60.0, n), rng.uniform(0.0, 10.0, n))]))
    slices[1][0] = [1.0, 1.9, 5.0, 55.0]                         # the one point of slice 1: bright and off the surface
    pts = np.concatenate(slices).astype(np.float32).astype(np.float64)
    case = {"points": np.ascontiguousarray(pts), "slice_offsets": np.cumsum((0,) + RAGGED_SIZES).astype(np.int64),
            "ground": ground, "kw": dict(RAGGED_GRID, intensity_floor=20.0)}
    return case, SO.paint_peaks(case["points"], case["slice_offsets"], ground, **case["kw"])
