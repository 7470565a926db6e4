"""Inputs the cloud-support tests share (test_support_gpu.py, test_support_cpu.py and the maker of
g17): the shapes case, the fixture's case and the painted drive.  Everything is seeded; the oracle's
results are computed once per process and never written to."""
import functools

import numpy as np

import _fuse_oracle as FO
import _support_oracle as O

BASE = np.array([400123.0, 3200456.0, 52.0])          # 400 km / 3,200 km from zero
FLOOR = 10.25                                         # intensity floor of the exact cases: a multiple of 1/4
SIZES = (1, 255, 256, 257, 3001)
MARGIN_D2, MARGIN_STATION, MARGIN_QUANT = 1e-9, 1e-9, 1e-8


def shapes_lines():
    """A 2-vertex line, one with a duplicated vertex, one whose vertices are all equal, one shorter
    than the step, one with a vertical segment, a 60 degree corner, two lines that cross and two
    parallel lines 0.4 m apart.  All tilted in z (the vertical segment apart)."""
    rng = np.random.default_rng(31)
    two = np.stack([BASE + [0.0, -6.0, 0.0], BASE + [30.0, -5.0, 0.4]])
    dup = FO.curved_carrier(12, BASE + [0.0, -3.0, 0.2], rng, 30.0)
    dup = np.concatenate([dup[:5], dup[4:5], dup[5:]])
    same = np.repeat((BASE + [10.0, 8.0, 0.0])[None], 4, axis=0)
    short = np.stack([BASE + [5.0, 5.0, 0.0], BASE + [5.3, 5.1, 0.01]])
    vertical = np.stack([BASE + [0.0, 2.0, 0.0], BASE + [10.0, 2.2, 0.1], BASE + [10.0, 2.2, 0.9], BASE + [20.0, 2.5, 1.0]])
    corner = np.stack([BASE + [0.0, 12.0, 0.0], BASE + [10.0, 12.0, 0.2], BASE + [5.0, 12.0 + 10.0 * np.sin(np.pi / 3), 0.3]])
    cross_a = np.stack([BASE + [0.0, -12.0, 0.0], BASE + [20.0, -8.0, 0.3]])
    cross_b = np.stack([BASE + [0.0, -8.0, 0.1], BASE + [20.0, -12.0, 0.2]])
    par_a = np.stack([BASE + [0.0, -20.0, 0.0], BASE + [25.0, -19.0, 0.3]])
    d = par_a[1] - par_a[0]
    normal = np.array([-d[1], d[0], 0.0]) / np.hypot(d[0], d[1])
    par_b = par_a + 0.4 * normal
    # no vertex on a float32 value: where u is clamped, h = w - a would else be a multiple of the
    # cloud's float32 spacing and hz * 65536 could sit exactly on a half-integer
    off = np.array([0.00123456789, 0.00456789123, 0.0123456789])
    return [l + off for l in (two, dup, same, short, vertical, corner, cross_a, cross_b, par_a, par_b)]


def cloud_near(lines, n, rng, spreads=(0.45, 1.5)):
    """n points around the lines' arcs (float64 xyz + intensity in multiples of 1/4): a station on a
    random line, from half a metre before its start to half a metre past its end, plus a random
    vector from a ball whose radius alternates between spreads."""
    usable = [l for l, v in enumerate(lines) if len(v) >= 2 and FO.carrier_cum(v)[-1] > 0]
    out = np.zeros((n, 4))
    for i in range(n):
        v = lines[usable[rng.integers(len(usable))]]
        cum = FO.carrier_cum(v)
        c = FO.carrier_point(v, cum, rng.uniform(-0.5, cum[-1] + 0.5))
        h = rng.normal(size=3)
        out[i, :3] = c + h / np.linalg.norm(h) * spreads[i % len(spreads)] * rng.uniform() ** (1.0 / 3.0)
        out[i, 3] = rng.integers(0, 400) / 4.0
    return out


@functools.lru_cache(maxsize=None)
def shapes_case():
    """(lines, cloud (3001,4) float32).  Row 0 is a plain point next to the first line.  Among the
    rest: points far outside the grid box, points inside it far from every line, rows with nan /
    inf / -inf in each field that would hit if they were kept, and intensities below the floor,
    negative and above 4096 + FLOOR."""
    lines = shapes_lines()
    rng = np.random.default_rng(17)
    n = SIZES[-1]
    cloud = cloud_near(lines, n, rng)
    far = rng.choice(np.arange(1, n), 80, replace=False)
    cloud[far[:40], :2] += rng.uniform(300.0, 900.0, (40, 2)) * rng.choice([-1.0, 1.0], (40, 2))      # outside the box
    cloud[far[40:], :3] = BASE + np.column_stack([rng.uniform(0, 30, 40), rng.uniform(-2, 1, 40) + 7.0, np.full(40, 5.0)])
    bad = rng.choice(np.setdiff1d(np.arange(1, n), far), 12 + 9, replace=False)
    for r, (field, value) in zip(bad[:12], [(f, v) for f in range(4) for v in (np.nan, np.inf, -np.inf)]):
        cloud[r, field] = value
    cloud[bad[12:15], 3] = [0.25, 5.0, 10.0]                  # below the floor
    cloud[bad[15:18], 3] = [-0.25, -30.0, -4096.0]            # negative
    cloud[bad[18:21], 3] = [4096.0 + FLOOR + 0.25, 5000.0, 65536.0]      # above the clamp
    cloud[0, :3] = 0.5 * (lines[0][0] + lines[0][1]) + [0.0, 0.1, 0.05]
    cloud[0, 3] = 37.5
    return lines, cloud.astype(np.float32)


@functools.lru_cache(maxsize=None)
def shapes_oracle(step, radius):
    """The oracle over all 3001 points; a prefix of the cloud is O.accumulate(hits, N, points)."""
    lines, cloud = shapes_case()
    return O.support(cloud, lines, step, radius, FLOOR)


@functools.lru_cache(maxsize=None)
def fixture_case():
    """g17: three curved lines of 9, 14 and 2 vertices and 2,500 points around them."""
    rng = np.random.default_rng(170)
    start = BASE + [-20.0, 0.0, -1.5]
    lines = [FO.curved_carrier(9, start, rng, 40.0, -3.0), FO.curved_carrier(14, start, rng, 45.0, 0.5),
             np.stack([start + [0.0, 4.0, 0.0], start + [35.0, 5.0, 0.6]])]
    cloud = cloud_near(lines, 2500, rng, spreads=(0.45, 0.45))
    return lines, cloud.astype(np.float32)


def assert_margins(m):
    assert m["d2"] >= MARGIN_D2 and m["station"] >= MARGIN_STATION and m["quant"] >= MARGIN_QUANT, m


# ------------------------------------------------------------------ the painted drive
def _distance_xy(p, line):
    best = np.full(len(p), np.inf)
    for a, b in zip(line[:-1, :2], line[1:, :2]):
        e = b - a
        u = np.clip(((p - a) @ e) / (e @ e), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(p - (a + u[:, None] * e), axis=1))
    return best


@functools.lru_cache(maxsize=None)
def painted_drive():
    """4 poses 25 m apart and 120 k ground points on x in [-8, 83], y in [-4, 4], all in local
    coordinates (no BASE: the cloud is float32).  Asphalt intensity floor(U(0, 10)); the points
    within 0.075 m of line A are paint, floor(U(40, 60)), and so are those within 0.075 m of line B
    where x mod 9 < 3: A is a solid marking, B a dashed one.  The third line, at y = 3.5, has
    asphalt under it.  Returns (poses (4,7), cloud (120000,4) float32, [A, B, C])."""
    rng = np.random.default_rng(7)
    poses = np.zeros((4, 7))
    for k in range(4):
        poses[k, :3] = [25.0 * k, 0.3 * k, 0.0]
        poses[k, 3:] = FO.quat_yaw_pitch(0.04 * (k - 1.5), 0.0)
    n = 120000
    xyz = np.stack([rng.uniform(-8.0, 83.0, n), rng.uniform(-4.0, 4.0, n), rng.normal(0.0, 0.02, n)], 1)
    a, b = np.array([-10.3, -1.7, 0.0]), np.array([90.1, -1.3, 0.0])
    lines = [np.stack([a, a + 0.473 * (b - a), b]), np.array([[-10.7, 1.9, 0.0], [90.4, 1.6, 0.0]]),
             np.array([[-10.0, 3.5, 0.0], [90.0, 3.5, 0.0]])]
    intensity = np.floor(rng.uniform(0.0, 10.0, n))
    paint = np.floor(rng.uniform(40.0, 60.0, n))
    on_a = _distance_xy(xyz[:, :2], lines[0]) <= 0.075
    on_b = (_distance_xy(xyz[:, :2], lines[1]) <= 0.075) & (np.mod(xyz[:, 0], 9.0) < 3.0)
    intensity[on_a | on_b] = paint[on_a | on_b]
    return poses, np.column_stack([xyz, intensity]).astype(np.float32), lines
