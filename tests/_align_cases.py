"""Inputs the paint-alignment tests share (test_align_cpu.py, test_align_gpu.py and the maker of
g19).  A case is {'points' (T,4) float64, 'slice_offsets', 'lines' [per slice the list of (n,3)
polylines], 'shifts' (K,2), 'shift_offsets', 'kw'}: the arguments of paint_scores.  The designed
cases (hits, tiles) are written point by point and go into the fixture; the seeded ones (segtile,
ragged, small) are generated here and the oracle's result is computed once per process and never
written to.  Every case stays at or below about 2e5 (candidate, shift, segment) products: the oracle
is a quadruple Python loop.

paint_scores_np is the second, independent restatement of the rule: numpy over the points of one
(line, segment) at a time, with a per-segment box pre-selection of its own.  paint_frame and
paint_drive generate the analytic frame and the detector drive of the end-to-end tests.

Their yaw is small on purpose (YAW = 1 mrad, the drive's poses up to 1.5 mrad).  The rule returns the
shortest near-best shift, which has no along-lane component only while that component buys nothing:
at a yaw psi an along-lane shift dx moves a line laterally by dx psi, and a row of the 0.02 m fine
grid that lies 0.02 m from the optimum sits 0.002 m outside the near-best band (0.018 m at r = 0.15),
so dx psi and the 0.3 m along-lane offset times psi must both stay well below 0.002 m.  At 3 mrad the
first frame of the drive returns dx = 0.1 (lateral residual 0.019 m, still inside its bound)."""
import functools

import numpy as np

import _align_oracle as O

RADIUS = 0.15
GUARD = 1e-6
TILE = 512                   # prh_align_tile()
FIXTURE_CASES = ("hits", "tiles")
KEYS = ("score", "hits")
NAN, INF = float("nan"), float("inf")


def _case(points, lines, shifts, kw=None, slice_offsets=None, shift_offsets=None):
    points = np.ascontiguousarray(np.concatenate(points) if isinstance(points, list) else points, dtype=np.float64)
    shifts = np.ascontiguousarray(np.concatenate(shifts) if isinstance(shifts, list) else shifts, dtype=np.float64)
    return {"points": points.reshape(-1, 4), "shifts": shifts.reshape(-1, 2), "kw": dict(kw or {}),
            "lines": [[np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in ls] for ls in lines],
            "slice_offsets": np.array([0, len(points)] if slice_offsets is None else slice_offsets, dtype=np.int64),
            "shift_offsets": np.array([0, len(shifts)] if shift_offsets is None else shift_offsets, dtype=np.int64)}


def hits_case():
    """radius 0.25 (r2 = 1/16 exactly).  Line A has a zero-length segment, line B one vertex, line C
    runs 0.25 m beside A.  Points: d2 == r2 exactly, on the line (qk = 1024), one ulp outside, past
    the line's end (u clamped), off in z, in two tubes, non-finite x / y / z / I, qi == 0 (I = 0,
    below the floor, half-way down) and qi at the clamp."""
    a = [[0.0, 0.0, 0.0], [4.0, 0.0, 0.0], [4.0, 0.0, 0.0], [8.0, 0.0, 0.0]]
    b = [[2.0, 5.0, 0.0]]
    c = [[0.0, 0.25, 0.0], [8.0, 0.25, 0.0]]
    pts = [[1.0, -0.25, 0.0, 10.0],                           # d2 == r2 on A: a hit with qk = 0
           [2.0, 0.0, 0.0, 20.0],                             # on A, and d2 == r2 on C
           [3.0, np.nextafter(-0.25, -INF), 0.0, 30.0],       # one ulp outside A
           [8.125, 0.0, 0.0, 12.0], [-0.125, 0.25, 0.0, 13.0],      # past the ends
           [2.5, 0.0, 0.1875, 50.0], [2.5, 0.0, 0.3125, 50.0],      # off in z: inside, outside
           [6.0, 0.125, 0.0, 40.0],                           # in the tubes of A and C
           [4.0, -0.125, 0.0, 21.0],                          # beside the zero-length segment
           [2.0, 5.0, 0.0, 33.0],                             # on the one-vertex line: no hit
           [NAN, 0.0, 0.0, 5.0], [1.0, INF, 0.0, 5.0], [1.0, 0.0, -INF, 5.0], [1.5, 0.0, 0.0, NAN], [1.5, 0.0, 0.0, INF],
           [1.5, 0.0, 0.0, -INF],
           [5.0, 0.0, 0.0, 0.0], [5.0, 0.0, 0.0, 0.001], [5.0, 0.0, 0.0, 0.5 / 256.0], [5.0, 0.0, 0.0, 1.5 / 256.0],
           [5.0, 0.0, 0.0, 2.5 / 256.0], [5.0, 0.0, 0.0, -3.0],
           [7.0, 0.0625, 0.0, 5000.0]]                        # the weight clamp
    shifts = [[0.0, 0.0], [0.0, -0.25], [0.125, 0.125], [-3.0, 0.25]]
    return _case(np.array(pts), [[a, b, c]], np.array(shifts), {"radius": 0.25})


def _strip(rng, n, length=10.0, half=0.4):
    """n bright points around the x axis: xy in sixty-fourths, intensity a whole number 1 .. 60."""
    x = np.round(rng.uniform(0.0, length, n) * 64.0) / 64.0
    y = np.round(rng.uniform(-half, half, n) * 64.0) / 64.0
    z = np.round(rng.normal(0.0, 0.02, n) * 1024.0) / 1024.0
    return np.column_stack([x, y, z, rng.integers(1, 61, n).astype(np.float64)])


def _table(rng, k):
    """k shifts within +-0.3 m in sixty-fourths, (0, 0) among them."""
    t = np.round(rng.uniform(-0.3, 0.3, (k, 2)) * 64.0) / 64.0
    t[rng.integers(0, k)] = 0.0
    return t


def tiles_case():
    """Six slices with 0, 1, 63, 64, 65 and 257 candidates (and some dim or far points the filter
    drops) and tables of 16, 1, 15, 16, 17 and 17 shifts, one line of two segments each."""
    rng = np.random.default_rng(19)
    n_c, n_k = (0, 1, 63, 64, 65, 257), (16, 1, 15, 16, 17, 17)
    pts, tabs = [], []
    for n in n_c:
        dim = _strip(rng, 3)
        dim[:, 3] = 0.0
        far = _strip(rng, 2) + np.array([0.0, 40.0, 0.0, 0.0])
        pts.append(np.concatenate([_strip(rng, n), dim, far]))
    for k in n_k:
        tabs.append(_table(rng, k))
    line = [[0.0, 0.0, 0.0], [5.0, 0.0625, 0.0], [10.0, 0.0, 0.0]]
    return _case(pts, [[line]] * 6, tabs, None, np.cumsum([0] + [len(p) for p in pts]), np.cumsum((0,) + n_k))


def _zigzag(n_vertices, x0=0.0, y0=0.0):
    k = np.arange(n_vertices)
    return np.column_stack([x0 + k / 16.0, y0 + (k % 2) / 64.0, np.zeros(n_vertices)])


def segtile_case():
    """Slice 0: one line of TILE segments; slice 1: one of TILE + 1; slice 2: two lines of 300
    vertices, the second straddling the tile.  Points sit at the first segment, at the last slot of
    the first tile, at the first of the second, and at random."""
    rng = np.random.default_rng(190)
    lines = [[_zigzag(TILE + 1)], [_zigzag(TILE + 2)], [_zigzag(300), _zigzag(300, 0.0, 1.0)]]
    pts = []
    for s, at in enumerate(((0, TILE - 1, TILE - 2, 100), (0, TILE - 1, TILE, 7), (0, 299, 211 + 300, 212 + 300, 250 + 300))):
        rows = []
        for k in at:
            y0 = 1.0 if (s == 2 and k >= 300) else 0.0
            kk = k - 300 if (s == 2 and k >= 300) else k
            rows.append([kk / 16.0 + 1.0 / 32.0, y0 + 1.0 / 32.0, 0.0, 10.0 + k % 7])
        extra = _strip(rng, 6, 32.0, 0.2)
        pts.append(np.concatenate([np.array(rows), extra]))
    shifts = np.array([[0.0, 0.0], [0.03125, -0.015625]])
    return _case(pts, lines, [shifts] * 3, None, np.cumsum([0] + [len(p) for p in pts]), [0, 2, 4, 6])


def ragged_case():
    """Six slices: lines and points; nothing at all; lines and no points; points and no lines; two
    lines (one with a vertex only) under another table; a slanted line off in z.  Every coordinate
    is a float32 value."""
    rng = np.random.default_rng(191)
    a = [[0.0, 0.0, 0.0], [4.0, 0.125, 0.0], [10.0, 0.0, 0.0]]
    b = [[0.0, 0.25, 0.0], [10.0, 0.375, 0.0]]
    c = [[0.0, -0.5, 0.25], [5.0, 0.5, 0.5], [5.0, 0.5, 0.5], [10.0, -0.5, 0.25]]
    p0, p3, p4 = _strip(rng, 90), _strip(rng, 40), _strip(rng, 70)
    p5 = _strip(rng, 60, 10.0, 0.7) + np.array([0.0, 0.0, 0.375, 0.0])
    t0, t4 = _table(rng, 20), _table(rng, 9)
    lines = [[a], [], [a, b], [], [a, [[3.0, 0.0, 0.0]], b], [c]]
    return _case([p0, p3, p4, p5], lines, [t0, t0[:3], t0, t0, t4, t0], None,
                 np.cumsum([0, 90, 0, 0, 40, 70, 60]), np.cumsum([0, 20, 3, 20, 20, 9, 20]))


def small_frames():
    """Three slices small enough for the oracle's two align stages (441 + 122 shifts): a line of two
    segments with 24 paint points 0.25 m to its left, the same with the paint on the line (no
    gain), and one with 5 points (below min_points = 8)."""
    rng = np.random.default_rng(192)
    line = [[0.0, 0.0, 0.0], [6.0, 0.0, 0.0], [12.0, 0.03125, 0.0]]
    pts = []
    for n, y in ((24, 0.25), (24, 0.0), (5, -0.3)):
        p = _strip(rng, n, 12.0, 0.03)
        p[:, 1] += y
        p[:, 3] = 40.0 + p[:, 3] % 20.0
        pts.append(p)
    return {"points": np.concatenate(pts), "slice_offsets": np.cumsum([0] + [len(p) for p in pts]),
            "lines": [[np.array(line)], [np.array(line)], [np.array(line)]]}


DESIGNED = {"hits": hits_case, "tiles": tiles_case}
SEEDED = {"segtile": segtile_case, "ragged": ragged_case}


@functools.lru_cache(maxsize=None)
def case(name):
    return dict(DESIGNED, **SEEDED)[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle's tables for case(name): computed once per process."""
    c = case(name)
    return O.paint_scores(c["points"], c["slice_offsets"], c["lines"], c["shifts"], c["shift_offsets"], **c["kw"])


def csr(lines_per_slice):
    """(vertices (V,3), line_offsets (L+1,), slice_line_offsets (S+1,)) of a case's lines."""
    flat = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for ls in lines_per_slice for v in ls]
    l_off = np.cumsum([0] + [len(v) for v in flat]).astype(np.int64)
    sl_off = np.cumsum([0] + [len(ls) for ls in lines_per_slice]).astype(np.int64)
    return (np.concatenate(flat) if l_off[-1] else np.zeros((0, 3))), l_off, sl_off


def from_csr(verts, l_off, sl_off):
    return [[verts[l_off[l]:l_off[l + 1]] for l in range(sl_off[s], sl_off[s + 1])] for s in range(len(sl_off) - 1)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ------------------------------------------------------------------ the numpy restatement
def paint_scores_np(points, slice_offsets, lines_per_slice, shifts, shift_offsets, radius=RADIUS, intensity_floor=0.0):
    """The rule in numpy float64, one rounding per operation as numpy does: per slice an array d2min
    [P, K] per line, filled one segment at a time over the points inside that segment's own
    reach-expanded box (cost only), then the integer sums."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    shifts = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    r2 = float(radius) * float(radius)
    out = {"score": np.zeros(len(shifts), dtype=np.int64), "hits": np.zeros(len(shifts), dtype=np.int64)}
    for s in range(len(slice_offsets) - 1):
        p = pts[int(slice_offsets[s]):int(slice_offsets[s + 1])]
        sh = shifts[int(shift_offsets[s]):int(shift_offsets[s + 1])]
        if len(p) == 0 or len(sh) == 0 or len(lines_per_slice[s]) == 0:
            continue
        with np.errstate(invalid="ignore"):
            wi = np.minimum(np.maximum(p[:, 3] - float(intensity_floor), 0.0), 4096.0)
        qi = np.where(np.isfinite(p[:, 3]), np.rint(np.nan_to_num(wi) * 256.0), 0.0).astype(np.int64)
        p, qi = p[np.isfinite(p[:, :3]).all(axis=1) & (qi > 0)], qi[np.isfinite(p[:, :3]).all(axis=1) & (qi > 0)]
        reach = float(radius) + float(np.abs(sh).max()) + GUARD
        score = np.zeros(len(sh), dtype=np.int64)
        hits = np.zeros(len(sh), dtype=np.int64)
        for line in lines_per_slice[s]:
            line = np.asarray(line, dtype=np.float64).reshape(-1, 3)
            d2min = np.full((len(p), len(sh)), np.inf)
            for k in range(len(line) - 1):
                a, e = line[k], line[k + 1] - line[k]
                l2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                if not l2 > 0.0:
                    continue
                lo, hi = np.minimum(line[k], line[k + 1])[:2] - reach, np.maximum(line[k], line[k + 1])[:2] + reach
                sel = np.flatnonzero((p[:, 0] >= lo[0]) & (p[:, 0] <= hi[0]) & (p[:, 1] >= lo[1]) & (p[:, 1] <= hi[1]))
                if len(sel) == 0:
                    continue
                wx = p[sel, 0][:, None] - sh[None, :, 0]
                wy = p[sel, 1][:, None] - sh[None, :, 1]
                wz = np.broadcast_to(p[sel, 2][:, None], wx.shape)
                gx, gy, gz = wx - a[0], wy - a[1], wz - a[2]
                u = np.minimum(np.maximum(((gx * e[0] + gy * e[1]) + gz * e[2]) / l2, 0.0), 1.0)
                hx, hy, hz = wx - (a[0] + u * e[0]), wy - (a[1] + u * e[1]), wz - (a[2] + u * e[2])
                d2min[sel] = np.minimum(d2min[sel], (hx * hx + hy * hy) + hz * hz)
            hit = d2min <= r2
            qk = np.rint((1.0 - np.where(hit, d2min, 0.0) / r2) * 1024.0).astype(np.int64)
            score += (np.where(hit, qk, 0) * qi[:, None]).sum(axis=0)
            hits += hit.sum(axis=0)
        out["score"][int(shift_offsets[s]):int(shift_offsets[s + 1])] = score
        out["hits"][int(shift_offsets[s]):int(shift_offsets[s + 1])] = hits
    return out


# ------------------------------------------------------------------ the analytic frame and the drive
LANE_Y = (-1.7, 1.9)
OFFSET = (0.3, 0.44)         # the detector's lines lie here from the lanes, in every ego frame
PAINT_HALF = 0.075
BOUND_DX, BOUND_Y = 0.02, 0.04
SEED = 193
YAW = 0.001                  # of the analytic frame; the drive's poses yaw by YAW * (k - 1.5)


def paint_cloud(rng, x_lo, x_hi, asphalt_per_m2=7.0, paint_per_m=60.0, z=0.0):
    """(n,4) float64: asphalt at intensity 0-10 over y in [-4, 4], and per lane a band of paint +-0.075
    m wide at intensity 40-60; heights z + N(0, 0.02)."""
    n_a = int(round(asphalt_per_m2 * (x_hi - x_lo) * 8.0))
    n_p = int(round(paint_per_m * (x_hi - x_lo)))
    parts = [np.column_stack([rng.uniform(x_lo, x_hi, n_a), rng.uniform(-4.0, 4.0, n_a), z + rng.normal(0.0, 0.02, n_a),
                              rng.uniform(0.0, 10.0, n_a)])]
    for y in LANE_Y:
        parts.append(np.column_stack([rng.uniform(x_lo, x_hi, n_p), y + rng.uniform(-PAINT_HALF, PAINT_HALF, n_p),
                                      z + rng.normal(0.0, 0.02, n_p), rng.uniform(40.0, 60.0, n_p)]))
    return np.concatenate(parts)


def paint_frame(paint_per_m=60.0, yaw=YAW, seed=SEED):
    """One frame in its own ego frame: the cloud over |x| <= 25, and the two lanes as the detector
    sees them - vertices every 5 m, turned by yaw about the origin, moved by OFFSET.  Returns (points,
    [line, line])."""
    rng = np.random.default_rng(seed)
    pts = paint_cloud(rng, -25.0, 25.0, paint_per_m=paint_per_m)
    c, s = np.cos(yaw), np.sin(yaw)
    lines = []
    for y in LANE_Y:
        x = np.linspace(-24.0, 24.0, 11)
        lines.append(np.column_stack([c * x - s * y + OFFSET[0], s * x + c * y + OFFSET[1], np.zeros(11)]))
    return pts, lines


def paint_drive(pose_z=0.0, pitch=0.0, seed=SEED):
    """The detector drive of the end-to-end tests: the world cloud over x in [-8, 128] with the road
    at z = 0, 4 poses 25 m apart with a little yaw (and pose_z, pitch for the raised variant), and
    per frame the BEV pixels of the two lanes moved by OFFSET in that frame.  Returns (cloud (n,4),
    poses (4,7), pixels [frame][lane] (n,2))."""
    import _fuse_oracle as FO
    rng = np.random.default_rng(seed)
    cloud = paint_cloud(rng, -8.0, 128.0)
    poses, pixels = [], []
    for k in range(4):
        pose = np.array([25.0 * (k + 1), 0.3 * k, pose_z, *FO.quat_yaw_pitch(YAW * (k - 1.5), pitch)])
        poses.append(pose)
        frame = []
        for y in LANE_Y:
            lane = np.stack([np.linspace(-10.0, 140.0, 601), np.full(601, y), np.zeros(601)], 1)
            ego = FO.to_ego(lane, pose)
            ego = ego[np.abs(ego[:, 0]) <= 24.0][::20]
            frame.append(np.stack([(25.0 - (ego[:, 1] + OFFSET[1])) / 0.05, (25.0 - (ego[:, 0] + OFFSET[0])) / 0.05], 1))
        pixels.append(frame)
    return cloud, np.array(poses), pixels


def pixel_to_ego(pixels):
    """predictions.pixel_to_ego, restated: x = 25 - v * 0.05, y = 25 - u * 0.05, z = 0."""
    px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    return np.column_stack([25.0 - px[:, 1] * 0.05, 25.0 - px[:, 0] * 0.05, np.zeros(len(px))])


def lateral_residual(lines, shift, lane_y, yaw=0.0, pose=None):
    """The largest distance of a vertex of the shifted lines from its lane: through the pose into the
    world, where the lanes run along x (pose given), or in paint_frame's own frame, where they are
    turned by yaw about the origin."""
    import _fuse_oracle as FO
    worst = 0.0
    for v, y in zip(lines, lane_y):
        w = np.array(v, dtype=np.float64)
        w[:, 0] += shift[0]
        w[:, 1] += shift[1]
        if pose is not None:
            lateral = FO.to_world(w[None], np.array([0]), pose[None])[0][:, 1]
        else:
            lateral = -np.sin(yaw) * w[:, 0] + np.cos(yaw) * w[:, 1]
        worst = max(worst, float(np.abs(lateral - y).max()))
    return worst
