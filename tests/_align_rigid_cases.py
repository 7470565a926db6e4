"""Inputs the rigid paint-alignment tests share (test_align_rigid_cpu.py, test_align_rigid_gpu.py and
the maker of g20).  A case is {'points' (T,4) float64, 'slice_offsets', 'lines' [per slice the list of
(n,3) polylines], 'poses' (K,3) dx dy theta, 'pose_offsets', 'pivots' (S,2), 'kw'}: the arguments of
rigid_scores.  The cases are _align_cases' clouds and lines under pose tables with real rotations and
non-zero pivots; the designed ones (hits, tiles) go into the fixture, the seeded ones (segtile,
ragged) are generated here, and the oracle's result is computed once per process and never written to.

rigid_scores_np is the second, independent restatement of the rule: numpy, the moved points of a
chunk of poses at a time, one (line, segment) at a time over the points inside that segment's own
box.  yawed_frame and yawed_drive are the analytic frame and the detector drive with the lines turned
about the sensor.

The bound of the analytic frame and of the drive (BOUND) is the rule's step 9': the shift bias 0.13 r,
the yaw bias 0.13 r sqrt(3) / lever and half a fine yaw step, both at the line end 24 m from the
pivot: 0.0195 + 0.0324 + 0.012 = 0.0639 m."""
import functools
import math

import numpy as np

import _align_cases as C
import _align_oracle as O
import _align_rigid_oracle as RO

KEYS = C.KEYS
FIXTURE_CASES = ("hits", "tiles")
LEVER = 25.0
END = 24.0                   # metres from the pivot to a line end
YAWS = (0.0, 0.006, 0.015)
BOUND = 0.13 * C.RADIUS + END * (0.13 * C.RADIUS * math.sqrt(3.0) / LEVER) + END * 0.0005


def _case(base, poses, pose_offsets, pivots, **more):
    out = {"points": base["points"], "slice_offsets": base["slice_offsets"], "lines": base["lines"], "kw": dict(base["kw"]),
           "poses": np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3),
           "pose_offsets": np.asarray(pose_offsets, dtype=np.int64),
           "pivots": np.ascontiguousarray(pivots, dtype=np.float64).reshape(-1, 2)}
    out.update(more)
    return out


def boundary_pair(line, pose, pivot, target, r2):
    """Two points one ulp of y apart, the first a hit of `line` under `pose` and the second not:
    `target` (on the tube's surface in the line's frame) is carried to the cloud's frame by the pose
    and its y stepped one ulp at a time, away from the line while the oracle hits and towards it
    while it does not, until the oracle flips."""
    row = RO.pose_table([pose])[0]
    x, y, z = RO.apply_pose(target, pose, pivot)
    away = 1.0 if y > RO.apply_pose((target[0], 0.0, 0.0), pose, pivot)[1] else -1.0

    def hit(yy):
        return O.d2_min(RO.moved_point(x, yy, z, row, pivot), line) <= r2
    inside = hit(y)
    for _ in range(4096):
        nxt = float(np.nextafter(y, away * np.inf if inside else -away * np.inf))
        if hit(nxt) != inside:
            return ((x, y, z), (x, nxt, z)) if inside else ((x, nxt, z), (x, y, z))
        y = nxt
    raise AssertionError("boundary_pair: the oracle did not flip within 4096 ulps")


def hits_case():
    """radius 0.25.  Slice 0: _align_cases.hits_case (d2 == r2, on the line, one ulp outside, a
    zero-length segment, a one-vertex line, non-finite x y z I, qi == 0, two tubes) under its four
    shifts at theta = 0 and four real poses, pivot (0, 0).  Slice 1: line A alone about the pivot (2,
    -1) under two real poses and (0, 0, 0); its points are, per pose and side of the line, the pair on each side of
    the tube's surface that the oracle separates by one ulp."""
    b = C.hits_case()
    t0 = np.column_stack([b["shifts"], np.zeros(len(b["shifts"]))])
    t0 = np.concatenate([t0, [[0.0, 0.0, 0.05], [0.125, -0.25, -0.03125], [-3.0, 0.25, 0.1], [0.0, 0.0, -0.1]]])
    line_a = b["lines"][0][0]
    pivot1 = (2.0, -1.0)
    t1 = np.array([[0.1, -0.05, 0.03], [0.0, 0.0, 0.0], [-0.25, 0.125, -0.0625]])
    extra = []
    for pose, target in ((t1[0], (3.0, -0.25, 0.0)), (t1[0], (6.5, 0.25, 0.0)), (t1[2], (1.0, 0.25, 0.0))):
        inside, outside = boundary_pair(line_a, pose, pivot1, target, 0.0625)
        extra += [[*inside, 17.0], [*outside, 19.0]]
    extra += [[2.0, 0.0, 0.0, 20.0], [7.0, 0.1, 0.0, 11.0]]
    pts = np.concatenate([b["points"], np.array(extra)])
    base = {"points": pts, "slice_offsets": np.array([0, len(b["points"]), len(pts)], dtype=np.int64),
            "lines": [b["lines"][0], [line_a]], "kw": {"radius": 0.25}}
    return _case(base, np.concatenate([t0, t1]), [0, len(t0), len(t0) + len(t1)], [[0.0, 0.0], pivot1],
                 n_boundary_pairs=3)


def _yaws(rng, k):
    """k yaws within +-0.06 rad in 1/1024ths."""
    return np.round(rng.uniform(-0.06, 0.06, k) * 1024.0) / 1024.0


def _with_yaws(base, seed, pivots):
    rng = np.random.default_rng(seed)
    sh = base["shifts"]
    th = _yaws(rng, len(sh))
    th[(sh[:, 0] == 0.0) & (sh[:, 1] == 0.0)] = 0.0          # the tables keep their (0, 0, 0) rows
    return _case(base, np.column_stack([sh, th]), base["shift_offsets"], pivots)


def tiles_case():
    """_align_cases.tiles_case - 0 / 1 / 63 / 64 / 65 / 257 candidates under 16 / 1 / 15 / 16 / 17 / 17
    rows - with a yaw on every row but (0, 0) and the pivots at the middle of the line and beside it."""
    return _with_yaws(C.tiles_case(), 20, [[5.0, 0.0], [0.0, 0.0], [5.0, 1.0], [0.0, -2.0], [10.0, 0.5], [4.0, 0.25]])


def segtile_case():
    """_align_cases.segtile_case - 512 and 513 segments, a line that straddles the tile - under (0, 0,
    0) and a pose of 2 mrad about the middle of the 32 m zigzag."""
    b = C.segtile_case()
    poses = np.array([[0.0, 0.0, 0.0], [0.03125, -0.015625, 0.001953125]] * 3)
    return _case(b, poses, b["shift_offsets"], [[16.0, 0.0], [16.0, 0.0], [9.0, 0.5]])


def ragged_case():
    """_align_cases.ragged_case - six slices, one empty, lines without points, points without lines,
    two tables - with yaws and a non-zero pivot in every slice."""
    return _with_yaws(C.ragged_case(), 201, [[5.0, 0.125], [1.0, 1.0], [5.0, 0.25], [-3.0, 2.0], [4.0, 0.0], [5.0, 0.0]])


DESIGNED = {"hits": hits_case, "tiles": tiles_case}
SEEDED = {"segtile": segtile_case, "ragged": ragged_case}


@functools.lru_cache(maxsize=None)
def case(name):
    return dict(DESIGNED, **SEEDED)[name]()


def args(c):
    return c["points"], c["slice_offsets"], c["lines"], c["poses"], c["pose_offsets"], c["pivots"]


@functools.lru_cache(maxsize=None)
def expected(name, intensity_floor=0.0):
    """The oracle's tables for case(name): computed once per process."""
    c = case(name)
    return RO.rigid_scores(c["points"], c["slice_offsets"], c["lines"], RO.pose_table(c["poses"]), c["pose_offsets"],
                           c["pivots"], c["kw"].get("radius", C.RADIUS), intensity_floor)


@functools.lru_cache(maxsize=None)
def small_align(scope):
    """The oracle's two stages on _align_cases.small_frames (min_points = 8): once per process."""
    f = C.small_frames()
    return RO.align(f["points"], f["slice_offsets"], f["lines"], min_points=8, scope=scope)


# ------------------------------------------------------------------ the numpy restatement
def rigid_scores_np(points, slice_offsets, lines_per_slice, table, pose_offsets, pivots=None, radius=C.RADIUS,
                    intensity_floor=0.0, chunk=512):
    """The rule in numpy float64, one rounding per operation as numpy does.  table (K,4) = dx dy c s.
    Per slice and chunk of poses the moved points [P, k]; per line d2min [P, k], filled one segment
    at a time over the points inside that segment's own box (cost only; the box is expanded by a
    reach computed here: the sine bounds the yaw); then the integer sums."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 4)
    table = np.asarray(table, dtype=np.float64).reshape(-1, 4)
    n_s = len(slice_offsets) - 1
    pivots = np.zeros((n_s, 2)) if pivots is None else np.asarray(pivots, dtype=np.float64).reshape(n_s, 2)
    r2 = float(radius) * float(radius)
    out = {"score": np.zeros(len(table), dtype=np.int64), "hits": np.zeros(len(table), dtype=np.int64)}
    for s in range(n_s):
        p = pts[int(slice_offsets[s]):int(slice_offsets[s + 1])]
        k0, k1 = int(pose_offsets[s]), int(pose_offsets[s + 1])
        if len(p) == 0 or k1 == k0 or len(lines_per_slice[s]) == 0:
            continue
        with np.errstate(invalid="ignore"):
            wi = np.minimum(np.maximum(p[:, 3] - float(intensity_floor), 0.0), 4096.0)
        qi = np.where(np.isfinite(p[:, 3]), np.rint(np.nan_to_num(wi) * 256.0), 0.0).astype(np.int64)
        ok = np.isfinite(p[:, :3]).all(axis=1) & (qi > 0)
        p, qi = p[ok], qi[ok]
        lines = [np.asarray(v, dtype=np.float64).reshape(-1, 3) for v in lines_per_slice[s]]
        allv = np.concatenate(lines)
        px, py = float(pivots[s, 0]), float(pivots[s, 1])
        rho = float(np.hypot(allv[:, 0] - px, allv[:, 1] - py).max())
        for c0 in range(k0, k1, chunk):
            t = table[c0:min(c0 + chunk, k1)]
            yaw = 1.001 * float(np.arcsin(np.abs(t[:, 3]).max()))
            reach = float(radius) + float(np.abs(t[:, :2]).max()) + yaw * (rho + float(radius)) + 2.0 * C.GUARD
            # the rule's box is wider than any hitter needs: drop the points outside all of them first
            near = np.zeros(len(p), dtype=bool)
            for line in lines:
                if len(line) > 1:
                    near |= ((p[:, 0] >= line[:, 0].min() - reach) & (p[:, 0] <= line[:, 0].max() + reach)
                             & (p[:, 1] >= line[:, 1].min() - reach) & (p[:, 1] <= line[:, 1].max() + reach))
            q, qq = p[near], qi[near]
            gx = (q[:, 0][:, None] - t[None, :, 0]) - px
            gy = (q[:, 1][:, None] - t[None, :, 1]) - py
            wx = (t[None, :, 2] * gx + t[None, :, 3] * gy) + px
            wy = (t[None, :, 2] * gy - t[None, :, 3] * gx) + py
            score = np.zeros(len(t), dtype=np.int64)
            hits = np.zeros(len(t), dtype=np.int64)
            for line in lines:
                d2min = np.full(wx.shape, np.inf)
                for k in range(len(line) - 1):
                    a, e = line[k], line[k + 1] - line[k]
                    l2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
                    if not l2 > 0.0:
                        continue
                    lo = np.minimum(line[k], line[k + 1])[:2] - reach
                    hi = np.maximum(line[k], line[k + 1])[:2] + reach
                    sel = np.flatnonzero((q[:, 0] >= lo[0]) & (q[:, 0] <= hi[0]) & (q[:, 1] >= lo[1]) & (q[:, 1] <= hi[1]))
                    if len(sel) == 0:
                        continue
                    ux, uy = wx[sel], wy[sel]
                    uz = np.broadcast_to(q[sel, 2][:, None], ux.shape)
                    hx, hy, hz = ux - a[0], uy - a[1], uz - a[2]
                    u = np.minimum(np.maximum(((hx * e[0] + hy * e[1]) + hz * e[2]) / l2, 0.0), 1.0)
                    hx, hy, hz = ux - (a[0] + u * e[0]), uy - (a[1] + u * e[1]), uz - (a[2] + u * e[2])
                    d2min[sel] = np.minimum(d2min[sel], (hx * hx + hy * hy) + hz * hz)
                hit = d2min <= r2
                qk = np.rint((1.0 - np.where(hit, d2min, 0.0) / r2) * 1024.0).astype(np.int64)
                score += (np.where(hit, qk, 0) * qq[:, None]).sum(axis=0)
                hits += hit.sum(axis=0)
            out["score"][c0:c0 + len(t)] = score
            out["hits"][c0:c0 + len(t)] = hits
    return out


# ------------------------------------------------------------------ the analytic frame and the drive, yawed
def yawed_frame(yaw):
    """_align_cases.paint_frame with the detector's lines turned by yaw about the ego origin (the
    pivot) before they are moved by OFFSET: (points, [line, line])."""
    return C.paint_frame(yaw=yaw)


def lateral_residual(lines, pose):
    """The largest |y - lane| over the vertices of yawed_frame's lines moved by the pose (pivot (0,
    0)): the paint of the frame lies along x at LANE_Y."""
    worst = 0.0
    for v, y in zip(lines, C.LANE_Y):
        worst = max(worst, max(abs(RO.apply_pose(p, pose)[1] - y) for p in v))
    return worst


DRIVE_YAW = 0.015


def yawed_drive():
    """_align_cases.paint_drive's cloud and poses; every frame's pixels turned by DRIVE_YAW about the
    ego origin and then moved by OFFSET.  Returns (cloud, poses, pixels [frame][lane] (n,2))."""
    cloud, poses, pixels = C.paint_drive()
    c, s = math.cos(DRIVE_YAW), math.sin(DRIVE_YAW)
    out = []
    for frame in pixels:
        lanes = []
        for px in frame:
            ego = C.pixel_to_ego(px)
            x, y = ego[:, 0] - C.OFFSET[0], ego[:, 1] - C.OFFSET[1]
            ex, ey = c * x - s * y + C.OFFSET[0], s * x + c * y + C.OFFSET[1]
            lanes.append(np.stack([(25.0 - ey) / 0.05, (25.0 - ex) / 0.05], 1))
        out.append(lanes)
    return cloud, poses, out
