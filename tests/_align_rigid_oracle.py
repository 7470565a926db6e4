"""The rigid paint-alignment rule of include/pointnet_refine_hip.h ("Rigid paint alignment - the
rule") restated in Python ints and floats: a quadruple loop over every point, pose, line and segment,
no filter, no tiles, no vector operation.  Steps 1 and 3-5 are _align_oracle's own functions (weight,
d2_min, round_half_even); step 2' (the inverse pose), pick_pose, pose_grid, apply_pose and the two
stages of align_lines_rigid are restated here, independently of pointnet_refine_amd/align.py.  The
pose table is (K,4) = dx dy c s: the sine and cosine are inputs, as they are for the device."""
import math

import numpy as np

import _align_oracle as O

INF = float("inf")


def pose_table(poses):
    """(K,3) dx dy theta -> (K,4) dx dy cos(theta) sin(theta), Python's libm."""
    return np.array([[float(dx), float(dy), math.cos(float(th)), math.sin(float(th))] for dx, dy, th in poses],
                    dtype=np.float64).reshape(-1, 4)


def moved_point(x, y, z, row, pivot):
    """Step 2': the point under the inverse of the pose row (dx, dy, c, s)."""
    dx, dy, c, s = (float(v) for v in row)
    px, py = float(pivot[0]), float(pivot[1])
    gx = (x - dx) - px
    gy = (y - dy) - py
    wx = (c * gx + s * gy) + px
    wy = (c * gy - s * gx) + py
    return (wx, wy, z)


def slice_scores(points, lines, table, pivot, r2, intensity_floor, hitters=None):
    """Steps 1-5 for one slice: (score [K], hits [K]) as Python ints.  hitters: a set that receives
    the row of every point that hits any line at any pose."""
    score, hits = [0] * len(table), [0] * len(table)
    for row, p in enumerate(points):
        x, y, z, i = float(p[0]), float(p[1]), float(p[2]), float(p[3])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        qi = O.weight(i, intensity_floor)
        if qi == 0:
            continue
        for k, pose in enumerate(table):
            w = moved_point(x, y, z, pose, pivot)
            for line in lines:
                d2 = O.d2_min(w, line)
                if d2 <= r2:
                    score[k] += qi * O.round_half_even((1.0 - d2 / r2) * 1024.0)
                    hits[k] += 1
                    if hitters is not None:
                        hitters.add(row)
    return score, hits


def rigid_scores(points, slice_offsets, lines_per_slice, table, pose_offsets, pivots=None, radius=0.15,
                 intensity_floor=0.0):
    """The rule for every (slice, pose): {'score', 'hits'} int64 (K,).  table (K,4) = dx dy c s."""
    points = np.asarray(points)
    table = np.asarray(table, dtype=np.float64).reshape(-1, 4)
    n_s = len(slice_offsets) - 1
    pivots = np.zeros((n_s, 2)) if pivots is None else np.asarray(pivots, dtype=np.float64).reshape(n_s, 2)
    r2 = float(radius) * float(radius)
    out = {"score": np.zeros(len(table), dtype=np.int64), "hits": np.zeros(len(table), dtype=np.int64)}
    for s in range(n_s):
        k0, k1 = int(pose_offsets[s]), int(pose_offsets[s + 1])
        sc, ht = slice_scores(points[int(slice_offsets[s]):int(slice_offsets[s + 1])], lines_per_slice[s], table[k0:k1],
                              pivots[s], r2, float(intensity_floor))
        out["score"][k0:k1], out["hits"][k0:k1] = sc, ht
    return out


def pose_grid(centre, half, step, yaw_centre, yaw_half, yaw_step):
    """(K,3): the yaw index outer, then shift_grid's x outer and y inner."""
    n = int(round(yaw_half / yaw_step))
    sh = O.shift_grid(centre, half, step)
    return np.array([[x, y, float(yaw_centre) + j * yaw_step] for j in range(-n, n + 1) for x, y in sh],
                    dtype=np.float64).reshape(-1, 3)


def pick_pose(poses, score, hits, lever=25.0, min_points=32, keep=(63, 64), gain=(5, 4)):
    """Steps 6'-10: (pose (dx, dy, theta), aligned, score at (0, 0, 0), score at the near-best row)."""
    ps = [(float(a), float(b), float(c)) for a, b, c in poses]
    sc, ht = [int(v) for v in score], [int(v) for v in hits]
    k0 = next(k for k in range(len(ps)) if ps[k] == (0.0, 0.0, 0.0))
    best = max(sc)
    if best == 0 or ht[sc.index(best)] < min_points:
        return (0.0, 0.0, 0.0), False, sc[k0], sc[k0]
    row, short = -1, INF
    for k in range(len(ps)):
        if sc[k] * keep[1] >= best * keep[0]:
            lt = lever * ps[k][2]
            n2 = ps[k][0] * ps[k][0] + ps[k][1] * ps[k][1] + lt * lt
            if n2 < short:
                row, short = k, n2
    if not sc[row] * gain[1] > sc[k0] * gain[0]:
        return (0.0, 0.0, 0.0), False, sc[k0], sc[row]
    return ps[row], True, sc[k0], sc[row]


def apply_pose(vertex, pose, pivot=(0.0, 0.0)):
    """The picked pose applied to one vertex (x, y, z): Python floats."""
    dx, dy, th = (float(v) for v in pose)
    c, s = math.cos(th), math.sin(th)
    px, py = float(pivot[0]), float(pivot[1])
    gx, gy = float(vertex[0]) - px, float(vertex[1]) - py
    return (((c * gx - s * gy) + px) + dx, ((s * gx + c * gy) + py) + dy, float(vertex[2]))


def align(points, slice_offsets, lines_per_slice, scores=None, max_shift=1.0, max_yaw=0.02, lever=25.0, radius=0.15,
          intensity_floor=0.0, scope="frame", min_points=32, keep=(63, 64), gain=(5, 4), pivots=None):
    """The two stages of align_lines_rigid over `scores` (this module's loops when None, or any
    restatement with rigid_scores' signature): (poses (S,3), aligned [S], score_zero [S], score_best [S])."""
    scores = rigid_scores if scores is None else scores
    n_s = len(lines_per_slice)

    def stage(tables):
        off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
        res = scores(points, slice_offsets, lines_per_slice, pose_table(np.concatenate(tables)), off, pivots, radius,
                     intensity_floor)
        per = [([int(v) for v in res["score"][off[s]:off[s + 1]]], [int(v) for v in res["hits"][off[s]:off[s + 1]]])
               for s in range(n_s)]
        if scope == "drive":
            total = ([sum(p[0][k] for p in per) for k in range(len(tables[0]))],
                     [sum(p[1][k] for p in per) for k in range(len(tables[0]))])
            return [pick_pose(tables[0], *total, lever, min_points, keep, gain)] * n_s
        return [pick_pose(tables[s], *per[s], lever, min_points, keep, gain) for s in range(n_s)]

    first = stage([pose_grid((0.0, 0.0), max_shift, 0.1, 0.0, max_yaw, 0.004)] * n_s)
    fine_half = 0.004 if max_yaw > 0.0 else 0.0
    picks = stage([np.concatenate([pose_grid(p[0][:2], 0.1, 0.02, p[0][2], fine_half, 0.001), np.zeros((1, 3))])
                   for p in first])
    return (np.array([p[0] for p in picks], dtype=np.float64).reshape(n_s, 3), [p[1] for p in picks],
            [p[2] for p in picks], [p[3] for p in picks])
