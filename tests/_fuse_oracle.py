"""Map fusion - the rule of include/pointnet_refine_hip.h restated in plain numpy / Python floats,
steps 1-6, one loop per sentence of the rule so it can be read against the header.  Python floats
are IEEE doubles and every operation below rounds once, in the order the header gives.
"""
import math

import numpy as np


def default_origin(poses_xyzq):
    """The first pose's translation, each component rounded down to a multiple of 1000 m."""
    p = np.asarray(poses_xyzq, dtype=np.float64).reshape(-1, 7)
    return np.floor(p[0, :3] / 1000.0) * 1000.0 if len(p) else np.zeros(3)


def carrier_cum(verts):
    """cum[0] = 0, cum[k+1] = cum[k] + sqrt(|V[k+1] - V[k]|^2), sequentially."""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    cum = np.zeros(len(v))
    for k in range(len(v) - 1):
        e = v[k + 1] - v[k]
        cum[k + 1] = cum[k] + math.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return cum


def rotation(q):
    """R of the normalised quaternion qx qy qz qw, with the products the drive slicer forms."""
    x, y, z, w = (float(c) for c in q)
    nrm = math.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / nrm, y / nrm, z / nrm, w / nrm
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    return [[x2 - y2 - z2 + w2, 2.0 * (xy - zw), 2.0 * (xz + yw)],
            [2.0 * (xy + zw), -x2 + y2 - z2 + w2, 2.0 * (yz - xw)],
            [2.0 * (xz - yw), 2.0 * (yz + xw), -x2 - y2 + z2 + w2]]


def to_world(pieces, piece_pose, poses_shifted):
    """Step 1: w = R p + t, each component ((R0 p0 + R1 p1) + R2 p2) + t."""
    pieces = np.asarray(pieces, dtype=np.float64)
    out = np.zeros_like(pieces)
    for p in range(pieces.shape[0]):
        pose = poses_shifted[int(piece_pose[p])]
        r = rotation(pose[3:])
        for i in range(pieces.shape[1]):
            a = [float(c) for c in pieces[p, i]]
            for c in range(3):
                out[p, i, c] = ((r[c][0] * a[0] + r[c][1] * a[1]) + r[c][2] * a[2]) + float(pose[c])
    return out


def project_point(w, verts, cum):
    """Step 2 for one point: (s, d, seg, d2 of every usable segment as {k: d2})."""
    w = [float(c) for c in w]
    best, best_u, best_k, all_d2 = math.inf, 0.0, -1, {}
    for k in range(len(verts) - 1):
        a = [float(c) for c in verts[k]]
        b = [float(c) for c in verts[k + 1]]
        e = [b[0] - a[0], b[1] - a[1], b[2] - a[2]]
        l2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        if not l2 > 0.0:
            continue
        g = [w[0] - a[0], w[1] - a[1], w[2] - a[2]]
        u = min(max(((g[0] * e[0] + g[1] * e[1]) + g[2] * e[2]) / l2, 0.0), 1.0)
        h = [w[c] - (a[c] + u * e[c]) for c in range(3)]
        d2 = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]
        all_d2[k] = d2
        if d2 < best:
            best, best_u, best_k = d2, u, k
    if best_k < 0:
        h = [w[c] - float(verts[0][c]) for c in range(3)]
        return 0.0, math.sqrt((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2]), -1, all_d2
    c0, c1 = float(cum[best_k]), float(cum[best_k + 1])
    return c0 + best_u * (c1 - c0), math.sqrt(best), best_k, all_d2


def project(world, piece_line, lines_shifted, cums, return_d2=False):
    """Step 2 for every point of world (P,M,3): s, d (P,M) float64 and seg (P,M) int32."""
    n_p, m = world.shape[:2]
    s, d, seg = np.zeros((n_p, m)), np.zeros((n_p, m)), np.zeros((n_p, m), dtype=np.int32)
    d2s = []
    for p in range(n_p):
        l = int(piece_line[p])
        for i in range(m):
            s[p, i], d[p, i], seg[p, i], dd = project_point(world[p, i], lines_shifted[l], cums[l])
            d2s.append(dd)
    return (s, d, seg, d2s) if return_d2 else (s, d, seg)


def taper(i, m):
    """Step 3."""
    return float(min(i + 1, m - i))


def node_counts(cums, lines_shifted, ds):
    """Step 4: nodes per line."""
    return [int(math.floor(float(c[-1]) / ds)) + 1 if len(v) >= 1 else 0 for c, v in zip(cums, lines_shifted)]


def _contributions(pos, s_p, w_p):
    """Step 4 for one node and one piece: [(om, x)] in ascending i."""
    m = len(s_p)
    out = []
    for i in range(m - 1):
        sa, sb = float(s_p[i]), float(s_p[i + 1])
        if not (sb > sa and sa <= pos and pos < sb):
            continue
        u = (pos - sa) / (sb - sa)
        ta, tb = taper(i, m), taper(i + 1, m)
        om = ta + u * (tb - ta)
        x = [float(w_p[i][c]) + u * (float(w_p[i + 1][c]) - float(w_p[i][c])) for c in range(3)]
        out.append((om, x))
    return out


def gather(world, s, piece_line, n_lines, counts, ds):
    """Steps 3-5.  Pieces of a line are taken in the order they come in.  Returns X (N,3), W (N,),
    C (N,) int32, spread (N,), offsets (n_lines+1,)."""
    off = np.zeros(n_lines + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    n = int(off[-1])
    X, W, C, spread = np.zeros((n, 3)), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n)
    for l in range(n_lines):
        mine = [p for p in range(len(piece_line)) if int(piece_line[p]) == l]
        for j in range(counts[l]):
            pos = float(j) * ds
            contrib = []
            for p in mine:
                contrib += _contributions(pos, s[p], world[p])
            if not contrib:
                continue
            w_sum, acc = 0.0, [0.0, 0.0, 0.0]
            for om, x in contrib:
                w_sum = w_sum + om
                for c in range(3):
                    acc[c] = acc[c] + om * x[c]
            mean = [acc[c] / w_sum for c in range(3)]
            var = 0.0
            for om, x in contrib:
                h = [x[c] - mean[c] for c in range(3)]
                var = var + om * ((h[0] * h[0] + h[1] * h[1]) + h[2] * h[2])
            k = int(off[l]) + j
            X[k], W[k], C[k], spread[k] = mean, w_sum, len(contrib), math.sqrt(var / w_sum)
    return X, W, C, spread, off


def polylines(X, C, ds, min_count=1, max_gap=5.0):
    """Step 6 for the nodes of one line: list of (k,3) arrays."""
    runs, cur, last = [], [], None
    for j in range(len(C)):
        if C[j] < min_count:
            continue
        if last is not None and (j - last) * ds > max_gap:
            runs.append(cur)
            cur = []
        cur.append(j)
        last = j
    runs.append(cur)
    return [X[r].copy() for r in runs if len(r) >= 2]


def fuse(lines, pieces, piece_line, piece_pose, poses_xyzq, step=0.5, min_count=1, max_gap=5.0, origin=None):
    """The whole rule.  Pieces may come in any order; they are grouped by line, their order within a
    line kept.  Returns a dict: fused [per line list of (k,3)], world (P,M,3), s, d, seg (P,M) in
    the caller's piece order, X, W, C, spread and offsets of the nodes (X with the origin added
    back where C > 0)."""
    poses = np.asarray(poses_xyzq, dtype=np.float64).reshape(-1, 7)
    origin = default_origin(poses) if origin is None else np.asarray(origin, dtype=np.float64).reshape(3)
    shifted = [np.asarray(l, dtype=np.float64).reshape(-1, 3) - origin for l in lines]
    ps = poses.copy()
    ps[:, :3] -= origin
    cums = [carrier_cum(v) for v in shifted]
    pieces = np.asarray(pieces, dtype=np.float64)
    pieces = pieces.reshape(-1, pieces.shape[-2] if pieces.ndim >= 2 else 2, 3)
    world = to_world(pieces, piece_pose, ps)
    s, d, seg, d2s = project(world, piece_line, shifted, cums, return_d2=True)
    counts = node_counts(cums, shifted, step)
    X, W, C, spread, off = gather(world, s, piece_line, len(lines), counts, step)
    Xo = X.copy()
    Xo[C > 0] += origin
    fused = [polylines(Xo[off[l]:off[l + 1]], C[off[l]:off[l + 1]], step, min_count, max_gap) for l in range(len(lines))]
    return {"fused": fused, "world": world + origin, "world_shifted": world, "s": s, "d": d, "seg": seg, "X": Xo,
            "X_shifted": X, "W": W, "C": C, "spread": spread, "offsets": off, "origin": origin, "d2": d2s}


# ------------------------------------------------------------------ synthetic cases and margins
def quat_yaw_pitch(yaw, pitch):
    """Unit quaternion qx qy qz qw of a yaw about z followed by a pitch about the new y."""
    cy, sy, cp, sp = math.cos(yaw / 2), math.sin(yaw / 2), math.cos(pitch / 2), math.sin(pitch / 2)
    return np.array([-sy * sp, cy * sp, sy * cp, cy * cp])


def make_poses(n, base, rng, spacing=25.0):
    """n poses `spacing` metres apart along x from base (3,), with yaw and a small pitch."""
    out = np.zeros((n, 7))
    for k in range(n):
        out[k, :3] = np.asarray(base, dtype=np.float64) + [spacing * k, rng.uniform(-1, 1), rng.uniform(-0.2, 0.2)]
        out[k, 3:] = quat_yaw_pitch(rng.uniform(-0.6, 0.6), rng.uniform(-0.05, 0.05))
    return out


def curved_carrier(n, base, rng, length=100.0, lateral=0.0):
    """n vertices, about `length` metres along x from base, gently curved, unevenly spaced."""
    t = np.sort(rng.uniform(0.0, 1.0, n))
    t[0], t[-1] = 0.0, 1.0
    x = length * t
    a, ph = rng.uniform(1.0, 3.0), rng.uniform(0, 6.28)
    return np.stack([x, lateral + a * np.sin(x / 30.0 + ph), 0.3 * np.sin(x / 50.0)], 1) + np.asarray(base, dtype=np.float64)


def carrier_point(verts, cum, s):
    """The carrier at arc position s; beyond its ends the end segments are continued."""
    verts = np.asarray(verts, dtype=np.float64)
    if len(verts) < 2 or cum[-1] <= 0:
        return verts[0] + np.array([s, 0.0, 0.0])
    k = int(np.clip(np.searchsorted(cum, s, side="right") - 1, 0, len(verts) - 2))
    while cum[k + 1] <= cum[k] and k + 2 < len(verts):
        k += 1
    while cum[k + 1] <= cum[k] and k > 0:
        k -= 1
    return verts[k] + (s - cum[k]) / (cum[k + 1] - cum[k]) * (verts[k + 1] - verts[k])


def to_ego(world, pose):
    """The inverse of step 1 in numpy (test inputs only)."""
    r = np.array(rotation(pose[3:]))
    return (np.asarray(world) - pose[:3]) @ r


def make_piece(verts, pose, s_values, rng, noise):
    """A piece in the ego frame of pose: the carrier at s_values plus N(0, noise) per component."""
    cum = carrier_cum(verts)
    w = np.stack([carrier_point(verts, cum, float(s)) for s in s_values])
    return to_ego(w + rng.normal(0.0, noise, w.shape) if noise > 0 else w, pose)


def margins(lines_shifted, cums, world, piece_line, s, step, d2s=None):
    """(node margin, segment margin): the smallest distance of a node position to any s of a piece
    that is not exactly 0 or cum_total, and the smallest lead in d2 of a point's best segment over
    every segment not next to it (segments of zero length do not count as being in between).  inf
    where nothing competes.  d2s: project's per-point {segment: d2} when it is at hand (fuse()["d2"])."""
    node_m, seg_m = math.inf, math.inf
    for p in range(world.shape[0]):
        l = int(piece_line[p])
        total = float(cums[l][-1]) if len(cums[l]) else 0.0
        for i in range(world.shape[1]):
            v = float(s[p, i])
            if v != 0.0 and v != total:
                node_m = min(node_m, abs(v - round(v / step) * step))
            d2 = d2s[p * world.shape[1] + i] if d2s is not None else project_point(world[p, i], lines_shifted[l], cums[l])[3]
            if not d2:
                continue
            vals = [d2[kk] for kk in sorted(d2)]               # usable segments in carrier order
            r = min(range(len(vals)), key=vals.__getitem__)    # the first smallest
            rest = vals[:max(r - 1, 0)] + vals[r + 2:]
            if rest:
                seg_m = min(seg_m, min(rest) - vals[r])
    return node_m, seg_m
