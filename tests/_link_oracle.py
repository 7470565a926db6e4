"""Piece linking - the rule of include/pointnet_refine_hip.h restated in plain Python floats, steps
1-7 (and step 8 through _fuse_oracle.fuse), one loop per sentence of the rule so it can be read
against the header.  Projection, gather and the synthetic helpers are _fuse_oracle's.
"""
import math

import numpy as np

import _fuse_oracle as O


def boxes(world):
    """Step 1: lo, hi (P,3)."""
    n_p, m = world.shape[:2]
    lo, hi = np.zeros((n_p, 3)), np.zeros((n_p, 3))
    for p in range(n_p):
        for c in range(3):
            lo[p, c] = min(float(world[p, k, c]) for k in range(m))
            hi[p, c] = max(float(world[p, k, c]) for k in range(m))
    return lo, hi


def candidates(lo, hi, frame, gate, slack=None):
    """Step 2: [(i, j)] by ascending i, then ascending j.  slack: a list that takes |difference| of
    every box comparison made."""
    out = []
    n_p = len(lo)
    for i in range(n_p):
        for j in range(i + 1, n_p):
            if int(frame[i]) == int(frame[j]):
                continue
            ok = True
            for c in range(3):
                a, b = float(lo[i, c]) - gate, float(hi[j, c])
                e, f = float(lo[j, c]) - gate, float(hi[i, c])
                if slack is not None:
                    slack.append(abs(a - b))
                    slack.append(abs(e - f))
                if not (a <= b and e <= f):
                    ok = False
            if ok:
                out.append((i, j))
    return out


def usable(verts):
    """The segments of a polyline with L2 > 0, in order."""
    out = []
    for k in range(len(verts) - 1):
        e = [float(verts[k + 1][c]) - float(verts[k][c]) for c in range(3)]
        if (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] > 0.0:
            out.append(k)
    return out


def raw_u(w, verts, k):
    """The unclamped u of point w on segment k."""
    a = [float(c) for c in verts[k]]
    e = [float(verts[k + 1][c]) - a[c] for c in range(3)]
    g = [float(w[c]) - a[c] for c in range(3)]
    return ((g[0] * e[0] + g[1] * e[1]) + g[2] * e[2]) / ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])


def directed(A, cum_a, B, cum_b, gate, track=None):
    """Step 3, a -> b: [(d, cum_a[k], s_b, e_a . e_b)] of the points that are in, in ascending k, and
    n_out.  track: a dict of lists 'gate', 'end', 'seg' that takes the margins of every point."""
    m = len(A)
    segs = usable(B)
    ins, n_out = [], 0
    for k in range(m):
        s_b, d, seg, d2 = O.project_point(A[k], B, cum_b)
        if track is not None and d2:
            vals = [d2[kk] for kk in sorted(d2)]
            r = min(range(len(vals)), key=vals.__getitem__)
            rest = vals[:max(r - 1, 0)] + vals[r + 2:]
            if rest:
                track["seg"].append(min(rest) - vals[r])
        if seg < 0:
            continue                                   # b has no usable segment
        a0 = [float(c) for c in B[seg]]
        e_b = [float(B[seg + 1][c]) - a0[c] for c in range(3)]
        ru = raw_u(A[k], B, seg)
        u = min(max(ru, 0.0), 1.0)                     # the u project_point used
        if track is not None:
            if seg == segs[0]:
                track["end"].append(abs(ru))
            if seg == segs[-1]:
                track["end"].append(abs(ru - 1.0))
        if (seg == segs[0] and u == 0.0) or (seg == segs[-1] and u == 1.0):
            continue                                   # end-clamped: beyond b
        if track is not None:
            track["gate"].append(abs(d - gate))
        if d <= gate:
            q = min(k, m - 2)
            e_a = [float(A[q + 1][c]) - float(A[q][c]) for c in range(3)]
            ins.append((d, float(cum_a[k]), s_b, (e_a[0] * e_b[0] + e_a[1] * e_b[1]) + e_a[2] * e_b[2]))
        else:
            n_out += 1
    return ins, n_out


def pair_stats(world, cum, i, j, gate, track=None):
    """Step 4: (n_in, n_out, sum_d, sum_self, sum_other, sum_dot) of the pair (i, j)."""
    fwd, out_f = directed(world[i], cum[i], world[j], cum[j], gate, track)
    bwd, out_b = directed(world[j], cum[j], world[i], cum[i], gate, track)
    sum_d = sum_self = sum_other = sum_dot = 0.0
    for d, ca, sb, dot in fwd:
        sum_d, sum_self, sum_other, sum_dot = sum_d + d, sum_self + ca, sum_other + sb, sum_dot + dot
    for d, ca, sb, dot in bwd:
        sum_d, sum_self, sum_other, sum_dot = sum_d + d, sum_self + sb, sum_other + ca, sum_dot + dot
    return len(fwd) + len(bwd), out_f + out_b, sum_d, sum_self, sum_other, sum_dot


def edge_of(n_in, n_out, sum_self, sum_other, sum_dot, min_in, out_ratio):
    """Step 5 for one candidate: (edge, rho, delta); delta is 0 where n_in is 0."""
    rho = 1 if sum_dot >= 0.0 else -1
    delta = (sum_self - rho * sum_other) / float(n_in) if n_in > 0 else 0.0
    return n_in >= min_in and out_ratio * n_out <= n_in, rho, delta


def link(world, frame, gate=1.0, min_in=4, out_ratio=4, track=None):
    """Steps 1-5 on shifted drive-frame pieces (P,M,3).  The dict link_pieces returns, plus 'cum'."""
    world = np.asarray(world, dtype=np.float64)
    cum = np.stack([O.carrier_cum(p) for p in world]) if len(world) else np.zeros(world.shape[:2])
    lo, hi = boxes(world)
    pairs = candidates(lo, hi, frame, gate, track["box"] if track is not None else None)
    rows = [pair_stats(world, cum, i, j, gate, track) for i, j in pairs]
    res = {"pairs": np.array(pairs, dtype=np.int64).reshape(-1, 2), "cum": cum}
    for c, (k, t) in enumerate((("n_in", np.int32), ("n_out", np.int32), ("sum_d", np.float64), ("sum_self", np.float64),
                                ("sum_other", np.float64), ("sum_dot", np.float64))):
        res[k] = np.array([r[c] for r in rows], dtype=t)
    edges = [edge_of(r[0], r[1], r[3], r[4], r[5], min_in, out_ratio) for r in rows]
    res["edge"] = np.array([e[0] for e in edges], dtype=bool)
    res["rho"] = np.array([e[1] for e in edges], dtype=np.int8)
    res["delta"] = np.array([e[2] for e in edges], dtype=np.float64)
    if track is not None:
        track["dot"] += [abs(float(r[5])) for r, e in zip(rows, edges) if e[0]]
    return res


def sync(n_pieces, links):
    """Step 6 up to the offsets: cluster, level, parent, sign, offset per piece."""
    nbr = [[] for _ in range(n_pieces)]                # (neighbour, n_in, rho, delta, this piece is the edge's i)
    for e in range(len(links["pairs"])):
        if not links["edge"][e]:
            continue
        i, j = int(links["pairs"][e][0]), int(links["pairs"][e][1])
        n_in, rho, delta = int(links["n_in"][e]), int(links["rho"][e]), float(links["delta"][e])
        nbr[i].append((j, n_in, rho, delta, True))
        nbr[j].append((i, n_in, rho, delta, False))
    cluster, level, parent = [-1] * n_pieces, [-1] * n_pieces, [-1] * n_pieces
    sign, offset = [1] * n_pieces, [0.0] * n_pieces
    n_clusters = 0
    for root in range(n_pieces):                       # ascending: an unvisited piece is its cluster's smallest
        if cluster[root] >= 0:
            continue
        cluster[root], level[root] = n_clusters, 0
        front, depth = [root], 0
        while front:
            reach = sorted({b for a in front for b, _, _, _, _ in nbr[a] if cluster[b] < 0})
            depth += 1
            for b in reach:
                best = None
                for a, n_in, rho, delta, b_is_i in nbr[b]:
                    if cluster[a] == n_clusters and level[a] == depth - 1:
                        if best is None or n_in > best[1] or (n_in == best[1] and a < best[0]):
                            best = (a, n_in, rho, delta, b_is_i)
                a, _, rho, delta, b_is_i = best
                parent[b], sign[b] = a, rho * sign[a]
                # the parent is the edge's i exactly when the child is not
                offset[b] = offset[a] + sign[a] * delta if not b_is_i else offset[a] - sign[b] * delta
            for b in reach:
                cluster[b], level[b] = n_clusters, depth
            front = reach
        n_clusters += 1
    return {"cluster": np.array(cluster, dtype=np.int64), "level": np.array(level, dtype=np.int64),
            "parent": np.array(parent, dtype=np.int64), "sign": np.array(sign, dtype=np.int8),
            "offset": np.array(offset, dtype=np.float64)}


def arc(cum, s):
    """Step 6's last sentences: g (P,M), reversed where sign < 0, minus the cluster's smallest."""
    n_p, m = cum.shape
    g = np.zeros((n_p, m))
    for p in range(n_p):
        row = [float(s["offset"][p]) + float(s["sign"][p]) * float(cum[p, k]) for k in range(m)]
        g[p] = row[::-1] if s["sign"][p] < 0 else row
    for c in range(int(s["cluster"].max()) + 1 if n_p else 0):
        mine = [p for p in range(n_p) if s["cluster"][p] == c]
        low = min(float(g[p, k]) for p in mine for k in range(m))
        for p in mine:
            g[p] = g[p] - low
    return g


def fuse_unmatched(pieces, piece_pose, poses_xyzq, gate=1.0, min_in=4, out_ratio=4, min_pieces=2, step=0.5, min_count=1,
                   max_gap=5.0, origin=None, track=None):
    """Steps 1-8.  Returns a dict: links, cluster (kept cluster per piece, -1 dropped), clusters_all,
    sign, offset, level, parent, g, carriers, kept and 'map', _fuse_oracle.fuse's dict of step 8."""
    poses = np.asarray(poses_xyzq, dtype=np.float64).reshape(-1, 7)
    origin = O.default_origin(poses) if origin is None else np.asarray(origin, dtype=np.float64).reshape(3)
    ps = poses.copy()
    ps[:, :3] -= origin
    pieces = np.asarray(pieces, dtype=np.float64)
    n_p = len(pieces)
    world = O.to_world(pieces, piece_pose, ps)
    links = link(world, piece_pose, gate, min_in, out_ratio, track)
    s = sync(n_p, links)
    g = arc(links["cum"], s)
    turned, ego = world.copy(), pieces.copy()
    for p in range(n_p):
        if s["sign"][p] < 0:
            turned[p], ego[p] = world[p, ::-1], pieces[p, ::-1]
    # step 7: clusters of at least min_pieces pieces, gathered with s := g, one line per cluster
    n_all = int(s["cluster"].max()) + 1 if n_p else 0
    big = [c for c in range(n_all) if int((s["cluster"] == c).sum()) >= min_pieces]
    line = np.array([big.index(c) if c in big else -1 for c in s["cluster"]], dtype=np.int64)
    sel = [p for p in range(n_p) if line[p] >= 0]
    counts = [int(math.floor(max(float(g[p].max()) for p in sel if line[p] == l) / step)) + 1 for l in range(len(big))]
    X, W, C, spread, off = O.gather(turned[sel], g[sel], line[sel], len(big), counts, step)
    drafts = [X[off[l]:off[l + 1]][C[off[l]:off[l + 1]] >= 1] for l in range(len(big))]
    final, carriers = {}, []
    for l, d in enumerate(drafts):
        if len(d) >= 2:
            final[l] = len(carriers)
            carriers.append(d + origin)
    cluster = np.array([final.get(int(l), -1) for l in line], dtype=np.int64)
    kept = np.flatnonzero(cluster >= 0)
    fused = O.fuse(carriers, ego[kept], cluster[kept], np.asarray(piece_pose)[kept], poses, step, min_count, max_gap, origin)
    return {"links": links, "cluster": cluster, "clusters_all": s["cluster"], "sign": s["sign"], "offset": s["offset"],
            "level": s["level"], "parent": s["parent"], "g": g, "carriers": carriers, "kept": kept, "map": fused,
            "world_shifted": world, "origin": origin}


def new_track():
    return {"gate": [], "end": [], "seg": [], "box": [], "dot": []}


def margins(track):
    """The smallest of, over a case run with track=new_track(): |d - gate| of interior points, the
    distance of the unclamped u from 0 on a winning first segment and from 1 on a winning last one,
    the lead in d2 of the best segment over non-adjacent ones, the slack of every box comparison,
    |sum_dot| of edges.  inf where nothing competes."""
    return {k: min(v) if v else math.inf for k, v in track.items()}


# ------------------------------------------------------------------ the synthetic drive of the fixture
def lane_points(lat, x):
    """(n,3): the lane at lateral position lat, y = lat + 2 sin(x / 30 + 1), z = 0.3 sin(x / 50)."""
    x = np.asarray(x, dtype=np.float64)
    return np.stack([x, lat + 2.0 * np.sin(x / 30.0 + 1.0), 0.3 * np.sin(x / 50.0)], 1)


LANES = (-3.5, 0.0, 3.5, 12.0)
LANE_LENGTH = 260.0


def lane_polyline(lat, base, n=1041):
    return lane_points(lat, np.linspace(0.0, LANE_LENGTH, n)) + np.asarray(base, dtype=np.float64)


def make_case(seed, base, n_poses=20, spacing=10.0, m=32, noise=0.05, lanes=LANES, permute=True):
    """The fixture's drive: lanes of 260 m seen from n_poses poses `spacing` m apart; every lane is
    clipped to ego |x| <= 25 per pose and resampled to m points (uniform in lane x) with N(0, noise)
    per component; every third piece is reversed; in every frame one lane of the four (frame number
    modulo 4) comes as two fragments (0-40 % and 55-100 % of its span); the piece order is permuted.
    Returns (pieces (P,m,3) ego, piece_pose (P,), poses (S,7), truth (P,) lane of each piece)."""
    rng = np.random.default_rng(seed)
    base = np.asarray(base, dtype=np.float64)
    poses = O.make_poses(n_poses, base + [30.0, 0.0, 0.0], rng, spacing=spacing)
    xs = np.linspace(0.0, LANE_LENGTH, 2601)
    pieces, piece_pose, truth = [], [], []
    for f in range(n_poses):
        split = lanes[f % len(lanes)]
        for l, lat in enumerate(lanes):
            pts = lane_points(lat, xs) + base
            inside = np.abs(O.to_ego(pts, poses[f])[:, 0]) <= 25.0
            if inside.sum() < 2:
                continue
            x0, x1 = xs[inside][0], xs[inside][-1]
            spans = [(x0, x1)] if lat != split else [(x0, x0 + 0.40 * (x1 - x0)), (x0 + 0.55 * (x1 - x0), x1)]
            for a, b in spans:
                w = lane_points(lat, np.linspace(a, b, m)) + base
                pieces.append(O.to_ego(w + rng.normal(0.0, noise, w.shape), poses[f]))
                piece_pose.append(f)
                truth.append(l)
    pieces = np.stack(pieces)
    pieces[::3] = pieces[::3, ::-1]
    order = rng.permutation(len(pieces)) if permute else np.arange(len(pieces))
    return pieces[order], np.array(piece_pose)[order], poses, np.array(truth)[order]


def distance_to_lane(points, lat, base):
    """Distance of every point of (n,3) to the true lane (a dense polyline of it)."""
    line = lane_polyline(lat, base, 2601)
    best = np.full(len(points), np.inf)
    for a, b in zip(line[:-1], line[1:]):
        e = b - a
        u = np.clip(((points - a) @ e) / (e @ e), 0.0, 1.0)
        best = np.minimum(best, np.linalg.norm(points - (a + u[:, None] * e), axis=1))
    return best
