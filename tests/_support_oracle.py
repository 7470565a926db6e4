"""Cloud support - the rule of include/pointnet_refine_hip.h restated in plain Python floats, one
loop per sentence of the rule so it can be read against the header.  Python floats are IEEE doubles
and every operation below rounds once, in the order the header gives.  There is no grid here:
every segment of every line for every point.
"""
import math

import numpy as np

from _fuse_oracle import carrier_cum, project_point


def default_origin(lines):
    """The first vertex of the first line that has one, each component rounded down to 1000 m."""
    for l in lines:
        v = np.asarray(l, dtype=np.float64).reshape(-1, 3)
        if len(v):
            return np.floor(v[0] / 1000.0) * 1000.0
    return np.zeros(3)


def node_counts(cums, step):
    """Nodes per line: floor(cum_total / step) + 1 with a vertex, else 0."""
    return [int(math.floor(float(c[-1]) / step)) + 1 if len(c) else 0 for c in cums]


def _half(x):
    """Distance of x to the nearest half-integer."""
    return abs((x - math.floor(x)) - 0.5)


def hit(w, intensity, verts, cum, n_nodes, step, r2, intensity_floor):
    """Steps 1-7 for one shifted point and one line: None without a usable segment, else a dict
    with d2, seg, lead (the best segment's lead over every segment not next to it) and, if d2 <= r2,
    'node', 'qi', 'qt', 'qz', 'clamped' and the unrounded 'pos' = s / step + 0.5, 't', 'hz', 'wi'."""
    s, _, k, all_d2 = project_point(w, verts, cum)                         # 1. projection
    if k < 0:
        return None
    vals = [all_d2[kk] for kk in sorted(all_d2)]
    r = sorted(all_d2).index(k)
    rest = vals[:max(r - 1, 0)] + vals[r + 2:]
    out = {"d2": all_d2[k], "seg": k, "lead": min(rest) - vals[r] if rest else math.inf, "hit": all_d2[k] <= r2}
    if not out["hit"]:                                                     # 2. hit
        return out
    w = [float(c) for c in w]
    a = [float(c) for c in verts[k]]
    b = [float(c) for c in verts[k + 1]]
    e = [b[0] - a[0], b[1] - a[1], b[2] - a[2]]
    l2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    g = [w[0] - a[0], w[1] - a[1], w[2] - a[2]]
    u = min(max(((g[0] * e[0] + g[1] * e[1]) + g[2] * e[2]) / l2, 0.0), 1.0)
    pos = s / step + 0.5                                                   # 3. station
    raw = int(math.floor(pos))
    exy2 = e[0] * e[0] + e[1] * e[1]                                       # 4. lateral offset
    t = (e[0] * g[1] - e[1] * g[0]) / math.sqrt(exy2) if exy2 > 0.0 else 0.0
    hz = w[2] - (a[2] + u * e[2])                                          # 5. height
    wi = min(max(float(intensity) - intensity_floor, 0.0), 4096.0)         # 6. weight
    out.update(node=min(raw, n_nodes - 1), clamped=raw > n_nodes - 1, pos=pos, t=t, hz=hz, wi=wi,
               qi=round(wi * 256.0), qt=round(t * 65536.0), qz=round(hz * 65536.0))    # 7. round-half-even
    return out


def support(cloud, lines, step=0.5, radius=0.3, intensity_floor=0.0, origin=None):
    """The whole rule.  cloud (T,4) float32, lines a list of (n,3).  Returns {'acc' (N,8) int64,
    'offsets', 'origin', 'hits': [(point, row, qi, qt, qz)] in point order, then line order,
    'margins': {'d2', 'station', 'lead', 'quant'}} (inf where nothing competes)."""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    origin = default_origin(lines) if origin is None else np.asarray(origin, dtype=np.float64).reshape(3)
    shifted = [np.asarray(l, dtype=np.float64).reshape(-1, 3) - origin for l in lines]
    cums = [carrier_cum(v) for v in shifted]
    counts = node_counts(cums, step)
    off = np.zeros(len(lines) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    r2 = radius * radius
    m = {"d2": math.inf, "station": math.inf, "lead": math.inf, "quant": math.inf}
    hits = []
    for i in range(len(cloud)):
        p = [float(c) for c in cloud[i]]
        if not all(math.isfinite(c) for c in p):
            continue
        w = [p[c] - float(origin[c]) for c in range(3)]
        for l in range(len(lines)):
            if len(shifted[l]) < 2:
                continue
            h = hit(w, p[3], shifted[l], cums[l], counts[l], step, r2, intensity_floor)
            if h is None:
                continue
            m["d2"] = min(m["d2"], abs(h["d2"] - r2))
            if not h["hit"]:
                continue
            m["lead"] = min(m["lead"], h["lead"])
            if not h["clamped"]:
                m["station"] = min(m["station"], abs(h["pos"] - round(h["pos"])))
            m["quant"] = min(m["quant"], _half(h["t"] * 65536.0), _half(h["hz"] * 65536.0), _half(h["wi"] * 256.0))
            hits.append((i, int(off[l]) + h["node"], h["qi"], h["qt"], h["qz"]))
    return {"acc": accumulate(hits, int(off[-1])), "offsets": off, "origin": origin, "hits": hits, "margins": m}


def accumulate(hits, n_nodes, points=None):
    """Step 8 over the hits of the first `points` points (None: all), in Python integers."""
    acc = [[0] * 8 for _ in range(n_nodes)]
    for i, row, qi, qt, qz in hits:
        if points is not None and i >= points:
            continue
        a = acc[row]
        a[0] += 1
        a[1] += 1 if qi > 0 else 0
        a[2] += qi
        a[3] += qt
        a[4] += qt * qt
        a[5] += qi * qt
        a[6] += qz
    return np.array(acc, dtype=np.int64).reshape(n_nodes, 8)


def support_numpy(cloud, lines, step=0.5, radius=0.3, intensity_floor=0.0, origin=None):
    """The same rule vectorised over the points (numpy, one rounding per operation as above): still
    every segment for every point, no grid.  Returns (acc, offsets)."""
    cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 4)
    origin = default_origin(lines) if origin is None else np.asarray(origin, dtype=np.float64).reshape(3)
    shifted = [np.asarray(l, dtype=np.float64).reshape(-1, 3) - origin for l in lines]
    cums = [carrier_cum(v) for v in shifted]
    counts = node_counts(cums, step)
    off = np.zeros(len(lines) + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    acc = np.zeros((int(off[-1]), 8), dtype=np.int64)
    keep = np.isfinite(cloud).all(1)
    w = cloud[keep, :3].astype(np.float64) - origin
    inten = cloud[keep, 3].astype(np.float64)
    r2 = radius * radius
    for l, v in enumerate(shifted):
        best = np.full(len(w), np.inf)
        best_u, best_hz, best_k = np.zeros(len(w)), np.zeros(len(w)), np.full(len(w), -1, dtype=np.int64)
        for k in range(len(v) - 1):
            a, e = v[k], v[k + 1] - v[k]
            l2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
            if not l2 > 0.0:
                continue
            g = w - a
            u = np.minimum(np.maximum(((g[:, 0] * e[0] + g[:, 1] * e[1]) + g[:, 2] * e[2]) / l2, 0.0), 1.0)
            h0, h1, h2 = w[:, 0] - (a[0] + u * e[0]), w[:, 1] - (a[1] + u * e[1]), w[:, 2] - (a[2] + u * e[2])
            d2 = (h0 * h0 + h1 * h1) + h2 * h2
            better = d2 < best
            best, best_u = np.where(better, d2, best), np.where(better, u, best_u)
            best_hz, best_k = np.where(better, h2, best_hz), np.where(better, k, best_k)
        sel = np.flatnonzero((best_k >= 0) & (best <= r2))
        if len(sel) == 0:
            continue
        k, u = best_k[sel], best_u[sel]
        a, e = v[k], v[k + 1] - v[k]
        s = cums[l][k] + u * (cums[l][k + 1] - cums[l][k])
        j = np.minimum(np.floor(s / step + 0.5).astype(np.int64), counts[l] - 1)
        g = w[sel] - a
        exy2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        flat = exy2 > 0.0
        t = np.where(flat, (e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]) / np.sqrt(np.where(flat, exy2, 1.0)), 0.0)
        wi = np.minimum(np.maximum(inten[sel] - intensity_floor, 0.0), 4096.0)
        qi, qt = np.rint(wi * 256.0).astype(np.int64), np.rint(t * 65536.0).astype(np.int64)
        qz = np.rint(best_hz[sel] * 65536.0).astype(np.int64)
        for c, val in enumerate((np.ones_like(qi), (qi > 0).astype(np.int64), qi, qt, qt * qt, qi * qt, qz)):
            np.add.at(acc[:, c], off[l] + j, val)
    return acc, off
