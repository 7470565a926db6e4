"""The ground-lift rule of include/pointnet_refine_hip.h ("Ground lift - the rule") restated in Python
ints and floats: brute force over all points of a query's slice, no grid, no vector operation.  A
Python float is an IEEE double and every expression below is one rounding per operation, so this is
the rule as the header words it.  line_stations and the host lift are restated here as well,
independently of pointnet_refine_amd/ground.py."""
import math

import numpy as np

NAN = float("nan")


def ground_query(points, qx, qy, r2, z_lo, bin, n_bins, min_points, peak_num, peak_den):
    """One query over the (n,4) points of its slice: (height, count, hits, bin)."""
    hist = [0] * n_bins
    kept = []                                   # (b, z) of the binned hits
    hits = 0
    for row in points:
        x, y, z = float(row[0]), float(row[1]), float(row[2])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        dx = x - qx
        dy = y - qy
        d2 = dx * dx + dy * dy
        if not d2 <= r2:
            continue
        hits += 1
        b = math.floor((z - z_lo) / bin)
        if 0 <= b < n_bins:
            hist[b] += 1
            kept.append((b, z))
    c3 = [(hist[b - 1] if b > 0 else 0) + hist[b] + (hist[b + 1] if b + 1 < n_bins else 0) for b in range(n_bins)]
    peak = max(c3)
    if peak < min_points:
        return NAN, 0, hits, -1
    thr = max(min_points, -((-peak * peak_num) // peak_den))
    g = next(b for b in range(n_bins) if c3[b] >= thr)
    while g + 1 < n_bins and c3[g + 1] > c3[g]:
        g += 1
    total, n = 0, 0
    for b, z in kept:
        if g - 1 <= b <= g + 1:
            total += int(round_half_even(z * 65536.0))
            n += 1
    return (float(total) / float(n)) / 65536.0, n, hits, g


def round_half_even(v):
    """rint of a finite double as a Python int."""
    f = math.floor(v)
    d = v - f                                   # exact for |v| < 2^52
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        return f + 1
    return f


def ground_heights(points, slice_offsets, queries, query_offsets, radius=0.5, min_points=5, peak_share=(1, 2), z_lo=-8.0,
                   bin=0.0625, n_bins=256):
    """The rule for every query: {'height' float64, 'count', 'hits', 'bin' int32}.  r2 is computed
    once, here, as the host does."""
    points = np.asarray(points)
    queries = np.asarray(queries, dtype=np.float64).reshape(-1, 2)
    r2 = float(radius) * float(radius)
    n_q = len(queries)
    out = {"height": np.full(n_q, np.nan), "count": np.zeros(n_q, dtype=np.int32), "hits": np.zeros(n_q, dtype=np.int32),
           "bin": np.full(n_q, -1, dtype=np.int32)}
    for s in range(len(slice_offsets) - 1):
        pts = points[int(slice_offsets[s]):int(slice_offsets[s + 1])]
        for q in range(int(query_offsets[s]), int(query_offsets[s + 1])):
            h, n, hits, g = ground_query(pts, float(queries[q, 0]), float(queries[q, 1]), r2, float(z_lo), float(bin),
                                         int(n_bins), int(min_points), int(peak_share[0]), int(peak_share[1]))
            out["height"][q], out["count"][q], out["hits"][q], out["bin"][q] = h, n, hits, g
    return out


def vertex_arcs(v):
    cum = [0.0]
    for k in range(1, len(v)):
        dx = float(v[k][0]) - float(v[k - 1][0])
        dy = float(v[k][1]) - float(v[k - 1][1])
        cum.append(cum[-1] + math.sqrt(dx * dx + dy * dy))
    return np.array(cum[:len(v)], dtype=np.float64)


def line_stations(lines, step=1.0):
    """(xy (N,2), arc (N,), offsets (L+1,)): stations at j * step, j = 0 .. floor(total / step), plus
    total if it is not the last; one station at the first vertex for a line of one vertex or of
    zero xy length; none for a line without a vertex."""
    xy, arc, off = [], [], [0]
    for v in lines:
        v = np.asarray(v, dtype=np.float64)
        if len(v) == 0:
            off.append(off[-1])
            continue
        cum = vertex_arcs(v)
        total = float(cum[-1])
        if not total > 0.0:
            s = [0.0]
        else:
            s = [j * float(step) for j in range(int(math.floor(total / float(step))) + 1)]
            if s[-1] != total:
                s.append(total)
        for sj in s:
            arc.append(sj)
            if total > 0.0:
                xy.append([float(np.interp(sj, cum, v[:, 0])), float(np.interp(sj, cum, v[:, 1]))])
            else:
                xy.append([float(v[0, 0]), float(v[0, 1])])
        off.append(off[-1] + len(s))
    return np.array(xy, dtype=np.float64).reshape(-1, 2), np.array(arc, dtype=np.float64), np.array(off, dtype=np.int64)


def lift(lines, arc, offsets, height):
    """The host rule: per line z(vertex) = interp(vertex arc, s[valid], h[valid]), the end values
    held outside; a line with no valid station unchanged.  Returns (lines, lifted flags)."""
    out, flags = [], []
    for l, v in enumerate(lines):
        v = np.array(v, dtype=np.float64).reshape(-1, 3)
        s = [float(a) for a in arc[offsets[l]:offsets[l + 1]]]
        h = [float(a) for a in height[offsets[l]:offsets[l + 1]]]
        ok = [k for k in range(len(s)) if math.isfinite(h[k])]
        if len(v) and ok:
            sv, hv = [s[k] for k in ok], [h[k] for k in ok]
            for i, a in enumerate(vertex_arcs(v)):
                v[i, 2] = np.interp(float(a), sv, hv)
        out.append(v)
        flags.append(bool(len(v) and ok))
    return out, np.array(flags, dtype=bool)
