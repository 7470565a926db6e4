"""Paint floor restated in plain Python: ints and floats, plain loops, one rounding per operation
(Python's float arithmetic is IEEE fp64, int -> float rounds to nearest even as a C cast does,
math.isqrt is the exact integer floor square root).  The rule is in include/pointnet_refine_hip.h,
"Paint floor - the rule"; this file is its second statement and the reference of test_floor_cpu.py /
test_floor_gpu.py.  No numpy in the arithmetic: arrays are only read row by row.  The ground table is
an input: the ground stage has its own rule and its own oracle."""
import math

DEFAULTS = dict(half_length=25.0, half_width=12.8, ground_cell=1.0, band=0.15, bin_width=1.0, n_bins=256, min_points=16)
OTSU_KEYS = ("t_lo", "t_hi", "t", "total", "above", "w0", "m0", "wr", "mr", "score")


def params(kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError(f"unknown parameter {k}")
        p[k] = v
    return p


def grid_shape(p):
    return (int(math.ceil(2.0 * float(p["half_length"]) / float(p["ground_cell"]))),
            int(math.ceil(2.0 * float(p["half_width"]) / float(p["ground_cell"]))))


def cell_centres(p):
    """The (gx * gy) query points of one slice's ground table, ix-major."""
    gx, gy = grid_shape(p)
    hl, hw, cell = float(p["half_length"]), float(p["half_width"]), float(p["ground_cell"])
    return [(-hl + (ix + 0.5) * cell, -hw + (iy + 0.5) * cell) for ix in range(gx) for iy in range(gy)]


def surface_bin(row, ground_s, p, gx, gy):
    """The bin of one point, None where it is no surface point.  ground_s[ix][iy]: the slice's table."""
    hl, hw, cell, band, width = (float(p[k]) for k in ("half_length", "half_width", "ground_cell", "band", "bin_width"))
    n_bins = int(p["n_bins"])
    x, y, z, intensity = float(row[0]), float(row[1]), float(row[2]), float(row[3])
    if not (math.isfinite(x) and math.isfinite(y)):
        return None
    fx, fy = math.floor((x + hl) / cell), math.floor((y + hw) / cell)
    if not (0 <= fx < gx and 0 <= fy < gy):
        return None
    g = float(ground_s[fx][fy])
    if g != g or not math.isfinite(z) or not abs(z - g) <= band:
        return None
    if not math.isfinite(intensity) or not intensity >= 0.0:
        return None
    q = intensity / width
    if q == math.inf:                                            # a bin_width far below 1 can overflow the quotient
        return n_bins - 1
    fb = math.floor(q)
    return n_bins - 1 if fb >= n_bins else int(fb)


def surface_histograms(points, slice_offsets, ground, **kw):
    """hist[s][b]: lists of ints.  ground[s][ix][iy] floats, NaN: none."""
    p = params(kw)
    gx, gy = grid_shape(p)
    hist = []
    for s in range(len(slice_offsets) - 1):
        h = [0] * int(p["n_bins"])
        for i in range(int(slice_offsets[s]), int(slice_offsets[s + 1])):
            b = surface_bin(points[i], ground[s], p, gx, gy)
            if b is not None:
                h[b] += 1
        hist.append(h)
    return hist


def score(w0, m0, wr, mr):
    w1, m1 = wr - w0, mr - m0
    d = float(m1) / float(w1) - float(m0) / float(w0)
    p = float(w0) * float(w1)
    return p * (d * d)


def otsu(h, min_points=16):
    """One row: the dict of OTSU_KEYS."""
    h = [max(int(c), 0) for c in h]
    n = len(h)
    r = [math.isqrt(c) for c in h]
    wr, mr, total = sum(r), sum(b * r[b] for b in range(n)), sum(h)
    pw, pm, pc = [0], [0], [0]                                   # sums over b < t
    for b in range(n):
        pw.append(pw[-1] + r[b])
        pm.append(pm[-1] + b * r[b])
        pc.append(pc[-1] + h[b])
    sc = [None] * n                                              # None: no candidate
    for t in range(1, n):
        if pc[t] >= min_points and total - pc[t] >= min_points and pw[t] > 0 and wr - pw[t] > 0:
            sc[t] = score(pw[t], pm[t], wr, mr)
    out = {"t_lo": -1, "t_hi": -1, "t": -1, "total": total, "above": 0, "w0": 0, "m0": 0, "wr": wr, "mr": mr, "score": 0.0}
    best, t_lo = 0.0, -1
    for t in range(1, n):
        if sc[t] is not None and sc[t] > best:
            best, t_lo = sc[t], t
    if t_lo < 0:
        return out
    t_hi = t_lo
    while t_hi + 1 < n and sc[t_hi + 1] is not None and sc[t_hi + 1] == best:
        t_hi += 1
    ts = (t_lo + t_hi) >> 1
    out.update({"t_lo": t_lo, "t_hi": t_hi, "t": ts, "above": total - pc[ts], "w0": pw[t_lo], "m0": pm[t_lo], "score": best})
    return out


def otsu_brute(h, min_points=16):
    """(t_lo, t_hi, t*) with every sum taken afresh for every t: no prefix, no shared state."""
    h = [max(int(c), 0) for c in h]
    n = len(h)

    def at(t):
        lo, hi = range(0, t), range(t, n)
        if sum(h[b] for b in lo) < min_points or sum(h[b] for b in hi) < min_points:
            return None
        w0, w1 = sum(math.isqrt(h[b]) for b in lo), sum(math.isqrt(h[b]) for b in hi)
        if w0 <= 0 or w1 <= 0:
            return None
        m0, m1 = sum(b * math.isqrt(h[b]) for b in lo), sum(b * math.isqrt(h[b]) for b in hi)
        d = float(m1) / float(w1) - float(m0) / float(w0)
        return (float(w0) * float(w1)) * (d * d)

    scores = {t: at(t) for t in range(1, n)}
    cands = [t for t in scores if scores[t] is not None]
    top = max((scores[t] for t in cands), default=0.0)
    if not top > 0.0:
        return -1, -1, -1
    t_lo = min(t for t in cands if scores[t] == top)
    t_hi = t_lo
    while scores.get(t_hi + 1) is not None and scores[t_hi + 1] == top:
        t_hi += 1
    return t_lo, t_hi, (t_lo + t_hi) >> 1


def drive_row(hist):
    n = len(hist[0]) if hist else 0
    return [sum(h[b] for h in hist) for b in range(n)]


def share_and_contrast(h, t, bin_width=1.0):
    """(paint_share, contrast) of a row with threshold bin t >= 1: c1 / W and mu1 - mu0 in intensity
    units, the means of the bin numbers over the raw counts times bin_width."""
    h = [max(int(c), 0) for c in h]
    c0, c1 = sum(h[:t]), sum(h[t:])
    s0, s1 = sum(b * h[b] for b in range(t)), sum(b * h[b] for b in range(t, len(h)))
    return float(c1) / float(c0 + c1), (float(s1) / float(c1) - float(s0) / float(c0)) * float(bin_width)
