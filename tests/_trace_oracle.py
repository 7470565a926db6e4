"""Paint tracing restated in plain Python: ints and floats, plain loops, one rounding per operation
(Python's float arithmetic is IEEE fp64, round() on a float is half-to-even, int -> float rounds to
nearest even as a C cast does).  The rule is in include/pointnet_refine_hip.h, "Paint tracing - the
rule"; this file is its second statement and the reference of test_trace_cpu.py / test_trace_gpu.py.
No numpy in the arithmetic: arrays are only read row by row."""
import math

DEFAULTS = dict(half_length=25.0, col=0.5, half_width=12.8, cell=0.05, intensity_floor=0.0, nms=4, min_points=3,
                min_weight=1, link_cells=3, gap_slope=1, max_gap_cols=24, min_peaks=3, min_length=5.0)
PEAK_KEYS = ("peak_offsets", "iy", "weight", "count", "xyz", "col", "succ", "pred")


def params(kw):
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise TypeError(f"unknown parameter {k}")
        p[k] = v
    return p


def grid_shape(p):
    return (int(round(2.0 * float(p["half_length"]) / float(p["col"]))),
            int(round(2.0 * float(p["half_width"]) / float(p["cell"]))))


def point_weight(intensity, intensity_floor):
    if not math.isfinite(intensity):
        return 0
    return int(round(min(max(intensity - intensity_floor, 0.0), 4096.0) * 256.0))


def slice_tables(rows, p, nx, ny):
    """{(ix, iy): [n, w, wx, wy, wz]} of one slice's rows, and the number of points kept."""
    hl, col, hw, cell, floor = (float(p[k]) for k in ("half_length", "col", "half_width", "cell", "intensity_floor"))
    tab, kept = {}, 0
    for row in rows:
        x, y, z, intensity = float(row[0]), float(row[1]), float(row[2]), float(row[3])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        fx, fy = math.floor((x + hl) / col), math.floor((y + hw) / cell)
        if not (0 <= fx < nx and 0 <= fy < ny):
            continue
        if abs(z) > 512.0:
            continue
        qi = point_weight(intensity, floor)
        if qi == 0:
            continue
        qx, qy, qz = int(round(x * 1024.0)), int(round(y * 1024.0)), int(round(z * 1024.0))
        t = tab.setdefault((fx, fy), [0, 0, 0, 0, 0])
        t[0] += 1
        t[1] += qi
        t[2] += qi * qx
        t[3] += qi * qy
        t[4] += qi * qz
        kept += 1
    return tab, kept


def column_peaks(tab, ix, ny, p):
    """The peaks of one column in ascending iy: (iy, b, n3, (x, y, z))."""
    nms, min_points, min_weight = int(p["nms"]), int(p["min_points"]), int(p["min_weight"])
    zero = [0, 0, 0, 0, 0]

    def box(iy, k):
        if not 0 <= iy < ny:
            return 0
        total = 0
        for j in (iy - 1, iy, iy + 1):
            if 0 <= j < ny:
                total += tab.get((ix, j), zero)[k]
        return total

    b = [box(iy, 1) for iy in range(ny)]

    def b_at(iy):
        return b[iy] if 0 <= iy < ny else 0

    out = []
    for iy in range(ny):
        if b[iy] < min_weight or box(iy, 0) < min_points:
            continue
        ok = True
        for k in range(1, nms + 1):
            if not (b[iy] > b_at(iy - k) and b[iy] >= b_at(iy + k)):
                ok = False
                break
        if ok:
            fb = float(b[iy])
            out.append((iy, b[iy], box(iy, 0), tuple((float(box(iy, k)) / fb) / 1024.0 for k in (2, 3, 4))))
    return out


def neighbour(columns, ix, iy, direction, nx, p):
    """succ (direction +1) or pred (-1) before the mutual test: (column, row in that column) or None."""
    for dc in range(1, int(p["max_gap_cols"]) + 2):
        c = ix + direction * dc
        if not 0 <= c < nx:
            break
        tol = int(p["link_cells"]) + int(p["gap_slope"]) * (dc - 1)
        best = None
        for r, pk in enumerate(columns[c]):
            d = abs(pk[0] - iy)
            if d <= tol and (best is None or d < best[0]):       # ascending iy: a tie keeps the smaller iy
                best = (d, r)
        if best is not None:
            return c, best[1]
    return None


def paint_peaks(points, slice_offsets, **kw):
    """{'peak_offsets' [S*nx+1], 'iy', 'weight', 'count', 'xyz' [(x, y, z)], 'col', 'succ', 'pred' (lists over
    the peaks in (slice, ix, iy) order), 'bright_points'}."""
    p = params(kw)
    nx, ny = grid_shape(p)
    out = {k: [] for k in PEAK_KEYS}
    out["peak_offsets"] = [0]
    out["bright_points"] = 0
    for s in range(len(slice_offsets) - 1):
        tab, kept = slice_tables(points[int(slice_offsets[s]):int(slice_offsets[s + 1])], p, nx, ny)
        out["bright_points"] += kept
        columns = [column_peaks(tab, ix, ny, p) for ix in range(nx)]
        first = []                                               # the global row of every column's first peak
        for ix in range(nx):
            first.append(out["peak_offsets"][-1])
            for iy, b, n3, xyz in columns[ix]:
                out["iy"].append(iy)
                out["weight"].append(b)
                out["count"].append(n3)
                out["xyz"].append(xyz)
                out["col"].append(s * nx + ix)
            out["peak_offsets"].append(first[-1] + len(columns[ix]))
        for ix in range(nx):
            for r, pk in enumerate(columns[ix]):
                for key, direction in (("succ", 1), ("pred", -1)):
                    q = neighbour(columns, ix, pk[0], direction, nx, p)
                    mutual = q is not None and neighbour(columns, q[0], columns[q[0]][q[1]][0], -direction, nx, p) == (ix, r)
                    out[key].append(first[q[0]] + q[1] if mutual else -1)
    return out


def chain_lines(peaks, n_slices, nx, min_peaks=3, min_length=5.0):
    """(lines_per_slice: lists of [(x, y, z)], dropped): the maximal chains of links in the order of
    their heads, those with fewer than min_peaks peaks or x_last - x_first < min_length left out."""
    lines = [[] for _ in range(n_slices)]
    dropped = 0
    for head in range(len(peaks["iy"])):
        if peaks["pred"][head] >= 0:
            continue
        chain, q = [], head
        while q >= 0:
            chain.append(peaks["xyz"][q])
            q = peaks["succ"][q]
        if len(chain) >= int(min_peaks) and chain[-1][0] - chain[0][0] >= float(min_length):
            lines[peaks["col"][head] // nx].append(chain)
        else:
            dropped += 1
    return lines, dropped


def trace_lines(points, slice_offsets, **kw):
    p = params(kw)
    nx, _ = grid_shape(p)
    peaks = paint_peaks(points, slice_offsets, **kw)
    n_s = len(slice_offsets) - 1
    lines, dropped = chain_lines(peaks, n_s, nx, p["min_peaks"], p["min_length"])
    report = {"slices": n_s, "bright_points": peaks["bright_points"], "peaks": len(peaks["iy"]),
              "links": sum(1 for q in peaks["succ"] if q >= 0), "lines": sum(len(ls) for ls in lines),
              "lines_dropped_short": dropped}
    return lines, report
