"""The surface gate of paint tracing restated in plain Python floats (include/pointnet_refine_hip.h,
"Paint tracing - the rule: surface gate"): which rows the gate leaves out, and nothing else - the rows
it keeps go to tests/_trace_oracle.py as they are, with their offsets recomputed.  The ground table is
an input, as in tests/_floor_oracle.py.  The reference of test_trace_surface_cpu.py / _gpu.py."""
import math

import _trace_oracle as O
from _floor_oracle import grid_shape

GATE = dict(band=0.15, ground_cell=1.0, g_half_length=None, g_half_width=None)    # None: the trace window's


def off_surface(row, ground_s, p, g):
    """True for a point that passes the tracing rule's own tests and is off the surface; p: the tracing
    parameters, g: band, ground_cell and the ground window half_length, half_width."""
    x, y, z, intensity = (float(v) for v in row)
    nx, ny = O.grid_shape(p)
    if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)) or abs(z) > 512.0:
        return False
    if not (0 <= math.floor((x + float(p["half_length"])) / float(p["col"])) < nx
            and 0 <= math.floor((y + float(p["half_width"])) / float(p["cell"])) < ny):
        return False
    if O.point_weight(intensity, float(p["intensity_floor"])) == 0:
        return False
    gx, gy = grid_shape(g)
    gix, giy = math.floor((x + g["half_length"]) / g["ground_cell"]), math.floor((y + g["half_width"]) / g["ground_cell"])
    if not (0 <= gix < gx and 0 <= giy < gy):
        return True
    h = float(ground_s[gix][giy])
    return h != h or not abs(z - h) <= g["band"]


def paint_peaks(points, slice_offsets, ground, **kw):
    """_trace_oracle.paint_peaks over the rows the gate keeps, with 'off_surface' (per slice) and 'keep'
    (per row: False where the gate left the row out) added.  kw: the tracing parameters and GATE's."""
    gate = {k: kw.pop(k, v) for k, v in GATE.items()}
    p = O.params(kw)
    g = {"band": float(gate["band"]), "ground_cell": float(gate["ground_cell"]),
         "half_length": float(p["half_length"] if gate["g_half_length"] is None else gate["g_half_length"]),
         "half_width": float(p["half_width"] if gate["g_half_width"] is None else gate["g_half_width"])}
    keep, off, new_offsets = [], [], [0]
    for s in range(len(slice_offsets) - 1):
        rows = range(int(slice_offsets[s]), int(slice_offsets[s + 1]))
        out = [off_surface(points[i], ground[s], p, g) for i in rows]
        keep += [not o for o in out]
        off.append(sum(out))
        new_offsets.append(new_offsets[-1] + len(out) - off[-1])
    peaks = O.paint_peaks([points[i] for i in range(len(keep)) if keep[i]], new_offsets, **kw)
    peaks["off_surface"], peaks["keep"] = off, keep
    return peaks
