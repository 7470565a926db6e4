"""Paint floor: the intensity threshold between asphalt and paint, read from the road itself.

``trace.paint_peaks``, ``align.paint_scores`` and ``support.node_support`` take an ``intensity_floor``
that depends on the lidar, on its calibration and on the road.  The number is in the cloud: asphalt and
paint are two populations of the intensity of the points on the road surface.  Per slice
``drive.slice_cloud`` returns, the points within ``band`` of the road height of their 1 m cell are
counted into an intensity histogram, and the threshold is Otsu's over the integer square roots of the
counts - which stays between the populations from a fraction of a percent of paint to a painted
majority, where the raw counts do not - with the middle of the plateau between separated populations
taken (``csrc/prh_floor.hpp``; the rule is in ``include/pointnet_refine_hip.h``, "Paint floor - the
rule", and restated in ``tests/_floor_oracle.py``).

  surface_ground      the road height of every cell of every slice: one ground.ground_heights call
  surface_histograms  HIP: the intensity histogram of every slice's surface points, one read of the cloud
  otsu_floors         HIP: the threshold of every histogram row, one wave per row
  paint_floor         the three above; the drive's floor is that of the integer sum of all rows
  resolve             what a caller's intensity_floor argument means: a number, or "auto"

    floor, report = paint_floor(points, offsets)

Scope: the rule always splits - a road with no paint still gets a floor; 'paint_share' and 'contrast'
are reported so the caller can judge, nothing is gated on them.  Intensity is taken as it is, with no
range or incidence correction.  There is no CPU fallback: without a GPU these raise RuntimeError.
"""
import numpy as np
import torch

from . import _gpu as G
from . import _lib as L
from . import ground as GR

HALF_LENGTH, HALF_WIDTH = 25.0, 12.8
GROUND_CELL, GROUND_RADIUS = 1.0, 0.75
MAX_CELLS = 1024             # gx and gy
BAND = 0.15
BIN_WIDTH, N_BINS = 1.0, 256
MAX_BINS = 1024              # prh_floor_max_bins()
MIN_POINTS = 16
OTSU_KEYS = ("t_lo", "t_hi", "t", "total", "above", "w0", "m0", "wr", "mr", "score")
_OTSU_DTYPES = (torch.int32,) * 3 + (torch.int64,) * 6 + (torch.float64,)


def _params(what, half_length=HALF_LENGTH, half_width=HALF_WIDTH, ground_cell=GROUND_CELL, ground_radius=GROUND_RADIUS,
            band=BAND, bin_width=BIN_WIDTH, n_bins=N_BINS, min_points=MIN_POINTS):
    """The checked parameters, with gx and gy ("Paint floor - the rule": Surface grid)."""
    half_length, half_width, ground_cell, ground_radius, band, bin_width = (
        float(v) for v in (half_length, half_width, ground_cell, ground_radius, band, bin_width))
    for name, v in (("half_length", half_length), ("half_width", half_width), ("ground_cell", ground_cell),
                    ("bin_width", bin_width)):
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError(f"{what}: {name} must be positive and finite")
    if not (np.isfinite(band) and band >= 0.0):
        raise ValueError(f"{what}: band must be finite and >= 0")
    if not 0.0 < ground_radius <= GR.MAX_RADIUS:
        raise ValueError(f"{what}: 0 < ground_radius <= {GR.MAX_RADIUS}")
    fx, fy = np.ceil(2.0 * half_length / ground_cell), np.ceil(2.0 * half_width / ground_cell)
    if not (1 <= fx <= MAX_CELLS and 1 <= fy <= MAX_CELLS):
        raise ValueError(f"{what}: 1 <= gx, gy <= {MAX_CELLS}, got {fx:g} x {fy:g}")
    return {"half_length": half_length, "half_width": half_width, "ground_cell": ground_cell, "ground_radius": ground_radius,
            "band": band, "bin_width": bin_width, "gx": int(fx), "gy": int(fy), "n_bins": _int(n_bins, 2, MAX_BINS, "n_bins", what),
            "min_points": _int(min_points, 1, 2 ** 62, "min_points", what)}


def _int(v, lo, hi, name, what):
    if isinstance(v, (bool, np.bool_)) or int(v) != v or not lo <= int(v) <= hi:
        raise ValueError(f"{what}: {name} must be an integer in {lo} .. {hi}")
    return int(v)


def _sliced(points, slice_offsets, what):
    dev = G.device("paintfloor", points.device if torch.is_tensor(points) and points.is_cuda else None)
    pts = G.points4(points, dev, what)
    off = G.offsets(slice_offsets, pts.shape[0], what, "slice_offsets")
    if len(off) > 1 and int(np.diff(off).max()) >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 points per slice")
    return dev, pts, off


def _surface_ground(pts, off, p):
    n_s, gx, gy = len(off) - 1, p["gx"], p["gy"]
    if n_s == 0:
        return torch.empty((0, gx, gy), dtype=torch.float64, device=pts.device)
    cx = -p["half_length"] + (np.arange(gx, dtype=np.float64) + 0.5) * p["ground_cell"]
    cy = -p["half_width"] + (np.arange(gy, dtype=np.float64) + 0.5) * p["ground_cell"]
    q = np.stack([np.repeat(cx, gy), np.tile(cy, gx)], 1)
    res = GR.ground_heights(pts, off, np.tile(q, (n_s, 1)), np.arange(n_s + 1, dtype=np.int64) * (gx * gy),
                            radius=p["ground_radius"])
    return res["height"].reshape(n_s, gx, gy)


def surface_ground(points, slice_offsets, half_length=HALF_LENGTH, half_width=HALF_WIDTH, ground_cell=GROUND_CELL,
                   ground_radius=GROUND_RADIUS):
    """The road height of every cell of the surface grid of every slice ("Paint floor - the rule":
    Surface grid): (S,gx,gy) float64 CUDA, NaN where there is none.  One ground.ground_heights call
    whose queries are the cell centres, with radius = ground_radius and ground's defaults otherwise."""
    what = "surface_ground"
    p = _params(what, half_length, half_width, ground_cell, ground_radius)
    _, pts, off = _sliced(points, slice_offsets, what)
    return _surface_ground(pts, off, p)


def ground_shape(ground, n_slices, p, what):
    """ValueError unless a caller's prebuilt ground table is (n_slices, gx, gy) of p = _params(...)."""
    shape = tuple(ground.shape) if torch.is_tensor(ground) else np.shape(ground)
    if shape != (n_slices, p["gx"], p["gy"]):
        raise ValueError(f"{what}: ground must be {(n_slices, p['gx'], p['gy'])}, got {shape}")


def _ground_table(ground, pts, off, p, dev, what):
    """The (S,gx,gy) float64 CUDA table: surface_ground's (None), or the caller's own, checked."""
    if ground is None:
        return _surface_ground(pts, off, p)
    ground = G.as_cuda(ground, dev, what, torch.float64)
    ground_shape(ground, len(off) - 1, p, what)
    return ground


def _histograms(pts, off, ground, p, dev, copies=None):
    n_s, n_bins = len(off) - 1, p["n_bins"]
    hist = torch.empty((n_s, n_bins), dtype=torch.int64, device=dev)
    off_t = torch.from_numpy(off).to(dev)
    lib = L.lib()
    args = (G.ptr(pts), 1 if pts.dtype == torch.float64 else 0, G.ptr(off_t), n_s, pts.shape[0], p["half_length"],
            p["half_width"], p["ground_cell"], p["gx"], p["gy"], G.ptr(ground), p["band"], p["bin_width"], n_bins, G.ptr(hist),
            dev.index, G.stream(dev))
    if copies is None:
        L.check(lib.prh_floor_hist(*args), "prh_floor_hist")
    else:
        L.check(lib.prh_test_floor_hist(int(copies), *args), "prh_test_floor_hist")
    return hist


def surface_histograms(points, slice_offsets, ground=None, copies=None, **params):
    """The intensity histogram of the surface points of every slice ("Paint floor - the rule").

    points (T,4) float64 or float32 x y z intensity, every slice in its own frame, with slice_offsets
    (S+1,) - what drive.slice_cloud returns (CUDA tensors are used where they are, numpy is
    uploaded).  ground: the (S,gx,gy) float64 table of road heights, NaN where there is none (None:
    surface_ground builds it).  params: half_length, half_width, ground_cell, ground_radius, band,
    bin_width, n_bins (the rule's).  copies: None, or the number of LDS copies of a block's histogram
    (1, 2, 4 or 8: the same bits, for measurement).  Returns (S,n_bins) int64 CUDA.  Bitwise
    reproducible, whatever the order of the points or their dtype."""
    what = "surface_histograms"
    p = _params(what, **params)
    dev, pts, off = _sliced(points, slice_offsets, what)
    if copies is not None and copies not in (1, 2, 4, 8):
        raise ValueError(f"{what}: copies must be 1, 2, 4 or 8")
    return _histograms(pts, off, _ground_table(ground, pts, off, p, dev, what), p, dev, copies)


def otsu_floors(hist, min_points=MIN_POINTS, bin_width=BIN_WIDTH):
    """The threshold of every histogram row ("Paint floor - the rule": Threshold of one row).

    hist (R,n_bins) int64, a CUDA tensor or numpy (uploaded).  Returns a dict of CUDA tensors, each
    (R,): 't_lo', 't_hi', 't' int32 (-1: no floor), 'total' (W), 'above' (c1 at t), 'w0', 'm0' (at
    t_lo), 'wr', 'mr' int64, 'score' float64, and 'floor' float64 = t * bin_width (NaN: none)."""
    what = "otsu_floors"
    shape = tuple(hist.shape) if torch.is_tensor(hist) else np.shape(hist)
    if len(shape) != 2:
        raise ValueError(f"{what}: hist must be (R,n_bins), got {shape}")
    n_bins = _int(shape[1], 2, MAX_BINS, "n_bins", what)
    min_points = _int(min_points, 1, 2 ** 62, "min_points", what)
    bin_width = float(bin_width)
    if not (np.isfinite(bin_width) and bin_width > 0.0):
        raise ValueError(f"{what}: bin_width must be positive and finite")
    if shape[0] >= 2 ** 31:
        raise ValueError(f"{what}: fewer than 2^31 rows")
    dev = G.device("paintfloor", hist.device if torch.is_tensor(hist) and hist.is_cuda else None)
    if not torch.is_tensor(hist):
        hist = np.asarray(hist, dtype=np.int64)
    h = G.as_cuda(hist, dev, what).to(torch.int64).contiguous()
    out = {k: torch.empty((shape[0],), dtype=d, device=dev) for k, d in zip(OTSU_KEYS, _OTSU_DTYPES)}
    L.check(L.lib().prh_floor_otsu(G.ptr(h), shape[0], n_bins, min_points, *(G.ptr(out[k]) for k in OTSU_KEYS), dev.index,
                                   G.stream(dev)), "prh_floor_otsu")
    out["floor"] = torch.where(out["t"] >= 0, out["t"].to(torch.float64) * bin_width,
                               torch.full_like(out["score"], float("nan")))
    return out


def paint_floor(points, slice_offsets, ground=None, **params):
    """The drive's intensity floor, read from its own road ("Paint floor - the rule").

    points, slice_offsets, ground: as surface_histograms takes them (ground: a table surface_ground
    has already built for these slices and parameters, which is then not built again); params: its
    parameters and min_points.  One surface_ground call, one pass over the points, then one otsu_floors call over the slices'
    rows and their integer sum, the drive's row.  Returns (floor: float, report {'floor', 'bin' (t*),
    'plateau' (t_lo, t_hi), 'surface_points', 'paint_share' (c1 / W), 'contrast' (mu1 - mu0 of the raw
    counts, in intensity units), 'floor_per_slice' (S,) float64 (NaN: none), 'slices_without_floor'});
    ValueError where the drive's row has no floor."""
    what = "paint_floor"
    p = _params(what, **params)
    dev, pts, off = _sliced(points, slice_offsets, what)
    hist = _histograms(pts, off, _ground_table(ground, pts, off, p, dev, what), p, dev)
    rows = torch.cat([hist, hist.sum(0, keepdim=True)])
    res = {k: v.cpu().numpy() for k, v in otsu_floors(rows, p["min_points"], p["bin_width"]).items()}
    t = int(res["t"][-1])
    if t < 0:
        raise ValueError(f"{what}: the {int(res['total'][-1])} surface points of the drive do not split into two "
                         f"populations of at least {p['min_points']} points")
    h = rows[-1].cpu().numpy()
    b = np.arange(len(h), dtype=np.int64)
    c0, c1 = int(h[:t].sum()), int(h[t:].sum())
    contrast = (float(int((b[t:] * h[t:]).sum())) / float(c1) - float(int((b[:t] * h[:t]).sum())) / float(c0)) * p["bin_width"]
    per_slice = res["floor"][:-1]
    report = {"floor": float(res["floor"][-1]), "bin": t, "plateau": (int(res["t_lo"][-1]), int(res["t_hi"][-1])),
              "surface_points": int(res["total"][-1]), "paint_share": float(int(res["above"][-1])) / float(int(res["total"][-1])),
              "contrast": contrast, "floor_per_slice": per_slice.copy(),
              "slices_without_floor": int(np.isnan(per_slice).sum())}
    return report["floor"], report


def resolve(intensity_floor, points, slice_offsets, what, ground=None, **params):
    """What a caller's intensity_floor means: a number passes through unchanged, with the report
    None; the string "auto" gives paint_floor(points, slice_offsets, ground, **params); anything else
    raises ValueError."""
    if isinstance(intensity_floor, str):
        if intensity_floor != "auto":
            raise ValueError(f"{what}: intensity_floor must be a number or 'auto', got {intensity_floor!r}")
        if points is None:
            raise ValueError(f"{what}: intensity_floor='auto' needs a sliced cloud, and there is no slice")
        return paint_floor(points, slice_offsets, ground, **params)
    try:
        ok = not isinstance(intensity_floor, (bool, np.bool_)) and float(intensity_floor) is not None
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: intensity_floor must be a number or 'auto', got {intensity_floor!r}")
    return intensity_floor, None


def floor_argument(text):
    """An --intensity-floor command-line value: a number, or the word auto."""
    return "auto" if text == "auto" else float(text)


def floor_line(report):
    """The PAINT FLOOR line of the examples, from a caller's report that holds report_keys' entries."""
    return (f"PAINT FLOOR  {report['floor']:g} read from {report['floor_surface_points']} surface points   "
            f"{100.0 * report['floor_paint_share']:.1f} % of them above it   contrast {report['floor_contrast']:.1f}")


def report_keys(report):
    """The entries a caller's report gains with intensity_floor='auto'."""
    return {"floor": report["floor"], "floor_surface_points": report["surface_points"],
            "floor_paint_share": report["paint_share"], "floor_contrast": report["contrast"]}
