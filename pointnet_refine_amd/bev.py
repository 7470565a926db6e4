"""BEV rendering: the reference's result viewer (tools/vis_inference_bev.py) and its training
picture (train_dist.py:18-56) without matplotlib - the intensity image, the percentile tone map,
the colour table, zoomed views per item and line overlays on the GPU (``csrc/prh_bev.hpp``), PNG
files from the standard library.  The reference argsorts the whole cloud per scene and opens one
matplotlib figure per item; here the slice points and the refined lines are on the device already
and never leave it before the finished views do.

  bev_map / bev_maps     HIP: generate_bev_map (:74-104), pixel for pixel: the maximum intensity per
                         pixel, in the dtype of the points; every slice of a CSR-packed cloud at once
  tone_map / colorize    HIP: percentile (exact radix select) + clip + power (:143-148); 'jet' / 'gray'
  crop_views             HIP: the zoomed views (:224-228) as pixel-aligned copies of the scene image
  draw_lines             HIP: polylines over a batch of views, by the rule written down in
                         include/pointnet_refine_hip.h ("Overlays - the rule")
  chamfer_xy             calc_metric (:154-176) on predictions.line_costs
  item_windows           host: the zoom rule (:178-214)
  jet_table / write_png  host: matplotlib's 'jet' from its piecewise-linear definition; 8-bit RGBA PNG
  render_scene           main()'s body for one scene (:132-271)
  render_sample          the training picture of sample 0 of a batch

Line widths of the reference are points at 100 dpi: 1 pt = 100 / 72 px (PX_PER_PT).  The GPU
functions have no CPU fallback: without a GPU they raise RuntimeError.
"""
import json
import os
import struct
import zlib

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L

RESOLUTION = 0.05            # vis_inference_bev.py:24
PADDING = 5.0                # :74
WINDOW_PAD = 10.0            # :207
PX_PER_PT = 100.0 / 72.0     # matplotlib line widths are points; the reference's figures are 100 dpi
# (:232,253,255); matplotlib's '--' is 3.7 on, 1.6 off in units of the line width
STYLE_GT = {"color": (0, 255, 0), "width": 2.0 * PX_PER_PT, "alpha": 0.8, "dash": None}
STYLE_NOISY = {"color": (255, 0, 0), "width": 1.5 * PX_PER_PT, "alpha": 1.0,
               "dash": (3.7 * 1.5 * PX_PER_PT, 1.6 * 1.5 * PX_PER_PT)}
STYLE_REFINED = {"color": (0, 255, 255), "width": 2.0 * PX_PER_PT, "alpha": 0.9, "dash": None}
# train_dist.py:45-47: no transparency there
STYLE_SAMPLE_GT = dict(STYLE_GT, alpha=1.0)
STYLE_SAMPLE_PRED = dict(STYLE_REFINED, alpha=1.0)


# ------------------------------------------------------------------ host side
_JET = {   # matplotlib's 'jet': (x, y) breakpoints per channel, linear in between
    "red": ((0.0, 0.0), (0.35, 0.0), (0.66, 1.0), (0.89, 1.0), (1.0, 0.5)),
    "green": ((0.0, 0.0), (0.125, 0.0), (0.375, 1.0), (0.64, 1.0), (0.91, 0.0), (1.0, 0.0)),
    "blue": ((0.0, 0.5), (0.11, 1.0), (0.34, 1.0), (0.65, 0.0), (1.0, 0.0)),
}


def jet_table():
    """(256,4) uint8: matplotlib's 'jet' as bytes.  Entry k samples the piecewise-linear channels at
    k / 255, in the breakpoints' own scale (x * 255) as matplotlib's table builder does, and a byte
    is int(value * 255)."""
    n = 256
    xind = (n - 1) * np.linspace(0.0, 1.0, n)
    out = np.full((n, 4), 255, dtype=np.uint8)
    for c, name in enumerate(("red", "green", "blue")):
        bp = np.array(_JET[name], dtype=np.float64)
        x, y = bp[:, 0] * (n - 1), bp[:, 1]
        ind = np.searchsorted(x, xind)[1:-1]
        dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut = np.concatenate(([y[0]], dist * (y[ind] - y[ind - 1]) + y[ind - 1], [y[-1]]))
        out[:, c] = (np.clip(lut, 0.0, 1.0) * 255).astype(np.uint8)
    return out


def gray_table():
    """(256,4) uint8: entry k is (k, k, k, 255)."""
    k = np.arange(256, dtype=np.uint8)
    return np.stack([k, k, k, np.full(256, 255, dtype=np.uint8)], 1)


def write_png(path, rgba):
    """8-bit RGBA PNG of an (H, W, 4) uint8 array (numpy or tensor): one IDAT, filter 0 rows."""
    if torch.is_tensor(rgba):
        rgba = rgba.detach().cpu().numpy()
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    if a.ndim != 3 or a.shape[2] != 4 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: expected (H, W, 4) uint8 with H, W >= 1, got {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 4 * w), dtype=np.uint8)
    rows[:, 1:] = a.reshape(h, 4 * w)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def _line(l):
    """A polyline as an (n, >=2) float64 array: an array, or the scene JSON's list of {'x','y','z'}."""
    if l is None:
        return np.zeros((0, 3))
    if isinstance(l, (list, tuple)) and len(l) and isinstance(l[0], dict):
        return np.array([[p["x"], p["y"], p.get("z", 0.0)] for p in l], dtype=np.float64)
    a = np.asarray(l, dtype=np.float64)
    return a.reshape(-1, a.shape[-1] if a.ndim == 2 else 3)


def item_windows(items, pad=WINDOW_PAD):
    """The reference's zoom rule (:178-214).  items: io.load_scene_items' dicts or the scene JSON's.
    Returns (windows (K,4) float64 rows y_lo, y_hi, x_lo, x_hi, kept: the item index of each): the
    bounds of the GT vertices (a GT of more than one vertex) and of every candidate's vertices,
    +- pad.  Skipped, as there: an item with neither, and an item whose window is empty."""
    wins, kept = [], []
    for idx, item in enumerate(items):
        gt = _line(item.get("position"))
        cands = [_line(c) for c in item.get("noisy_candidates", []) or []]
        xs, ys = [], []
        if len(gt) > 1:
            xs.append(gt[:, 0]); ys.append(gt[:, 1])
        if not cands and not len(gt) > 1:
            continue
        for c in cands:
            xs.append(c[:, 0]); ys.append(c[:, 1])
        xs, ys = (np.concatenate(v) if v else np.zeros(0) for v in (xs, ys))
        if not len(xs):
            continue
        min_x, max_x, min_y, max_y = xs.min() - pad, xs.max() + pad, ys.min() - pad, ys.max() + pad
        if max_y - min_y <= 0 or max_x - min_x <= 0:
            continue
        wins.append([min_y, max_y, min_x, max_x]); kept.append(idx)
    return np.array(wins, dtype=np.float64).reshape(-1, 4), kept


class Views:
    """A batch of RGBA views of different sizes in one buffer: data (P,4) uint8 CUDA, view k =
    data[offsets[k]:offsets[k+1]].reshape(shapes[k] + (4,)) = views[k]; windows (K,4) y_lo, y_hi,
    x_lo, x_hi in metres; resolution in metres per pixel."""

    def __init__(self, data, offsets, shapes, windows, resolution):
        self.data, self.offsets, self.shapes = data, offsets, shapes
        self.windows, self.resolution = windows, resolution

    def __len__(self):
        return len(self.shapes)

    def __getitem__(self, k):
        h, w = self.shapes[k]
        return self.data[self.offsets[k]:self.offsets[k + 1]].view(int(h), int(w), 4)


# ------------------------------------------------------------------ GPU side
def _points_t(points, dev, what):
    if not torch.is_tensor(points):
        points = np.asarray(points)
        if points.dtype not in (np.float32, np.float64):
            raise ValueError(f"{what}: points must be float32 or float64, got {points.dtype}")
        if points.ndim == 2 and points.shape[1] >= 4:
            points = points[:, :4]
    p = G.as_cuda(points, dev, what)
    if p.dtype not in (torch.float32, torch.float64) or p.dim() != 2 or p.shape[1] < 4:
        raise ValueError(f"{what}: points must be (n, >=4) float32 or float64, got {tuple(p.shape)} {p.dtype}")
    return p[:, :4].contiguous()


def _geometry(T, bounds, padding, resolution):
    """Shape and extent as numpy computes them on scalars of dtype T (:80-87): one rounding per operation."""
    res = T(resolution)
    x_min, x_max, y_min, y_max = bounds
    if padding is not None:
        pad = T(padding)
        x_min, x_max, y_min, y_max = T(x_min) - pad, T(x_max) + pad, T(y_min) - pad, T(y_max) + pad
    else:
        x_min, x_max, y_min, y_max = T(x_min), T(x_max), T(y_min), T(y_max)
    w, h = int((y_max - y_min) / res), int((x_max - x_min) / res)
    return max(h, 0), max(w, 0), [y_min, y_max, x_min, x_max]


def _raster(p, offsets, n_slices, h, w, extent, resolution, dev, what):
    image = torch.empty((n_slices, h, w), dtype=torch.float32, device=dev)
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    L.check(L.lib().prh_bev_raster(G.ptr(p), G.ptr(offsets) if offsets is not None else None, n_slices, p.shape[0],
                                   int(p.dtype == torch.float64), float(extent[0]), float(extent[3]),
                                   float((np.float64 if p.dtype == torch.float64 else np.float32)(resolution)),
                                   h, w, G.ptr(image), G.ptr(bad), dev.index, G.stream(dev)), "prh_bev_raster")
    if int(bad.item()):
        raise ValueError(f"{what}: a NaN or infinite x, y or intensity")
    return image


def bev_map(points, resolution=RESOLUTION, padding=PADDING, extent=None):
    """generate_bev_map (:74-104), equal as numbers pixel for pixel.  points (n, >=4) float32 or
    float64, numpy or CUDA tensor; the arithmetic runs in that dtype as numpy's does: bounds =
    min / max of x and y -+ padding, W = int((y_max - y_min) / resolution), H likewise from x,
    u = int32((y - y_min) / resolution), v = int32((x_max - x) / resolution), every operation rounded
    on its own, truncation toward zero, points outside the image dropped.  A pixel holds the maximum
    intensity (as float32) of its points - what the reference's sort-then-overwrite leaves - and 0.0
    when it has none.  extent=(y_min, y_max, x_min, x_max): the bounds are these, no padding.
    Returns (image (H, W) float32 CUDA, [y_min, y_max, x_min, x_max] scalars of the points' dtype).
    Bitwise reproducible.  ValueError for n = 0 and for a NaN or infinite x, y or intensity."""
    dev = G.device("bev")
    p = _points_t(points, dev, "bev_map")
    dev = p.device
    if p.shape[0] == 0:
        raise ValueError("bev_map: zero-size array of points has no minimum")
    T = np.float64 if p.dtype == torch.float64 else np.float32
    if extent is None:
        lib = L.lib()
        nb = lib.prh_bev_bounds_workspace_bytes()
        ws = G.workspace(nb, dev)
        info = torch.empty((5,), dtype=torch.float64, device=dev)
        L.check(lib.prh_bev_bounds(G.ptr(p), p.shape[0], int(T is np.float64), G.ptr(info), G.ptr(ws), nb, dev.index,
                                   G.stream(dev)), "prh_bev_bounds")
        info = info.cpu().numpy()
        if info[4] != 0.0:
            raise ValueError("bev_map: a NaN or infinite x, y or intensity")
        h, w, ext = _geometry(T, info[:4], padding, resolution)
    else:
        h, w, ext = _geometry(T, (extent[2], extent[3], extent[0], extent[1]), None, resolution)
    return _raster(p, None, 1, h, w, ext, resolution, dev, "bev_map")[0], ext


def bev_maps(points, offsets, extent, resolution=RESOLUTION):
    """bev_map(points[offsets[s]:offsets[s+1]], extent=extent) for every slice s of a CSR-packed
    cloud (what drive.slice_cloud returns) in one launch sequence: (S, H, W) float32 CUDA; an empty
    slice is all zero."""
    dev = G.device("bev")
    p = _points_t(points, dev, "bev_maps")
    dev = p.device
    off = (offsets.detach() if torch.is_tensor(offsets) else torch.from_numpy(np.asarray(offsets))).to(dev, torch.int64)
    off = off.reshape(-1).contiguous()
    oh = off.cpu().numpy()
    if len(oh) < 1 or oh[0] != 0 or oh[-1] != p.shape[0] or np.any(np.diff(oh) < 0):
        raise ValueError(f"bev_maps: offsets must rise from 0 to the number of points ({p.shape[0]})")
    T = np.float64 if p.dtype == torch.float64 else np.float32
    h, w, ext = _geometry(T, (extent[2], extent[3], extent[0], extent[1]), None, resolution)
    return _raster(p, off, len(oh) - 1, h, w, ext, resolution, dev, "bev_maps")


def _image_t(image, what):
    if not torch.is_tensor(image) or not image.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what} needs a GPU (there is no CPU fallback)")
        if torch.is_tensor(image):
            raise RuntimeError(f"{what}: tensors must be CUDA tensors (there is no CPU fallback)")
        image = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).to(G.device("bev"))
    if image.dtype != torch.float32 or image.dim() not in (2, 3):
        raise ValueError(f"{what}: image must be (H, W) or (S, H, W) float32, got {tuple(image.shape)} {image.dtype}")
    return image.detach().contiguous()


def _lerp(a, b, gamma):
    """numpy's linear percentile between two neighbours, in float32 as numpy computes it there."""
    a, b, t = np.float32(a), np.float32(b), np.float32(gamma)
    d = b - a
    return b - d * (np.float32(1) - t) if t >= 0.5 else a + d * t


def percentile_positive(image, percentile=90.0):
    """np.percentile(s[s > 0], percentile) for every slice s of image ((H, W) or (S, H, W) float32
    CUDA) without sorting: an exact radix select of the two neighbouring order statistics on the
    device, numpy's 'linear' interpolation between them.  Returns (p list of np.float32 or None
    where a slice has no positive pixel, stats (S,4) float64: count, lower, upper, weight)."""
    img = _image_t(image, "percentile_positive")
    dev = img.device
    s = 1 if img.dim() == 2 else img.shape[0]
    pix = img.numel() // max(s, 1)
    lib = L.lib()
    nb = lib.prh_bev_select_workspace_bytes(s)
    ws = G.workspace(nb, dev)
    out = torch.zeros((s, 4), dtype=torch.float64, device=dev)
    L.check(lib.prh_bev_select(G.ptr(img), s, pix, float(np.float32(percentile) / np.float32(100)), G.ptr(out), G.ptr(ws), nb, dev.index,
                               G.stream(dev)), "prh_bev_select")
    st = out.cpu().numpy()
    return [(_lerp(r[1], r[2], r[3]) if r[0] > 0 else None) for r in st], st


def tone_map(image, percentile=90.0, gamma=0.6):
    """:143-148: p = np.percentile(image[image > 0], percentile), norm = clip(image / p, 0, 1) **
    gamma in float32; with no positive pixel norm = image and p = None.  image (H, W) -> (norm, p);
    (S, H, W) -> (norm, [p per slice]): every slice is tone-mapped on its own."""
    img = _image_t(image, "tone_map")
    dev = img.device
    ps, _ = percentile_positive(img, percentile)
    s = 1 if img.dim() == 2 else img.shape[0]
    pix = img.numel() // max(s, 1)
    pt = torch.tensor([float(p) if p is not None else 0.0 for p in ps], dtype=torch.float32, device=dev)
    norm = torch.empty_like(img)
    L.check(L.lib().prh_bev_tone(G.ptr(img), s, pix, G.ptr(pt), float(gamma), G.ptr(norm), dev.index, G.stream(dev)),
            "prh_bev_tone")
    return (norm, ps[0]) if img.dim() == 2 else (norm, ps)


def colorize(norm, image, cmap="jet"):
    """matplotlib's mapping of norm in [0, 1] to a 256-entry table (index = int(norm * 256), 256 ->
    255), alpha 255; pixels with image == 0 (the reference's mask, :151) are opaque black, the
    reference's axes background.  cmap 'jet' or 'gray'.  Returns norm.shape + (4,) uint8 CUDA."""
    if cmap not in ("jet", "gray"):
        raise ValueError("colorize: cmap must be 'jet' or 'gray'")
    nrm, img = _image_t(norm, "colorize"), _image_t(image, "colorize")
    if nrm.shape != img.shape:
        raise ValueError("colorize: norm and image must have one shape")
    dev = nrm.device
    table = torch.from_numpy((jet_table() if cmap == "jet" else gray_table()).view(np.uint32).reshape(-1).view(np.int32)).to(dev)
    out = torch.empty(tuple(nrm.shape) + (4,), dtype=torch.uint8, device=dev)
    L.check(L.lib().prh_bev_colorize(G.ptr(nrm), G.ptr(img), nrm.numel(), G.ptr(table), G.ptr(out), dev.index,
                                     G.stream(dev)), "prh_bev_colorize")
    return out


def crop_views(rgba, extent, windows, resolution=RESOLUTION):
    """The reference shows the whole image and zooms (interpolation='nearest', :224-228); here every
    window (rows y_lo, y_hi, x_lo, x_hi) gets a copy of the scene image rgba (H, W, 4) uint8 CUDA at
    the image's own resolution, all in one launch, black outside the image.  A view is aligned to
    the image's pixel grid: its first column is image column floor((y_lo - y_min) / resolution), its
    first row image row floor((x_max - x_hi) / resolution), its shape round((y_hi - y_lo) /
    resolution) x round((x_hi - x_lo) / resolution), at least 1 x 1; Views.windows holds the
    windows moved onto that grid (by less than a pixel), the ones to draw lines with."""
    if not torch.is_tensor(rgba) or not rgba.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("crop_views needs a GPU (there is no CPU fallback)")
        raise RuntimeError("crop_views: rgba must be a CUDA tensor (there is no CPU fallback)")
    if rgba.dtype != torch.uint8 or rgba.dim() != 3 or rgba.shape[2] != 4:
        raise ValueError(f"crop_views: rgba must be (H, W, 4) uint8, got {tuple(rgba.shape)} {rgba.dtype}")
    src = rgba.detach().contiguous()
    dev = src.device
    win = np.asarray(windows, dtype=np.float64).reshape(-1, 4)
    y_min, x_max, res = float(extent[0]), float(extent[3]), float(resolution)
    u0 = np.floor((win[:, 0] - y_min) / res).astype(np.int64)
    v0 = np.floor((x_max - win[:, 3]) / res).astype(np.int64)
    w = np.maximum(np.floor((win[:, 1] - win[:, 0]) / res + 0.5), 1).astype(np.int64)
    h = np.maximum(np.floor((win[:, 3] - win[:, 2]) / res + 0.5), 1).astype(np.int64)
    if len(win) and (np.abs(u0).max() >= 2 ** 30 or np.abs(v0).max() >= 2 ** 30 or w.max() >= 2 ** 30 or h.max() >= 2 ** 30):
        raise ValueError("crop_views: a window is too far from the image or too large")
    off = G.csr_offsets(h * w)
    snapped = np.stack([y_min + u0 * res, y_min + (u0 + w) * res, x_max - (v0 + h) * res, x_max - v0 * res], 1)
    data = torch.empty((int(off[-1]), 4), dtype=torch.uint8, device=dev)
    if len(win):
        vt = torch.from_numpy(np.stack([u0, v0, h, w], 1).astype(np.int32)).to(dev)
        ot = torch.from_numpy(off).to(dev)
        L.check(L.lib().prh_bev_crop(G.ptr(src), src.shape[0], src.shape[1], G.ptr(vt), G.ptr(ot), len(win), int(off[-1]),
                                     G.ptr(data), dev.index, G.stream(dev)), "prh_bev_crop")
    return Views(data, off, np.stack([h, w], 1).astype(np.int64).reshape(-1, 2), snapped.reshape(-1, 4), res)


def pack_lines(lines, line_view, styles, windows, resolution):
    """The host half of draw_lines: segments in the pixel units of each line's view, their arc
    lengths and the style rows, as the C entry points take them (fp64).  Returns (segments (n,5),
    segment_line (n,) int32, styles (L,7), line_view (L,) int32)."""
    win = np.asarray(windows, dtype=np.float64).reshape(-1, 4)
    lv = np.asarray(line_view, dtype=np.int64).reshape(-1)
    if len(lv) != len(lines) or len(styles) != len(lines):
        raise ValueError("draw_lines: one view index and one style per line")
    if len(lv) and (lv.min() < 0 or lv.max() >= len(win)):
        raise ValueError("draw_lines: a line names a view that does not exist")
    segs, seg_line = [], []
    st = np.zeros((len(lines), 7), dtype=np.float64)
    for l, line in enumerate(lines):
        s = styles[l]
        dash = s.get("dash") or (0.0, 0.0)
        st[l] = [*s["color"], s.get("alpha", 1.0), s["width"], dash[0], dash[1]]
        a = _line(line)
        if len(a) < 2:
            continue
        y_lo, _, _, x_hi = win[lv[l]]
        px = np.stack([(a[:, 1] - y_lo) / resolution, (x_hi - a[:, 0]) / resolution], 1)
        d = np.diff(px, axis=0)
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        start = np.concatenate(([0.0], np.cumsum(length)[:-1]))
        segs.append(np.column_stack([px[:-1], px[1:], start]))
        seg_line.append(np.full(len(d), l, dtype=np.int32))
    segs = np.concatenate(segs) if segs else np.zeros((0, 5))
    seg_line = np.concatenate(seg_line) if seg_line else np.zeros(0, dtype=np.int32)
    return np.ascontiguousarray(segs), seg_line, st, lv.astype(np.int32)


def draw_lines(canvas, window, lines, line_view, styles, resolution=None):
    """Polylines over a batch of views in one launch sequence, in place; returns canvas.

    canvas: Views (window and resolution default to its own) or an (S, H, W, 4) / (H, W, 4) uint8
    CUDA tensor with window (S,4) / (4,) rows y_lo, y_hi, x_lo, x_hi in metres; column u grows with
    y, row v with decreasing x, pixel centres at half-integers.  lines: (n, >=2) arrays in metres (x,
    y first); line_view[l] the view of line l; styles[l] a dict of 'color' (RGB 0..255), 'width'
    (pixels), 'alpha' and 'dash' ((on, off) pixels along the line from its first vertex, or None) -
    STYLE_GT, STYLE_NOISY, STYLE_REFINED are the reference's (widths there are points at 100 dpi:
    1 pt = 100 / 72 px).  A segment covers a pixel centre at distance d by clamp(width / 2 + 0.5 -
    d, 0, 1), zero where the nearest point is in an 'off' stretch; a line covers it by the maximum
    over its segments; lines are composited in the order given, rgb = rgb * (1 - alpha * c) +
    color * (alpha * c) in fp64, rounded once at the end.  Work scales with the segments' bounding
    boxes (segments are binned to 16 x 16 tiles).  Bitwise reproducible."""
    if isinstance(canvas, Views):
        data, off, shapes = canvas.data, canvas.offsets, canvas.shapes
        window = canvas.windows if window is None else window
        resolution = canvas.resolution if resolution is None else resolution
    else:
        if not torch.is_tensor(canvas) or not canvas.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("draw_lines needs a GPU (there is no CPU fallback)")
            raise RuntimeError("draw_lines: canvas must be a CUDA tensor (there is no CPU fallback)")
        if canvas.dtype != torch.uint8 or canvas.dim() not in (3, 4) or canvas.shape[-1] != 4 or not canvas.is_contiguous():
            raise ValueError("draw_lines: canvas must be a contiguous (S, H, W, 4) or (H, W, 4) uint8 tensor")
        s = 1 if canvas.dim() == 3 else canvas.shape[0]
        h, w = canvas.shape[-3], canvas.shape[-2]
        data = canvas
        off = np.arange(s + 1, dtype=np.int64) * (h * w)
        shapes = np.tile(np.array([[h, w]], dtype=np.int64), (s, 1))
        resolution = RESOLUTION if resolution is None else resolution
    if not torch.cuda.is_available():
        raise RuntimeError("draw_lines needs a GPU (there is no CPU fallback)")
    dev = data.device
    segs, seg_line, st, lv = pack_lines(lines, line_view, styles, window, float(resolution))
    if len(np.asarray(window).reshape(-1, 4)) != len(shapes):
        raise ValueError("draw_lines: one window per view")
    if len(segs) == 0 or len(shapes) == 0:
        return canvas
    lib = L.lib()
    tile = lib.prh_bev_tile()
    ntx, nty = -(-shapes[:, 1] // tile), -(-shapes[:, 0] // tile)
    dims = np.stack([shapes[:, 0], shapes[:, 1], ntx, nty], 1).astype(np.int32)
    base = G.csr_offsets(ntx * nty)
    n_tiles = int(base[-1])
    if n_tiles == 0:
        return canvas
    tile_view = np.repeat(np.arange(len(shapes), dtype=np.int32), ntx * nty)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    segs_t, seg_line_t, st_t, lv_t, dims_t, base_t, off_t, tv_t = (up(a) for a in (segs, seg_line, st, lv, dims, base[:-1],
                                                                                   off, tile_view))
    counts = torch.empty((n_tiles,), dtype=torch.int32, device=dev)
    L.check(lib.prh_bev_draw_count(G.ptr(segs_t), G.ptr(seg_line_t), len(segs), G.ptr(st_t), G.ptr(lv_t), G.ptr(dims_t),
                                   G.ptr(base_t), n_tiles, G.ptr(counts), dev.index, G.stream(dev)), "prh_bev_draw_count")
    tile_off = G.exclusive_scan(counts)
    n_items = int(tile_off[-1].item())
    if n_items == 0:
        return canvas
    nb = lib.prh_bev_draw_workspace_bytes(n_tiles, n_items)
    ws = G.workspace(nb, dev)
    L.check(lib.prh_bev_draw(G.ptr(segs_t), G.ptr(seg_line_t), len(segs), G.ptr(st_t), G.ptr(lv_t), G.ptr(dims_t), G.ptr(base_t),
                             G.ptr(off_t), G.ptr(tv_t), G.ptr(tile_off), n_tiles, n_items, G.ptr(data), G.ptr(ws), nb,
                             dev.index, G.stream(dev)), "prh_bev_draw")
    return canvas


def chamfer_xy(gt_lines, pred_lines):
    """calc_metric (:154-176) for batches of line pairs: (mean over GT vertices of the xy distance
    to the nearest prediction vertex + the same the other way) / 2, float64 (n,) numpy; -1.0 where
    the GT is None or empty.  Two predictions.line_costs calls, every pair a frame of its own."""
    from .predictions import line_costs
    if len(gt_lines) != len(pred_lines):
        raise ValueError("chamfer_xy: one prediction per GT line")
    G.device("bev")
    out = np.full(len(gt_lines), -1.0)
    idx = [i for i, g in enumerate(gt_lines) if g is not None and len(g) > 0]
    if idx:
        g = [_line(gt_lines[i]) for i in idx]
        p = [_line(pred_lines[i]) for i in idx]
        frames = np.arange(len(idx) + 1, dtype=np.int64)
        g2p = line_costs(g, frames, p, frames)[0].cpu().numpy()
        p2g = line_costs(p, frames, g, frames)[0].cpu().numpy()
        out[idx] = (g2p + p2g) / 2.0
    return out


def render_scene(model, pcd_points, items, out_dir=None, name=None, num_line_points=32, num_context_points=2048,
                 crop_radius=0.5, resolution=RESOLUTION):
    """main()'s body for one scene (:132-271).  pcd_points (P, >=4) float32 or float64, numpy or CUDA;
    items: io.load_scene_items' list.  The scene image (bev_map, tone_map, 'jet'), one view per
    item item_windows keeps, the first candidate of each item (if it has two vertices or more)
    refined through io.refine_scene - all of the scene in one call - and GT (if more than one
    vertex), candidate and refined line drawn in that order.  Returns {'views' Views, 'items' [item
    index of each view], 'windows' (K,4), 'err_noisy' / 'err_refined' (K,) float64: calc_metric
    against the resampled GT, -1.0 without a GT, NaN without a candidate, 'refined' / 'noisy' [(M,3)
    or None per view], 'image', 'extent', 'p'}.  With out_dir: NAME_item_K.png per view (K the item
    index) and NAME.json with the window and the reference's legend labels per item.  No text is
    drawn into the image."""
    from .context import resample_polyline
    from .io import refine_scene
    if not torch.cuda.is_available():
        raise RuntimeError("render_scene needs a GPU (there is no CPU fallback)")
    image, extent = bev_map(pcd_points, resolution)
    norm, p = tone_map(image)
    rgba = colorize(norm, image, "jet")
    windows, kept = item_windows(items)
    views = crop_views(rgba, extent, windows, resolution)
    gts, cands = [], []
    for idx in kept:
        gt = _line(items[idx].get("position"))
        gts.append(gt if len(gt) > 1 else None)
        c = [_line(c) for c in items[idx].get("noisy_candidates", []) or []][:1]
        cands.append(c[0] if c and len(c[0]) >= 2 else None)
    rows = [k for k, c in enumerate(cands) if c is not None]
    refined, noisy = refine_scene(model, pcd_points, [cands[k][:, :3] for k in rows], num_line_points,
                                  num_context_points, crop_radius)
    ref_of, noisy_of = [None] * len(kept), [None] * len(kept)
    for r, k in enumerate(rows):
        ref_of[k], noisy_of[k] = refined[r], noisy[r]
    err_noisy, err_refined = np.full(len(kept), np.nan), np.full(len(kept), np.nan)
    if rows:
        gt_res = [resample_polyline(gts[k][:, :3], num_line_points) if gts[k] is not None else None for k in rows]
        err_noisy[rows] = chamfer_xy(gt_res, [noisy_of[k] for k in rows])
        err_refined[rows] = chamfer_xy(gt_res, [ref_of[k] for k in rows])
    lines, line_view, styles = [], [], []
    for k in range(len(kept)):
        for line, style in ((gts[k], STYLE_GT), (cands[k], STYLE_NOISY), (ref_of[k], STYLE_REFINED)):
            if line is not None:
                lines.append(line); line_view.append(k); styles.append(style)
    draw_lines(views, None, lines, line_view, styles)
    res = {"views": views, "items": kept, "windows": views.windows, "err_noisy": err_noisy, "err_refined": err_refined,
           "refined": ref_of, "noisy": noisy_of, "image": image, "extent": extent, "p": p}
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        name = "scene" if name is None else name
        host = views.data.cpu().numpy()
        doc = {"resolution": float(resolution), "items": []}
        for k, idx in enumerate(kept):
            h, w = views.shapes[k]
            png = f"{name}_item_{idx}.png"
            write_png(os.path.join(out_dir, png), host[views.offsets[k]:views.offsets[k + 1]].reshape(h, w, 4))
            entry = {"item": int(idx), "file": png, "window": [float(v) for v in views.windows[k]]}
            if cands[k] is not None:
                entry.update(err_noisy=float(err_noisy[k]), err_refined=float(err_refined[k]),
                             noisy_label=f"Noisy (E={err_noisy[k]:.2f}m)", refined_label=f"Refined (E={err_refined[k]:.2f}m)")
            doc["items"].append(entry)
        with open(os.path.join(out_dir, f"{name}.json"), "w") as f:
            json.dump(doc, f, indent=4)
    return res


def render_sample(context, noisy, pred_offset, gt_offset, resolution=0.02, padding=0.5):
    """The training picture (train_dist.py:18-56) of sample 0 of a batch: the context points (B, N,
    4) as a 'gray' BEV at a fixed resolution over the points' own bounds (+ padding), brightest
    point of a pixel shown, scaled by the largest intensity; on top the noisy line (B, M, 3) dashed
    red, noisy + gt_offset lime and noisy + pred_offset cyan, in the reference's order.  Returns
    (H, W, 4) uint8 CUDA."""
    if not torch.cuda.is_available():
        raise RuntimeError("render_sample needs a GPU (there is no CPU fallback)")
    ctx = context[0].detach().to(torch.float32)
    image, extent = bev_map(ctx, resolution, padding)
    norm, _ = tone_map(image, 100.0, 1.0)
    canvas = colorize(norm, image, "gray")
    line = noisy[0].detach().double().cpu().numpy()
    gt = line + gt_offset[0].detach().double().cpu().numpy()
    pred = line + pred_offset[0].detach().double().cpu().numpy()
    h, w = image.shape
    y_min, x_max = float(extent[0]), float(extent[3])
    window = [y_min, y_min + w * resolution, x_max - h * resolution, x_max]
    draw_lines(canvas, window, [line, gt, pred], [0, 0, 0], [STYLE_NOISY, STYLE_SAMPLE_GT, STYLE_SAMPLE_PRED], resolution)
    return canvas
