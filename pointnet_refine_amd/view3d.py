"""3-D scene views: the reference's Plotly and matplotlib viewers (inference_whole_scene.py:242-404,
tools/visualize_data.py:58-144, check_global_align.py, visualize_sampled_pointcloud.py:11-113)
without either library and without their point caps - every point of the cloud is splatted into a
64-bit depth buffer on the GPU (``csrc/prh_view.hpp``), polylines are drawn into the same buffer
and the finished views leave the device as RGBA and depth images.  The rule - camera rows,
projection, depth word, splat, lines, resolve - is written down in include/pointnet_refine_hip.h
("3-D views - the rule"); images are the same bits every run.

  orbit_camera / fit_camera   host: fp64 camera rows (matplotlib's view_init angles, degrees)
  view_bounds                 HIP: min / max of x, y, z
  new_zbuffer                 HIP: (V, H, W) depth words, all empty
  splat_points                HIP: one pass over the cloud, every camera of the call
  pack_lines3d / draw_lines3d host: near-plane cut and projection in numpy fp64; HIP: coverage
  resolve                     HIP: words -> (RGBA, float32 depth)
  viridis_table               host: matplotlib's 'viridis' as a literal (bev.jet_table / gray_table beside it)
  render_scene3d              inference_whole_scene.py's figure for one scene
  render_sample3d             visualize_sampled_pointcloud.py's figure of sample 0 of a batch
  render_cloud3d              visualize_data.py's / check_global_align.py's figure
  render_drive3d              check_global_align.py's figure of a drive directory: the merged cloud
                              against its GT, and every slice in its own view (one CSR splat)

Edges are hard: there is no blending and no transparency (the reference's opacity values are not
reproduced).  The GPU functions have no CPU fallback: without a GPU they raise RuntimeError.
"""
import json
import math
import os

import numpy as np
import torch

from . import _gpu as G
from . import _lib as L
from .bev import _line, _points_t, gray_table, jet_table, write_png  # noqa: F401  (tables re-exported)

MAX_LINES = 1 << 24
LINE_BIAS = 0.15             # metres: lifts a line lying on the road in front of the road's own points
# colours of the reference's traces (CSS names as Plotly / matplotlib resolve them)
STYLE_CONTEXT_GT = {"color": (255, 165, 0), "width": 2.0, "marker": 0.0, "dash": None, "bias": LINE_BIAS}
STYLE_GT = {"color": (0, 128, 0), "width": 2.0, "marker": 0.0, "dash": None, "bias": LINE_BIAS}
STYLE_NOISY = {"color": (255, 0, 0), "width": 1.5, "marker": 0.0, "dash": (9.0, 6.0), "bias": LINE_BIAS}
STYLE_REFINED = {"color": (255, 0, 255), "width": 2.0, "marker": 4.0, "dash": None, "bias": LINE_BIAS}
STYLE_SAMPLE_NOISY = {"color": (255, 0, 0), "width": 2.0, "marker": 5.0, "dash": None, "bias": LINE_BIAS}
STYLE_SAMPLE_GT = {"color": (0, 128, 0), "width": 2.0, "marker": 5.0, "dash": None, "bias": LINE_BIAS}
CATEGORY_COLORS = {"lane_line": (255, 0, 0), "curb": (255, 165, 0)}       # visualize_data.py: anything else blue
OTHER_COLOR = (0, 0, 255)
CANDIDATE_COLORS = ((0, 255, 255), (255, 255, 0), (255, 0, 255))          # cyan, yellow, magenta


# ------------------------------------------------------------------ host side: cameras
def _cos_sin_deg(angle):
    """cos and sin of an angle in degrees, exact (0, +-1) at multiples of 90."""
    a = math.fmod(float(angle), 360.0)
    q = a / 90.0
    if q == math.floor(q):
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
    r = math.radians(a)
    return math.cos(r), math.sin(r)


def _pixel_scale(fov, height):
    if not 0.0 < fov < 180.0:
        raise ValueError("camera: fov must lie in (0, 180) degrees")
    return (height / 2.0) / math.tan(math.radians(fov) / 2.0)


def orbit_camera(target, elev, azim, distance, fov=40.0, ortho_scale=None, near=0.1, height=720, width=960):
    """The camera row (16,) float64 of an orbit camera about target (3,) at elevation elev and
    azimuth azim (degrees, matplotlib's view_init convention: azim turns about +z from +x, elev lifts
    the eye above the xy plane) at `distance` metres.  Perspective with a vertical field of view of
    fov degrees, or orthographic at ortho_scale pixels per metre when that is given.  near: points
    and line parts nearer than this (along the view direction) are not drawn; it must not be
    negative, and must be positive in a perspective view.  width is not used by the row (the image
    centre is taken from the buffer); it is accepted so that a camera is described in one place."""
    c = np.asarray(target, dtype=np.float64).reshape(3)
    ce, se = _cos_sin_deg(elev)
    ca, sa = _cos_sin_deg(azim)
    if not (np.isfinite(c).all() and math.isfinite(distance) and distance >= 0.0):
        raise ValueError("orbit_camera: target and distance must be finite, distance not negative")
    ortho = ortho_scale is not None
    if near < 0.0 or (not ortho and not near > 0.0):
        raise ValueError("orbit_camera: near must be positive (not negative in an orthographic view)")
    if height < 1 or width < 1:
        raise ValueError("orbit_camera: height and width must be at least 1")
    out_dir = np.array([ce * ca, ce * sa, se])
    row = np.zeros(16, dtype=np.float64)
    row[0:3] = c + float(distance) * out_dir
    row[3:6] = (-sa, ca, 0.0)
    row[6:9] = (-se * ca, -se * sa, ce)
    row[9:12] = -out_dir
    if ortho:
        if not (math.isfinite(ortho_scale) and ortho_scale > 0.0):
            raise ValueError("orbit_camera: ortho_scale must be positive")
        row[12] = float(ortho_scale)
    else:
        row[12] = _pixel_scale(float(fov), height)
    row[13] = float(near)
    row[14] = 1.0 if ortho else 0.0
    return row + 0.0          # -0.0 -> +0.0


def _bounds_of(points_or_bounds):
    b = points_or_bounds
    if not torch.is_tensor(b):
        b = np.asarray(b)
        if b.shape == (2, 3) or b.shape == (6,):
            b = b.astype(np.float64).reshape(2, 3) if b.shape == (2, 3) else b.astype(np.float64).reshape(3, 2).T
            return b[0].copy(), b[1].copy()
    return view_bounds(b)


def fit_camera(points_or_bounds, elev, azim, fov=40.0, ortho=False, near=0.1, height=720, width=960, margin=1.05,
               target=None):
    """orbit_camera looking at the centre of a bounding box - of points (n, >=4) (view_bounds, on
    the GPU), or given as ((x_min, y_min, z_min), (x_max, y_max, z_max)) or (x_min, x_max, y_min,
    y_max, z_min, z_max) - from a distance at which the box's bounding sphere (radius * margin)
    fits into the image on both axes.  ortho=True: orthographic, the sphere's diameter across the
    shorter image side.  target: look there instead (the sphere then is the one about target that
    holds the box)."""
    lo, hi = _bounds_of(points_or_bounds)
    if target is None:
        c = (lo + hi) / 2.0
        radius = float(np.sqrt((((hi - lo) / 2.0) ** 2).sum()))
    else:
        c = np.asarray(target, dtype=np.float64).reshape(3)
        radius = float(np.sqrt((np.maximum(np.abs(lo - c), np.abs(hi - c)) ** 2).sum()))
    radius = max(radius * float(margin), 1e-6)
    if ortho:
        return orbit_camera(c, elev, azim, radius + near, ortho_scale=(min(height, width) / 2.0) / radius, near=near,
                            height=height, width=width)
    s = _pixel_scale(float(fov), height)
    half = math.atan2(min(height, width) / 2.0, s)                # the narrower half-angle
    distance = max(radius / math.sin(half), radius + near)
    return orbit_camera(c, elev, azim, distance, fov=fov, near=near, height=height, width=width)


def _cameras(cameras):
    cams = np.ascontiguousarray(np.asarray(cameras, dtype=np.float64).reshape(-1, 16))
    if not np.isfinite(cams).all():
        raise ValueError("cameras must be finite")
    return cams


# ------------------------------------------------------------------ GPU side
def _need_gpu(what):
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} needs a GPU (there is no CPU fallback)")


def _zbuf(zbuf, what):
    _need_gpu(what)
    if not torch.is_tensor(zbuf) or not zbuf.is_cuda:
        raise RuntimeError(f"{what}: zbuf must be a CUDA tensor (there is no CPU fallback)")
    if zbuf.dtype != torch.int64 or zbuf.dim() != 3 or not zbuf.is_contiguous():
        raise ValueError(f"{what}: zbuf must be a contiguous (V, H, W) int64 tensor (new_zbuffer)")
    return zbuf


def view_bounds(points):
    """(lo (3,), hi (3,)) float64: the bounding box of x, y, z of points (n, >=4), exact.
    ValueError for n = 0 and for a NaN or infinite x, y, z or intensity."""
    dev = G.device("view3d")
    p = _points_t(points, dev, "view_bounds")
    dev = p.device
    if p.shape[0] == 0:
        raise ValueError("view_bounds: zero-size array of points has no minimum")
    lib = L.lib()
    nb = lib.prh_view_bounds_workspace_bytes()
    ws = G.workspace(nb, dev)
    info = torch.empty((7,), dtype=torch.float64, device=dev)
    L.check(lib.prh_view_bounds(G.ptr(p), p.shape[0], int(p.dtype == torch.float64), G.ptr(info), G.ptr(ws), nb,
                                dev.index, G.stream(dev)), "prh_view_bounds")
    info = info.cpu().numpy()
    if info[6] != 0.0:
        raise ValueError("view_bounds: a NaN or infinite x, y, z or intensity")
    return info[0:6:2].copy(), info[1:6:2].copy()


def new_zbuffer(n_views, height, width, device=None):
    """(V, H, W) int64 CUDA: one depth word per pixel, (bits(float32(depth)) << 32) | payload, all
    ones (-1) = empty.  View it as uint64 on the host to compare words."""
    dev = G.device("view3d", device)
    if n_views < 0 or height < 1 or width < 1:
        raise ValueError("new_zbuffer: n_views >= 0, height and width >= 1")
    z = torch.empty((int(n_views), int(height), int(width)), dtype=torch.int64, device=dev)
    L.check(L.lib().prh_view_clear(G.ptr(z), int(n_views), int(height), int(width), dev.index, G.stream(dev)),
            "prh_view_clear")
    return z


def splat_points(zbuf, points, cameras, size, cmin, cmax, offsets=None, slice_view=None):
    """Every point of points (n, >=4) float32 or float64 (numpy or CUDA) into every view of zbuf
    (V, H, W) under cameras (V, 16), as size x size pixels (1..9) with the colour index of its
    intensity between cmin and cmax; in place, returns zbuf.  offsets (S+1,) with slice_view: the
    cloud is a CSR of slices (what drive.slice_cloud returns) and slice s is drawn only into its own
    views - slice_view (S,) ints (one view each, -1 none), a list of S lists of views, or an (S, V)
    mask.  The cloud is read once.  ValueError for a NaN or infinite x, y, z or intensity."""
    z = _zbuf(zbuf, "splat_points")
    dev = z.device
    p = _points_t(points, dev, "splat_points")
    if p.device != dev:
        raise ValueError("splat_points: points and zbuf must be on one device")
    cams = _cameras(cameras)
    v, h, w = z.shape
    if len(cams) != v:
        raise ValueError(f"splat_points: {len(cams)} cameras for {v} views")
    if not 1 <= int(size) <= 9:
        raise ValueError("splat_points: size must be 1..9")
    cmin, cmax = float(cmin), float(cmax)
    if not (math.isfinite(cmin) and math.isfinite(cmax) and cmax > cmin):
        raise ValueError("splat_points: cmin < cmax, both finite")
    off_t = mask = None
    n_slices = 0
    if (offsets is None) != (slice_view is None):
        raise ValueError("splat_points: offsets and slice_view go together")
    if offsets is not None:
        oh = (offsets.detach().cpu().numpy() if torch.is_tensor(offsets) else np.asarray(offsets)).astype(np.int64).reshape(-1)
        if len(oh) < 2 or oh[0] != 0 or oh[-1] != p.shape[0] or np.any(np.diff(oh) < 0):
            raise ValueError(f"splat_points: offsets must rise from 0 to the number of points ({p.shape[0]})")
        n_slices = len(oh) - 1
        mask = _slice_mask(slice_view, n_slices, v)
        off_t = torch.from_numpy(oh).to(dev)
    lib = L.lib()
    step = lib.prh_view_max_views()
    bad = torch.zeros((1,), dtype=torch.int32, device=dev)
    for v0 in range(0, v, step):
        v1 = min(v0 + step, v)
        cam_t = torch.from_numpy(cams[v0:v1].copy()).to(dev)
        mask_t = torch.from_numpy(np.ascontiguousarray(mask[:, v0:v1])).to(dev) if mask is not None else None
        L.check(lib.prh_view_splat(G.ptr(p), p.shape[0], int(p.dtype == torch.float64), G.ptr(cam_t), v1 - v0,
                                   G.ptr(off_t) if off_t is not None else None, n_slices,
                                   G.ptr(mask_t) if mask_t is not None else None, int(size), cmin, cmax, h, w,
                                   G.ptr(z[v0:v1]), G.ptr(bad), dev.index, G.stream(dev)), "prh_view_splat")
        if int(bad.item()):
            raise ValueError("splat_points: a NaN or infinite x, y, z or intensity")
    return zbuf


def _slice_mask(slice_view, n_slices, n_views):
    mask = np.zeros((n_slices, n_views), dtype=np.uint8)
    sv = slice_view.detach().cpu().numpy() if torch.is_tensor(slice_view) else slice_view
    if isinstance(sv, np.ndarray) and sv.ndim == 2:
        if sv.shape != (n_slices, n_views):
            raise ValueError("splat_points: a slice_view mask must be (slices, views)")
        return np.ascontiguousarray(sv != 0, dtype=np.uint8)
    if len(sv) != n_slices:
        raise ValueError("splat_points: one slice_view entry per slice")
    for s, views in enumerate(sv):
        for k in np.atleast_1d(np.asarray(views, dtype=np.int64)):
            if k == -1:
                continue
            if not 0 <= k < n_views:
                raise ValueError("splat_points: a slice names a view that does not exist")
            mask[s, k] = 1
    return mask


def _style_rows(styles):
    st = np.zeros((len(styles), 8), dtype=np.float64)
    for l, s in enumerate(styles):
        dash = s.get("dash") or (0.0, 0.0)
        st[l] = [*s["color"], s.get("width", 0.0), s.get("marker", 0.0), dash[0], dash[1], s.get("bias", 0.0)]
    if not np.isfinite(st).all() or (st[:, 3:7] < 0).any():
        raise ValueError("styles: width, marker and dash must be finite and not negative")
    return st


def pack_lines3d(lines, styles, cameras, height, width, line_views=None):
    """The host half of draw_lines3d, in numpy fp64: every (polyline, view) pair - line l in the
    views line_views[l] (None: every view) - taken to view space, each segment cut to d >= near by
    linear interpolation there, projected without the floor.  A line of one vertex gives one
    zero-length segment (its marker).  Returns (segments (n, 8) = ax ay bx by arc_a L wa wb,
    segment_ids (n, 2) int32 = line, view, styles (L, 8) = r g b width marker dash_on dash_off bias)."""
    cams = _cameras(cameras)
    if len(styles) != len(lines):
        raise ValueError("draw_lines3d: one style per line")
    if len(lines) > MAX_LINES:
        raise ValueError("draw_lines3d: at most 2^24 lines")
    st = _style_rows(styles)
    half_w, half_h = width / 2.0, height / 2.0
    segs, ids = [], []
    for l, line in enumerate(lines):
        a = _line(line)
        if len(a) == 0:
            continue
        if a.shape[1] < 3:
            a = np.column_stack([a, np.zeros(len(a))])
        views = range(len(cams)) if line_views is None or line_views[l] is None else np.atleast_1d(line_views[l])
        for v in views:
            v = int(v)
            if not 0 <= v < len(cams):
                raise ValueError("draw_lines3d: a line names a view that does not exist")
            cam = cams[v]
            near, ortho, s = cam[13], cam[14] != 0.0, cam[12]
            q = a[:, :3] - cam[0:3]
            vs = np.stack([(q[:, 0] * cam[3 + 3 * j] + q[:, 1] * cam[4 + 3 * j]) + q[:, 2] * cam[5 + 3 * j] for j in range(3)], 1)
            if len(vs) == 1:
                p0, p1 = vs, vs
            else:
                p0, p1 = vs[:-1], vs[1:]
            in0, in1 = p0[:, 2] >= near, p1[:, 2] >= near
            keep = in0 | in1
            if not keep.any():
                continue
            p0, p1, in0, in1 = p0[keep].copy(), p1[keep].copy(), in0[keep], in1[keep]
            with np.errstate(divide="ignore", invalid="ignore"):      # rows that are not cut are not used
                t = (near - p0[:, 2]) / (p1[:, 2] - p0[:, 2])
                cut = p0 + t[:, None] * (p1 - p0)
            cut[:, 2] = near
            p0[~in0] = cut[~in0]
            p1[~in1] = cut[~in1]
            k0 = np.full(len(p0), s) if ortho else s / p0[:, 2]
            k1 = np.full(len(p1), s) if ortho else s / p1[:, 2]
            ax, ay = half_w + p0[:, 0] * k0, half_h - p0[:, 1] * k0
            bx, by = half_w + p1[:, 0] * k1, half_h - p1[:, 1] * k1
            ex, ey = bx - ax, by - ay
            length = np.sqrt(ex * ex + ey * ey)
            arc = np.concatenate(([0.0], np.cumsum(length)[:-1]))
            wa, wb = (p0[:, 2], p1[:, 2]) if ortho else (1.0 / p0[:, 2], 1.0 / p1[:, 2])
            segs.append(np.column_stack([ax, ay, bx, by, arc, length, wa, wb]))
            ids.append(np.column_stack([np.full(len(ax), l), np.full(len(ax), v)]).astype(np.int32))
    segs = np.concatenate(segs) if segs else np.zeros((0, 8))
    ids = np.concatenate(ids) if ids else np.zeros((0, 2), dtype=np.int32)
    return np.ascontiguousarray(segs), np.ascontiguousarray(ids), st


def draw_lines3d(zbuf, lines, styles, cameras, line_views=None):
    """Polylines into the depth buffer, in place; returns zbuf.  lines: (n, 3) arrays in metres;
    styles[l]: a dict of 'color' (RGB 0..255), 'width' (pixels; 0: no strokes), 'marker' (vertex
    disc diameter in pixels; 0: none), 'dash' ((on, off) pixels along the screen path from the first
    drawn vertex, or None) and 'bias' (metres subtracted from the line's depth).  Line l carries the
    payload l: resolve colours it with styles[l], so give resolve the same list.  Work scales with
    the segments' bounding boxes on screen."""
    z = _zbuf(zbuf, "draw_lines3d")
    dev = z.device
    cams = _cameras(cameras)
    v, h, w = z.shape
    if len(cams) != v:
        raise ValueError(f"draw_lines3d: {len(cams)} cameras for {v} views")
    segs, ids, st = pack_lines3d(lines, styles, cams, h, w, line_views)
    if len(segs) == 0 or v == 0:
        return zbuf
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    segs_t, ids_t, st_t, cam_t = up(segs), up(ids), up(st), up(cams)
    L.check(L.lib().prh_view_lines(G.ptr(segs_t), G.ptr(ids_t), len(segs), G.ptr(st_t), len(st), G.ptr(cam_t), v, h, w,
                                   G.ptr(z), dev.index, G.stream(dev)), "prh_view_lines")
    return zbuf


def _pack_rgb(rgb):
    c = np.clip(np.rint(np.asarray(rgb, dtype=np.float64).reshape(-1, 3)), 0, 255).astype(np.uint32)
    return (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | np.uint32(0xff000000)).astype(np.uint32)


def resolve(zbuf, table, styles=(), background=(0, 0, 0)):
    """(rgba (V, H, W, 4) uint8 CUDA, depth (V, H, W) float32 CUDA) of a depth buffer: an empty
    pixel shows background and depth +inf, a point table[lut] ((256, 4) uint8: jet_table(),
    gray_table(), viridis_table()), a line styles[l]['color']; alpha is 255."""
    z = _zbuf(zbuf, "resolve")
    dev = z.device
    tab = np.ascontiguousarray(np.asarray(table, dtype=np.uint8).reshape(256, 4))
    tab_t = torch.from_numpy(tab.view(np.uint32).reshape(-1).view(np.int32)).to(dev)
    col = _pack_rgb([s["color"] for s in styles]) if len(styles) else np.zeros(0, dtype=np.uint32)
    col_t = torch.from_numpy(col.view(np.int32)).to(dev)
    rgba = torch.empty(tuple(z.shape) + (4,), dtype=torch.uint8, device=dev)
    depth = torch.empty(tuple(z.shape), dtype=torch.float32, device=dev)
    L.check(L.lib().prh_view_resolve(G.ptr(z), z.numel(), G.ptr(tab_t), G.ptr(col_t), len(col), int(_pack_rgb(background)[0]),
                                     G.ptr(rgba), G.ptr(depth), dev.index, G.stream(dev)), "prh_view_resolve")
    return rgba, depth


# ------------------------------------------------------------------ tools
def _render(points, cameras, height, width, size, cmin, cmax, table, lines, styles, background=(0, 0, 0)):
    cams = _cameras(cameras)
    z = new_zbuffer(len(cams), height, width, points.device if torch.is_tensor(points) and points.is_cuda else None)
    splat_points(z, points, cams, size, cmin, cmax)
    draw_lines3d(z, lines, styles, cams)
    rgba, depth = resolve(z, table, styles, background)
    return z, rgba, depth


def _write(out_dir, name, rgba, doc):
    os.makedirs(out_dir, exist_ok=True)
    host = rgba.cpu().numpy()
    for k, view in enumerate(doc["views"]):
        write_png(os.path.join(out_dir, view["file"]), host[k])
    with open(os.path.join(out_dir, f"{name}.json"), "w") as f:
        json.dump(doc, f, indent=4)


def _lines_bounds(lines, pad):
    v = np.concatenate([l[:, :3] for l in lines])
    return np.stack([v.min(0) - pad, v.max(0) + pad])


def render_scene3d(model, pcd_points, items, out_dir=None, name=None, closeups=False, num_line_points=32,
                   num_context_points=1024, crop_radius=0.3, height=720, width=960, point_size=2, elev=35.0,
                   azim=180.0, closeup_pad=5.0):
    """inference_whole_scene.py's figure (:242-404) for one scene, every point drawn.  The whole
    cloud in 'jet' between intensity 1 and 40; view 0 looks at the ego origin from behind and above
    (azim 180, elev 35) from where the cloud's bounding sphere fits; closeups=True adds one view per
    item that has a line, fitted to that item's lines +- closeup_pad.  Lines, in the reference's
    order: the context GT of item 0 orange, per item the GT (more than one vertex) green and per
    candidate of two vertices or more the resampled noisy line red dashed and the refined line
    magenta with vertex markers (metrics.evaluate_scene: the same refinement and metrics as the
    evaluation tool).  Returns {'rgba' (V, H, W, 4), 'depth', 'zbuf', 'cameras' (V, 16), 'lines',
    'styles', 'labels': the reference's legend names, metric strings included, one per line,
    'view_items': the item of each view (-1: the overview), 'eval': evaluate_scene's dict}.  With
    out_dir: NAME_view_K.png per view and NAME.json with cameras and labels.  No text is drawn."""
    from .metrics import evaluate_scene
    _need_gpu("render_scene3d")
    dev = G.device("view3d")
    pts = _points_t(pcd_points, dev, "render_scene3d")
    ev = evaluate_scene(model, pts, items, num_line_points, num_context_points, crop_radius)
    lines, styles, labels = [], [], []
    if len(items):
        for c in items[0].get("context_lines", []) or []:
            c = _line(c)
            if len(c):
                lines.append(c); styles.append(STYLE_CONTEXT_GT); labels.append("Context GT")
    per_item = [[] for _ in items]
    row = 0
    for i, item in enumerate(items):
        gt = _line(item.get("position"))
        if len(gt) > 1:
            lines.append(gt); styles.append(STYLE_GT); labels.append(f"GT Line {i}")
            per_item[i].append(gt)
        for cand in item.get("noisy_candidates", []) or []:
            if len(_line(cand)) < 2:
                continue
            info = ""
            if ev["valid"][row]:
                info = (f"<br>{'(Bad Match) ' if ev['bad_match'][row] else ''}ADE: {ev['ade_noisy'][row]:.2f}->"
                        f"{ev['ade_refined'][row]:.2f}<br>Lat: {ev['lat_noisy'][row]:.2f}->{ev['lat_refined'][row]:.2f}")
            lines += [ev["noisy"][row], ev["refined"][row]]
            styles += [STYLE_NOISY, STYLE_REFINED]
            labels += [f"Noisy {i}{info}", f"Refined {i}"]
            per_item[i] += [ev["noisy"][row], ev["refined"][row]]
            row += 1
    lo, hi = view_bounds(pts)
    cams = [fit_camera((lo, hi), elev, azim, height=height, width=width, target=(0.0, 0.0, 0.0))]
    view_items = [-1]
    if closeups:
        for i, ls in enumerate(per_item):
            if ls:
                cams.append(fit_camera(_lines_bounds(ls, closeup_pad), elev, azim, height=height, width=width))
                view_items.append(i)
    cams = np.stack(cams)
    z, rgba, depth = _render(pts, cams, height, width, point_size, 1.0, 40.0, jet_table(), lines, styles)
    res = {"rgba": rgba, "depth": depth, "zbuf": z, "cameras": cams, "lines": lines, "styles": styles, "labels": labels,
           "view_items": view_items, "eval": ev}
    if out_dir is not None:
        name = "scene3d" if name is None else name
        doc = {"height": int(height), "width": int(width), "cmap": "jet", "cmin": 1.0, "cmax": 40.0,
               "views": [{"file": f"{name}_view_{k}.png", "item": int(view_items[k]), "camera": [float(x) for x in cams[k]]}
                         for k in range(len(cams))],
               "lines": [{"label": labels[l], "color": [int(c) for c in styles[l]["color"]]} for l in range(len(lines))]}
        _write(out_dir, name, rgba, doc)
    return res


def render_sample3d(context, noisy, target_offset, out_dir=None, name=None, height=600, width=800, point_size=3,
                    elev=20.0, azim=60.0):
    """visualize_sampled_pointcloud.py's figure (:11-113) of sample 0 of a batch - what the network
    sees: the context points (B, N, 4) in 'viridis' over their own intensity range, the noisy line
    (B, M, 3) red and the GT noisy + target_offset green, both with vertex markers, at elev 20,
    azim 60, the camera fitted to the points.  Returns {'rgba' (H, W, 4), 'depth', 'zbuf', 'cameras',
    'labels'}; the inputs are not modified."""
    _need_gpu("render_sample3d")
    ctx = context[0].detach().to(torch.float32).contiguous()
    line = noisy[0].detach().double().cpu().numpy()
    gt = line + target_offset[0].detach().double().cpu().numpy()
    inten = ctx[:, 3]
    cmin, cmax = float(inten.min()), float(inten.max())
    if not cmax > cmin:
        cmax = cmin + 1.0
    lo, hi = view_bounds(ctx)
    both = _lines_bounds([line, gt], 0.0)
    cams = fit_camera((np.minimum(lo, both[0]), np.maximum(hi, both[1])), elev, azim, height=height, width=width)[None]
    styles, labels = [STYLE_SAMPLE_NOISY, STYLE_SAMPLE_GT], ["Noisy Line", "GT Line"]
    z, rgba, depth = _render(ctx, cams, height, width, point_size, cmin, cmax, viridis_table(), [line, gt], styles,
                             background=(255, 255, 255))
    if out_dir is not None:
        name = "sample3d" if name is None else name
        _write(out_dir, name, rgba, {"height": int(height), "width": int(width), "cmap": "viridis", "cmin": cmin, "cmax": cmax,
                                     "views": [{"file": f"{name}.png", "camera": [float(x) for x in cams[0]]}],
                                     "lines": [{"label": labels[l], "color": list(styles[l]["color"])} for l in range(2)]})
    return {"rgba": rgba[0], "depth": depth[0], "zbuf": z, "cameras": cams, "labels": labels}


def _category_style(category, bias=LINE_BIAS):
    return {"color": CATEGORY_COLORS.get(category, OTHER_COLOR), "width": 3.0, "marker": 0.0, "dash": None, "bias": bias}


def _footprint_bias(cam, target, elev, point_size):
    """LINE_BIAS plus the depth a splat's footprint spans on level ground at the camera's target:
    zoomed out, a pixel holds metres of road, and the nearest of its points would hide a line on it."""
    metres_per_pixel = 1.0 / cam[12] if cam[14] != 0.0 else float(np.linalg.norm(cam[0:3] - np.asarray(target))) / cam[12]
    return LINE_BIAS + point_size * metres_per_pixel / max(math.tan(math.radians(abs(elev))), 0.1)


def render_cloud3d(points, lines, categories=None, candidates=None, out_dir=None, name=None, height=720, width=960,
                   point_size=2, elev=30.0, azim=-60.0):
    """visualize_data.py's (:58-144) and check_global_align.py's figure: the cloud (every point) in
    'viridis' between intensity 0 and 30, the GT lines coloured by categories[l] ('lane_line' red,
    'curb' orange, anything else or None blue) and up to three noisy candidates in cyan, yellow and
    magenta, the camera fitted to the cloud.  Returns {'rgba' (H, W, 4), 'depth', 'zbuf', 'cameras',
    'labels'}; the inputs are not modified."""
    _need_gpu("render_cloud3d")
    dev = G.device("view3d")
    pts = _points_t(points, dev, "render_cloud3d")
    all_lines, styles, labels = [], [], []
    for l, line in enumerate(lines):
        cat = categories[l] if categories is not None else None
        all_lines.append(_line(line))
        styles.append(_category_style(cat))
        labels.append(f"GT: {cat}" if cat is not None else f"GT Line {l}")
    for k, cand in enumerate(candidates or []):
        all_lines.append(_line(cand))
        styles.append({"color": CANDIDATE_COLORS[k % 3], "width": 2.0, "marker": 0.0, "dash": (9.0, 6.0), "bias": LINE_BIAS})
        labels.append(f"Noisy {k}")
    cams = fit_camera(view_bounds(pts), elev, azim, height=height, width=width)[None]
    z, rgba, depth = _render(pts, cams, height, width, point_size, 0.0, 30.0, viridis_table(), all_lines, styles)
    if out_dir is not None:
        name = "cloud3d" if name is None else name
        _write(out_dir, name, rgba, {"height": int(height), "width": int(width), "cmap": "viridis", "cmin": 0.0, "cmax": 30.0,
                                     "views": [{"file": f"{name}.png", "camera": [float(x) for x in cams[0]]}],
                                     "lines": [{"label": labels[l], "color": list(styles[l]["color"])}
                                               for l in range(len(all_lines))]})
    return {"rgba": rgba[0], "depth": depth[0], "zbuf": z, "cameras": cams, "labels": labels}


def render_drive3d(drive_dir, gt_json, out_dir=None, name=None, max_slices=None, height=720, width=960, point_size=2,
                   elev=35.0, azim=180.0):
    """check_global_align.py's figure for a drive directory (pose/*.json and merged.pcd, the layout
    drive.slice_drive reads) and, beside it, what the slicer makes of the drive.  View 0: every point
    of the merged cloud against the GT polylines of gt_json, in the drive's own frame.  Views 1..S:
    the slices drive.plan_slices cuts (the first max_slices of them), each in its ego frame from
    behind and above its origin - all slices come out of one drive.slice_cloud call and go into
    their views in one splat_points call (offsets + slice_view), with the GT clipped to each slice
    (drive.clip_lines).  Colours as render_cloud3d; the lines' depth bias grows with the ground a
    pixel holds, so that a zoomed-out road does not hide the lines lying on it.  Returns {'rgba' (1 + S, H, W, 4), 'depth',
    'zbuf', 'cameras', 'lines', 'line_views', 'styles', 'labels', 'names': the pose name of each
    slice, 'points', 'offsets': slice_cloud's}.  With out_dir: NAME_merged.png, NAME_slice_POSE.png
    and NAME.json.  ValueError for a drive without poses or points."""
    from . import drive as D
    _need_gpu("render_drive3d")
    dev = G.device("view3d")
    poses = D.load_poses(os.path.join(drive_dir, "pose"))
    have = poses and os.path.exists(os.path.join(drive_dir, "merged.pcd"))
    cloud = D.load_merged_cloud(drive_dir) if have else np.zeros((0, 4))
    if cloud.shape[0] == 0 or cloud.shape[1] < 4:
        raise ValueError(f"render_drive3d: {drive_dir} has no poses or no points")
    cloud_t = torch.from_numpy(np.ascontiguousarray(cloud, dtype=np.float32)).to(dev)
    gt_items = D.load_gt_items(gt_json) if gt_json and os.path.exists(gt_json) else []
    chosen = D.plan_slices(poses)
    chosen = chosen if max_slices is None else chosen[:int(max_slices)]
    names = [poses[j]["filename_ts"] for j in chosen]
    n_s = len(chosen)
    lo, hi = view_bounds(cloud_t)
    cams = [fit_camera((lo, hi), elev, azim, height=height, width=width)]
    bias = _footprint_bias(cams[0], (lo + hi) / 2.0, elev, point_size)
    lines = [it["points"] for it in gt_items]
    styles = [_category_style(it["category"], bias) for it in gt_items]
    labels = [f"GT: {it['category']}" for it in gt_items]
    line_views = [[0] for _ in gt_items]
    points = offsets = None
    if n_s:
        pq = D.poses_xyzq(poses, chosen)
        points, offsets, _ = D.slice_cloud(cloud_t, pq)
        half = D.SEGMENT_LEN / 2.0
        box = view_bounds(points) if points.shape[0] else (np.array([-half, -half, -1.0]), np.array([half, half, 1.0]))
        cams += [fit_camera(box, elev, azim, height=height, width=width, target=(0.0, 0.0, 0.0))] * n_s
        bias = _footprint_bias(cams[1], (0.0, 0.0, 0.0), elev, point_size)
        for s, kept in enumerate(D.clip_lines(list(lines), pq) if lines else [[] for _ in chosen]):
            for l, v in kept:
                lines.append(v); styles.append(_category_style(gt_items[l]["category"], bias))
                labels.append(f"{names[s]} GT: {gt_items[l]['category']}"); line_views.append([1 + s])
    cams = np.stack(cams)
    z = new_zbuffer(1 + n_s, height, width, dev)
    splat_points(z[0:1], cloud_t, cams[0:1], point_size, 0.0, 30.0)
    if n_s and points.shape[0]:
        splat_points(z[1:], points, cams[1:], point_size, 0.0, 30.0, offsets=offsets, slice_view=np.arange(n_s))
    draw_lines3d(z, lines, styles, cams, line_views)
    rgba, depth = resolve(z, viridis_table(), styles)
    if out_dir is not None:
        name = "drive3d" if name is None else name
        files = [f"{name}_merged.png"] + [f"{name}_slice_{n}.png" for n in names]
        _write(out_dir, name, rgba, {"height": int(height), "width": int(width), "cmap": "viridis", "cmin": 0.0, "cmax": 30.0,
                                     "views": [{"file": files[k], "slice": names[k - 1] if k else None,
                                                "camera": [float(x) for x in cams[k]]} for k in range(1 + n_s)],
                                     "lines": [{"label": labels[l], "color": list(styles[l]["color"]), "views": line_views[l]}
                                               for l in range(len(lines))]})
    return {"rgba": rgba, "depth": depth, "zbuf": z, "cameras": cams, "lines": lines, "line_views": line_views,
            "styles": styles, "labels": labels, "names": names, "points": points, "offsets": offsets}


# ------------------------------------------------------------------ colour table
def viridis_table():
    """(256, 4) uint8: matplotlib's 'viridis' as bytes (its 256 listed colours, a byte is
    int(value * 255)); no matplotlib import."""
    rgb = np.frombuffer(bytes.fromhex(_VIRIDIS_HEX), dtype=np.uint8).reshape(256, 3)
    return np.column_stack([rgb, np.full(256, 255, dtype=np.uint8)])


_VIRIDIS_HEX = (
    "44015444025544035745055845065a45085b46095c460b5e460c5f460e61470f62471163471265471466471567471669"
    "47186a48196b481a6c481c6e481d6f481e70482071482172482273482374472575472676472777472878472a79472b7a"
    "472c7b462d7c462f7c46307d46317e45327f45347f453580453681443781443982433a83433b83433c84423d84423e85"
    "4240854141864142864043874044873f45873f47883e48883e49893d4a893d4b893d4c893c4d8a3c4e8a3b508a3b518a"
    "3a528b3a538b39548b39558b38568b38578c37588c37598c365a8c365b8c355c8c355d8c345e8d345f8d33608d33618d"
    "32628d32638d31648d31658d31668d30678d30688d2f698d2f6a8d2e6b8e2e6c8e2e6d8e2d6e8e2d6f8e2c708e2c718e"
    "2c728e2b738e2b748e2a758e2a768e2a778e29788e29798e287a8e287a8e287b8e277c8e277d8e277e8e267f8e26808e"
    "26818e25828e25838d24848d24858d24868d23878d23888d23898d22898d228a8d228b8d218c8d218d8c218e8c208f8c"
    "20908c20918c1f928c1f938b1f948b1f958b1f968b1e978a1e988a1e998a1e998a1e9a891e9b891e9c891e9d881e9e88"
    "1e9f881ea0871fa1871fa2861fa38620a48520a58521a68521a78422a78423a88323a98224aa8225ab8126ac8127ad80"
    "28ae7f29af7f2ab07e2bb17d2cb17d2eb27c2fb37b30b47a32b57a33b67935b77836b87738b97639b9763bba753dbb74"
    "3ebc7340bd7242be7144be7045bf6f47c06e49c16d4bc26c4dc26b4fc36951c46853c56755c66657c66559c7645bc862"
    "5ec96160c96062ca5f64cb5d67cc5c69cc5b6bcd596dce5870ce5672cf5574d05477d05279d1517cd24f7ed24e81d34c"
    "83d34b86d44988d5478bd5468dd64490d64392d74195d73f97d83e9ad83c9dd93a9fd938a2da37a5da35a7db33aadb32"
    "addc30afdc2eb2dd2cb5dd2bb7dd29bade27bdde26bfdf24c2df22c5df21c7e01fcae01ecde01dcfe11cd2e11bd4e11a"
    "d7e219dae218dce218dfe318e1e318e4e318e7e419e9e419ece41aeee51bf1e51cf3e51ef6e61ff8e621fae622fde724"
)
