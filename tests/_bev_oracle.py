"""Brute-force fp64 numpy restatement of the overlay rule of include/pointnet_refine_hip.h
("Overlays - the rule"): every pixel against every segment of every line.  Used by
test_bev_cpu.py (hand-checked pixels) and test_bev_gpu.py (the oracle of draw_lines)."""
import numpy as np


def coverage(line_px, width, dash, h, w):
    """(h, w) coverage of a polyline given in pixel units ((n,2) columns u, v): the maximum over its
    segments of clamp(width / 2 + 0.5 - d, 0, 1) at the pixel centres, zero where the nearest point
    of the segment is in an 'off' stretch of the dash."""
    cu, cv = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    cov = np.zeros((h, w))
    s0 = 0.0
    for a, b in zip(line_px[:-1], line_px[1:]):
        e = b - a
        len2 = e[0] * e[0] + e[1] * e[1]
        t = np.zeros((h, w))
        if len2 > 0:
            t = np.clip(((cu - a[0]) * e[0] + (cv - a[1]) * e[1]) / len2, 0.0, 1.0)
        du, dv = cu - (a[0] + t * e[0]), cv - (a[1] + t * e[1])
        c = np.clip(0.5 * width + 0.5 - np.sqrt(du * du + dv * dv), 0.0, 1.0)
        if dash is not None and dash[1] > 0:
            c = np.where(np.fmod(s0 + t * np.sqrt(len2), dash[0] + dash[1]) >= dash[0], 0.0, c)
        cov = np.maximum(cov, c)
        s0 += np.sqrt(len2)
    return cov


def draw(canvas, window, lines, styles, resolution):
    """canvas (h, w, 4) uint8 -> a new array with the lines composited in order; returns (image,
    touched mask)."""
    h, w = canvas.shape[:2]
    rgb = canvas[..., :3].astype(np.float64)
    touched = np.zeros((h, w), dtype=bool)
    y_lo, _, _, x_hi = window
    for line, st in zip(lines, styles):
        line = np.asarray(line, dtype=np.float64)
        if len(line) < 2:
            continue
        px = np.stack([(line[:, 1] - y_lo) / resolution, (x_hi - line[:, 0]) / resolution], 1)
        c = coverage(px, st["width"], st.get("dash"), h, w)
        a = (st.get("alpha", 1.0) * c)[..., None]
        rgb = np.where(c[..., None] > 0, rgb * (1.0 - a) + np.array(st["color"], dtype=np.float64) * a, rgb)
        touched |= c > 0
    out = canvas.copy()
    out[..., :3] = np.where(touched[..., None], np.clip(np.rint(rgb), 0, 255), canvas[..., :3]).astype(np.uint8)
    return out, touched
