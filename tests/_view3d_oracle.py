"""A numpy restatement of the 3-D view rule of include/pointnet_refine_hip.h ("3-D views - the
rule"): camera rows, projection, depth words, splats, line segments and their coverage, resolve.
It shares no code with pointnet_refine_amd.view3d: the product is checked against it word for word.
Everything is fp64 with one rounding per operation, written in the rule's order; the buffers are
numpy uint64 and every write is a minimum."""
import math

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def camera(target, elev, azim, distance, height, fov=None, ortho_scale=None, near=0.1):
    """A camera row from the closed forms; angles in degrees."""
    e, a = math.radians(elev), math.radians(azim)
    out = np.array([math.cos(e) * math.cos(a), math.cos(e) * math.sin(a), math.sin(e)])
    row = np.zeros(16)
    row[0:3] = np.asarray(target, dtype=np.float64) + distance * out
    row[3:6] = [-math.sin(a), math.cos(a), 0.0]
    row[6:9] = [-math.sin(e) * math.cos(a), -math.sin(e) * math.sin(a), math.cos(e)]
    row[9:12] = -out
    row[12] = ortho_scale if ortho_scale is not None else (height / 2.0) / math.tan(math.radians(fov) / 2.0)
    row[13] = near
    row[14] = 0.0 if ortho_scale is None else 1.0
    return row


def view_space(p, cam):
    """(n,3) points -> xr, yu, d."""
    p = np.asarray(p, dtype=np.float64)
    q0, q1, q2 = p[:, 0] - cam[0], p[:, 1] - cam[1], p[:, 2] - cam[2]
    xr = (q0 * cam[3] + q1 * cam[4]) + q2 * cam[5]
    yu = (q0 * cam[6] + q1 * cam[7]) + q2 * cam[8]
    d = (q0 * cam[9] + q1 * cam[10]) + q2 * cam[11]
    return xr, yu, d


def screen(xr, yu, d, cam, h, w):
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.full_like(d, cam[12]) if cam[14] != 0.0 else cam[12] / d
        return w / 2.0 + xr * k, h / 2.0 - yu * k


def words(depth, payload):
    d = np.where(depth > 0.0, depth, 0.0).astype(np.float32)
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(payload).astype(np.uint64)


def new_zbuffer(v, h, w):
    return np.full((v, h, w), EMPTY, dtype=np.uint64)


def lut_index(intensity, cmin, cmax):
    c = np.floor((np.asarray(intensity, dtype=np.float64) - cmin) / (cmax - cmin) * 256.0)
    return np.clip(c, 0.0, 255.0).astype(np.int64)


def splat(zbuf, points, cams, size, cmin, cmax, offsets=None, mask=None):
    """In place.  Returns, per view, (landed: points whose own pixel is in the image, hits (H, W):
    how many points have their own pixel there, tied: pixels decided by the payload)."""
    pts = np.asarray(points)
    v_n, h, w = zbuf.shape
    p = pts[:, :3].astype(np.float64)
    payload = np.uint64(0x01000000) | lut_index(pts[:, 3], cmin, cmax).astype(np.uint64)
    stats = []
    slice_of = None
    if offsets is not None:
        slice_of = np.searchsorted(np.asarray(offsets), np.arange(len(pts)), side="right") - 1
    for v in range(v_n):
        cam = cams[v]
        xr, yu, d = view_space(p, cam)
        ok = d >= cam[13]
        if slice_of is not None:
            ok &= np.asarray(mask)[slice_of, v] != 0
        x, y = screen(xr, yu, d, cam, h, w)
        with np.errstate(invalid="ignore"):
            fx, fy = np.floor(x), np.floor(y)
            ok &= (fx >= -16) & (fx < w + 16) & (fy >= -16) & (fy < h + 16)
        col, row = fx[ok].astype(np.int64), fy[ok].astype(np.int64)
        wd = words(d[ok], payload[ok])
        own = (col >= 0) & (col < w) & (row >= 0) & (row < h)
        hits = np.zeros((h, w), dtype=np.int64)
        np.add.at(hits, (row[own], col[own]), 1)
        before = zbuf[v].copy()
        cand = []
        for i in range(size):
            for j in range(size):
                r, c = row + i - size // 2, col + j - size // 2
                m = (c >= 0) & (c < w) & (r >= 0) & (r < h)
                np.minimum.at(zbuf[v], (r[m], c[m]), wd[m])
                cand.append((r[m], c[m], wd[m]))
        # pixels this call decided by the payload: a losing word with the winner's depth bits
        tied = np.zeros((h, w), dtype=bool)
        for r, c, x in cand:
            won = zbuf[v][r, c]
            lost = (x != won) & ((x >> np.uint64(32)) == (won >> np.uint64(32))) & (won != before[r, c])
            tied[r[lost], c[lost]] = True
        stats.append((int(own.sum()), hits, int(tied.sum())))
    return stats


def style_row(s):
    dash = s.get("dash") or (0.0, 0.0)
    return np.array([s["color"][0], s["color"][1], s["color"][2], s.get("width", 0.0), s.get("marker", 0.0), dash[0],
                     dash[1], s.get("bias", 0.0)], dtype=np.float64)


def segments(lines, cams, h, w, line_views=None):
    """Every (polyline, view) pair cut to d >= near and projected: (segments (n, 8), ids (n, 2))."""
    segs, ids = [], []
    for l, line in enumerate(lines):
        pts = np.asarray(line, dtype=np.float64).reshape(-1, 3)
        views = range(len(cams)) if line_views is None or line_views[l] is None else line_views[l]
        for v in views:
            cam = cams[v]
            near, ortho = cam[13], cam[14] != 0.0
            xr, yu, d = view_space(pts, cam)
            vs = [np.array([xr[i], yu[i], d[i]]) for i in range(len(pts))]
            pairs = [(vs[0], vs[0])] if len(vs) == 1 else [(vs[i], vs[i + 1]) for i in range(len(vs) - 1)]
            arc = 0.0
            for a, b in pairs:
                ina, inb = a[2] >= near, b[2] >= near
                if not ina and not inb:
                    continue
                if ina != inb:
                    t = (near - a[2]) / (b[2] - a[2])
                    c = a + t * (b - a)
                    c[2] = near
                    a, b = (c, b) if not ina else (a, c)
                (ax, ay), (bx, by) = (screen(np.array([e[0]]), np.array([e[1]]), np.array([e[2]]), cam, h, w) for e in (a, b))
                ax, ay, bx, by = float(ax[0]), float(ay[0]), float(bx[0]), float(by[0])
                ex, ey = bx - ax, by - ay
                length = math.sqrt(ex * ex + ey * ey)
                wa, wb = (a[2], b[2]) if ortho else (1.0 / a[2], 1.0 / b[2])
                segs.append([ax, ay, bx, by, arc, length, wa, wb])
                ids.append([l, v])
                arc = arc + length
    return np.array(segs, dtype=np.float64).reshape(-1, 8), np.array(ids, dtype=np.int32).reshape(-1, 2)


def draw(zbuf, segs, ids, styles, cams):
    """In place: every pixel centre of the view is tested against every segment."""
    _, h, w = zbuf.shape
    cx, cy = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    for g, (l, v) in zip(segs, ids):
        st = style_row(styles[l])
        width, marker, on, off, bias = st[3], st[4], st[5], st[6], st[7]
        ortho = cams[v][14] != 0.0
        ax, ay, bx, by, arc, length, wa, wb = g
        depth = np.full((h, w), np.inf)
        hit = np.zeros((h, w), dtype=bool)
        ex, ey = bx - ax, by - ay
        len2 = ex * ex + ey * ey
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if width > 0.0:
                t = np.zeros((h, w))
                if len2 > 0.0:
                    t = np.clip(((cx - ax) * ex + (cy - ay) * ey) / len2, 0.0, 1.0)
                nx, ny = ax + t * ex, ay + t * ey
                dx, dy = cx - nx, cy - ny
                hw = 0.5 * width
                cover = dx * dx + dy * dy <= hw * hw
                if off > 0.0:
                    cover &= ~(np.fmod(arc + t * length, on + off) >= on)
                wt = (1.0 - t) * wa + t * wb
                depth = np.where(cover, wt if ortho else 1.0 / wt, depth)
                hit |= cover
            if marker > 0.0:
                hm = 0.5 * marker
                for px, py, wv in ((ax, ay, wa), (bx, by, wb)):
                    ux, uy = cx - px, cy - py
                    cover = ux * ux + uy * uy <= hm * hm
                    dv = wv if ortho else 1.0 / wv
                    depth = np.where(cover & (~hit | (dv < depth)), dv, depth)
                    hit |= cover
        hit &= ~np.isnan(depth)
        wd = words(depth[hit] - bias, np.full(int(hit.sum()), l))
        zbuf[v][hit] = np.minimum(zbuf[v][hit], wd)
    return zbuf


def resolve(zbuf, table, styles, background=(0, 0, 0)):
    """(rgba uint8 zbuf.shape + (4,), depth float32)."""
    payload = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    bits = (zbuf >> np.uint64(32)).astype(np.uint32)
    empty = zbuf == EMPTY
    is_point = (payload & 0x01000000) != 0
    rgba = np.zeros(zbuf.shape + (4,), dtype=np.uint8)
    rgba[..., :3] = np.asarray(background, dtype=np.uint8)
    rgba[..., 3] = 255
    pt = ~empty & is_point
    rgba[pt] = np.asarray(table, dtype=np.uint8)[payload[pt] & 255]
    rgba[pt, 3] = 255
    ln = ~empty & ~is_point
    if ln.any():
        cols = np.array([s["color"] for s in styles], dtype=np.uint8).reshape(-1, 3)
        rgba[ln, :3] = cols[payload[ln]]
    depth = np.where(empty, np.float32(np.inf), bits.view(np.float32))
    return rgba, depth.astype(np.float32)
