"""Writes tests/golden/g14_view3d.npz: a small synthetic 3-D view scene (cloud, cameras, lines) and
what tests/_view3d_oracle.py makes of it - depth words after the splat and after the lines, RGBA and
depth.  Nothing here comes from the reference; the data are drawn from a seeded generator.  The
builders are shared with the tests.

    python tests/make_golden_g14_view3d.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _view3d_oracle as O  # noqa: E402

H, W = 33, 47                 # no multiple of 16 or 64
CMIN, CMAX = 1.0, 40.0
N_CLOUD = 5000


def cameras():
    """(3, 16): an oblique perspective camera, an oblique orthographic one, a perspective one
    looking straight down (elev 90).  near of camera 0 is set by cloud() to the depth of point 0."""
    return np.stack([O.camera((0.0, 0.0, 0.0), 60.0, -60.0, 8.0, H, fov=40.0, near=0.5),
                     O.camera((0.5, -0.5, 0.0), 55.0, 20.0, 10.0, H, ortho_scale=5.0, near=0.5),
                     O.camera((0.0, 0.0, 0.0), 90.0, 0.0, 10.0, H, fov=36.0, near=0.25)])


def cloud(dtype, seed=14):
    """(cloud (N_CLOUD, 4) of dtype, cameras (3, 16)).  In order: point 0 lies exactly at d == near
    of camera 0 (near is set to its depth) and point 1 just nearer than that; 40 points behind the
    cameras; 60 far off-screen; 100 pairs at one position with two intensities; the rest uniform
    over a box somewhat larger than the views, so that splats hang over every border.  Intensities
    run from below CMIN to above CMAX."""
    rng = np.random.default_rng(seed)
    cams = cameras()
    eye0, f0 = cams[0, 0:3], cams[0, 9:12]
    special = [eye0 + 2.5 * f0 + 0.3 * cams[0, 3:6], eye0 + 2.4999 * f0 + 0.3 * cams[0, 3:6]]
    behind = [cams[k % 3, 0:3] - rng.uniform(0.5, 3.0) * cams[k % 3, 9:12] + rng.normal(0, 0.5, 3) for k in range(40)]
    off = np.column_stack([rng.uniform(30, 60, 60) * rng.choice([-1, 1], 60), rng.uniform(-60, 60, 60), rng.normal(0, 1, 60)])
    pair = np.column_stack([rng.uniform(-3, 3, 100), rng.uniform(-3, 3, 100), rng.normal(0, 0.2, 100)])
    n_rest = N_CLOUD - 2 - 40 - 60 - 200
    rest = np.column_stack([rng.uniform(-5.0, 5.0, n_rest), rng.uniform(-5.0, 5.0, n_rest), rng.normal(0, 0.3, n_rest)])
    xyz = np.concatenate([np.array(special), np.array(behind), off, np.repeat(pair, 2, axis=0), rest])
    inten = rng.uniform(-5.0, 60.0, len(xyz))
    pts = np.column_stack([xyz, inten]).astype(dtype)
    _, _, d = O.view_space(pts[:1, :3].astype(np.float64), cams[0])
    cams[0, 13] = d[0]
    return pts, cams


def lines_scene(cams=None):
    """(lines, styles, cameras) for the line tests (cams: use these rows instead of cameras()): solid, dashed and marker-only styles, widths 1
    and 4, a zero-length segment, a single vertex, a segment cut by the near plane, one wholly
    behind the cameras, one far larger than the image, and two lines that cross in one plane (equal
    depth under the camera that looks straight down)."""
    cams = cameras() if cams is None else np.array(cams, dtype=np.float64)
    lines = [
        np.array([[-3.0, -2.0, 0.1], [0.0, 0.5, 0.4], [3.0, -1.0, 0.0]]),                      # 0 solid, width 1
        np.array([[-4.0, 2.0, 0.0], [-1.0, 2.5, 0.2], [2.0, 1.5, 0.1], [4.0, 3.0, 0.0]]),      # 1 dashed, width 4
        np.array([[-2.0, -3.0, 0.5], [0.0, -2.0, 0.5], [2.0, -3.0, 0.5]]),                     # 2 markers only
        np.array([[1.0, 1.0, 0.3], [1.0, 1.0, 0.3]]),                                          # 3 zero length
        np.array([[-1.5, 0.0, 1.0]]),                                                          # 4 single vertex
        np.array([[0.0, 0.0, 0.0], cams[0, 0:3] - 1.0 * cams[0, 9:12]]),                       # 5 through camera 0's near plane
        np.array([cams[0, 0:3] - 1.0 * cams[0, 9:12], cams[0, 0:3] - 3.0 * cams[0, 9:12]]),    # 6 behind camera 0
        np.array([[-1000.0, -700.0, 0.0], [1000.0, 702.0, 0.0]]),                              # 7 far larger than the image
        np.array([[-3.0, -3.0, 0.0], [3.0, 3.0, 0.0]]),                                        # 8, 9 cross at equal depth
        np.array([[-3.0, 3.0, 0.0], [3.0, -3.0, 0.0]]),
    ]
    styles = [
        {"color": (10, 200, 30), "width": 1.0, "marker": 0.0, "dash": None, "bias": 0.0},
        {"color": (250, 20, 20), "width": 4.0, "marker": 0.0, "dash": (3.0, 2.0), "bias": 0.0},
        {"color": (255, 0, 255), "width": 0.0, "marker": 5.0, "dash": None, "bias": 0.0},
        {"color": (0, 255, 255), "width": 4.0, "marker": 0.0, "dash": None, "bias": 0.0},
        {"color": (255, 255, 0), "width": 1.0, "marker": 3.0, "dash": None, "bias": 0.0},
        {"color": (255, 165, 0), "width": 1.0, "marker": 2.0, "dash": None, "bias": 0.05},
        {"color": (1, 2, 3), "width": 4.0, "marker": 4.0, "dash": None, "bias": 0.0},
        {"color": (90, 90, 250), "width": 4.0, "marker": 0.0, "dash": (7.0, 3.0), "bias": 0.0},
        {"color": (200, 200, 200), "width": 1.0, "marker": 0.0, "dash": None, "bias": 0.0},
        {"color": (120, 60, 0), "width": 4.0, "marker": 0.0, "dash": None, "bias": 0.0},
    ]
    return lines, styles, cams


def table():
    """A 256-entry colour table that tells every index apart."""
    k = np.arange(256)
    return np.stack([k, 255 - k, (k * 7) % 256, np.full(256, 255)], 1).astype(np.uint8)


def golden(points=None, cams=None):
    """The fixture's arrays.  With the fixture's own points and camera rows given, everything else is
    rebuilt from them: the rows come from sines and cosines, whose last bit may differ between
    math libraries, and nothing downstream of the rows does."""
    if points is None:
        pts, cams = cloud(np.float32)
        pts = pts[:1200]
    else:
        pts, cams = np.asarray(points), np.array(cams, dtype=np.float64)
    z = O.new_zbuffer(3, H, W)
    O.splat(z, pts, cams, 2, CMIN, CMAX)
    splat_words = z.copy()
    lines, styles, lcams = lines_scene(cams)
    segs, ids = O.segments(lines, lcams, H, W)
    O.draw(z, segs, ids, styles, lcams)
    rgba, depth = O.resolve(z, table(), styles, (7, 8, 9))
    return {"points": pts, "cameras": lcams, "splat_words": splat_words, "segments": segs, "segment_ids": ids,
            "words": z, "rgba": rgba, "depth": depth}


if __name__ == "__main__":
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g14_view3d.npz")
    np.savez_compressed(out, **golden())
    print(out, os.path.getsize(out), "bytes")
